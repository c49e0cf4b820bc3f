/* Host check of observations in time slots (include/spdy.h, "ensemble analysis, observations in time slots") on a host-only plan:
 * every rejection of spdy_slot_set in its documented order, a rejected call changes nothing, the table "slot_first", the reset by
 * spdy_letkf_set_obs and spdy_pobs_set, the check order of every *_dev call up to SPDY_ERR_NO_DEVICE, and the lifetime rule on a
 * destroyed plan.  Built by `make hostcheck` in speedy.f90_amd with the address and undefined-behaviour sanitizers on the host
 * code of the plan, the analysis and the nature run; exits 0 when every call returns the documented code and text. */
#include <stdio.h>
#include <string.h>

#include "spdy.h"

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "line %d: %s -- %s\n", __LINE__, #cond, spdy_last_error()); \
            return 1;                                                        \
        }                                                                    \
    } while (0)
#define IS(call, code, text) CHECK((call) == (code) && strstr(spdy_last_error(), text))

enum { KX = 5, IX = 96, IY = 24, NMEM = 3, MAXOBS = 6 };

static int slots_are(spdy_letkf *l, const int *first, int n)
{
    double buf[SPDY_MAX_SLOTS + 1];
    if (spdy_letkf_table(l, "slot_first", buf, SPDY_MAX_SLOTS + 1) != n) return 0;
    for (int s = 0; s < n; ++s)
        if (buf[s] != (double)first[s]) return 0;
    return 1;
}

int main(void)
{
    spdy_plan *p = NULL, *gone = NULL, *other = NULL;
    spdy_letkf *l = NULL, *lg = NULL, *lo = NULL;
    spdy_nature *n = NULL;
    double mem[4] = {0.0, 0.0, 0.0, 0.0}, *q = mem, *d = NULL;      /* a non-null "device pointer": no check dereferences one */
    const spdy_obs obs[5] = {{SPDY_OBS_T, 1, 10.0, 5.0, 1.0, 1.0}, {SPDY_OBS_PS, 0, 20.0, -5.0, 2.0, 0.5}, {SPDY_OBS_U, 2, 30.0, 0.0, 3.0, 2.0},
                             {SPDY_OBS_V, 4, 40.0, 50.0, 3.0, 2.0}, {SPDY_OBS_Q, 0, 50.0, -60.0, 3.0, 2.0}};
    const spdy_pobs pobs[2] = {{SPDY_OBS_T, SPDY_OBS_AT_P, 50000.0, 10.0, 5.0, 1.0, 1.0}, {SPDY_OBS_U, 2, -1.0, 30.0, 0.0, 3.0, 2.0}};
    const int three[4] = {0, 2, 2, 5}, late[4] = {1, 2, 2, 5}, back[4] = {0, 3, 2, 5}, shrt[4] = {0, 2, 2, 4}, lng[4] = {0, 2, 2, 6};
    const int one[2] = {0, 5}, two[3] = {0, 1, 2}, none[3] = {0, 0, 0};
    int many[SPDY_MAX_SLOTS + 2];
    CHECK(spdy_plan_create(30, IX, IY, KX, NMEM * (2 * KX + 1), SPDY_DEVICE_NONE, &p) == SPDY_OK);
    CHECK(spdy_plan_create(30, IX, IY, KX, NMEM * (2 * KX + 1), SPDY_DEVICE_NONE, &gone) == SPDY_OK);
    CHECK(spdy_plan_create(30, IX, IY, KX, NMEM * (2 * KX + 1), SPDY_DEVICE_NONE, &other) == SPDY_OK);
    CHECK(spdy_letkf_create(p, NMEM, MAXOBS, &l) == SPDY_OK && spdy_letkf_create(gone, NMEM, MAXOBS, &lg) == SPDY_OK);
    CHECK(spdy_letkf_create(other, NMEM, MAXOBS, &lo) == SPDY_OK && spdy_nature_create(p, 7ull, 1, &n) == SPDY_OK);
    CHECK(spdy_plan_destroy(gone) == SPDY_OK);
    CHECK(spdy_letkf_set_obs(l, 5, obs) == SPDY_OK && spdy_letkf_table(l, "slot_first", NULL, 0) == 0);
    /* spdy_slot_set: the rejections in the order of the checks; each later argument is invalid too */
    IS(spdy_slot_set(NULL, 99, NULL), SPDY_ERR_ARG, "null analysis object");
    IS(spdy_slot_set(lg, 99, NULL), SPDY_ERR_STATE, "has been destroyed");
    IS(spdy_slot_set(l, -1, NULL), SPDY_ERR_ARG, "slot_set: nslots=-1 outside [0, 32]");
    IS(spdy_slot_set(l, SPDY_MAX_SLOTS + 1, NULL), SPDY_ERR_ARG, "slot_set: nslots=33 outside [0, 32]");
    IS(spdy_slot_set(l, 3, NULL), SPDY_ERR_ARG, "slot_set: null ranges");
    IS(spdy_slot_set(l, 3, late), SPDY_ERR_ARG, "slot_set: first[0]=1 must be 0");
    IS(spdy_slot_set(l, 3, back), SPDY_ERR_ARG, "slot_set: first[2]=2 < first[1]=3");
    IS(spdy_slot_set(l, 3, shrt), SPDY_ERR_ARG, "slot_set: first[3]=4 must be nobs=5");
    IS(spdy_slot_set(l, 3, lng), SPDY_ERR_ARG, "slot_set: first[3]=6 must be nobs=5");
    CHECK(spdy_letkf_table(l, "slot_first", NULL, 0) == 0);
    CHECK(spdy_slot_set(l, 3, three) == SPDY_OK && slots_are(l, three, 4));
    IS(spdy_slot_set(l, 3, back), SPDY_ERR_ARG, "slot_set: first[2]=2 < first[1]=3");
    CHECK(slots_are(l, three, 4));                                   /* a rejected call changes nothing */
    IS(spdy_letkf_table(l, "slot_first", mem, 3), SPDY_ERR_ARG, "analysis table 'slot_first' has 4 values, the buffer 3");
    for (int s = 0; s <= SPDY_MAX_SLOTS + 1; ++s) many[s] = s < SPDY_MAX_SLOTS ? 0 : 5;
    CHECK(spdy_slot_set(l, SPDY_MAX_SLOTS, many) == SPDY_OK && slots_are(l, many, SPDY_MAX_SLOTS + 1));
    CHECK(spdy_slot_set(l, 0, NULL) == SPDY_OK && spdy_letkf_table(l, "slot_first", NULL, 0) == 0);
    CHECK(spdy_slot_set(l, 0, late) == SPDY_OK && spdy_letkf_table(l, "slot_first", NULL, 0) == 0);      /* first is not read */
    /* a new network returns the object to no slots; a rejected set does not */
    CHECK(spdy_slot_set(l, 1, one) == SPDY_OK && slots_are(l, one, 2));
    IS(spdy_letkf_set_obs(l, MAXOBS + 1, obs), SPDY_ERR_ARG, "nobs=7 outside");
    CHECK(slots_are(l, one, 2));
    CHECK(spdy_letkf_set_obs(l, 5, obs) == SPDY_OK && spdy_letkf_table(l, "slot_first", NULL, 0) == 0);
    CHECK(spdy_slot_set(l, 1, one) == SPDY_OK && spdy_pobs_set(l, 2, pobs) == SPDY_OK && spdy_letkf_table(l, "slot_first", NULL, 0) == 0);
    IS(spdy_slot_set(l, 1, one), SPDY_ERR_ARG, "slot_set: first[1]=5 must be nobs=2");
    CHECK(spdy_slot_set(l, 2, two) == SPDY_OK && slots_are(l, two, 3));
    CHECK(spdy_letkf_set_obs(l, 0, NULL) == SPDY_OK && spdy_letkf_table(l, "slot_first", NULL, 0) == 0);
    CHECK(spdy_slot_set(l, 2, none) == SPDY_OK && slots_are(l, none, 3));
    CHECK(spdy_letkf_set_obs(l, 5, obs) == SPDY_OK && spdy_letkf_set_localization(l, 5.0e5, 0.1, 1.1) == SPDY_OK);
    /* the observe calls: the object, no slots, the slot, a pointer, the device */
    IS(spdy_slot_observe_grid_dev(NULL, -1, NULL, q, q, q, q), SPDY_ERR_ARG, "null analysis object");
    IS(spdy_slot_observe_dev(NULL, -1, NULL, q, q, q, q), SPDY_ERR_ARG, "null analysis object");
    IS(spdy_slot_observe_grid_dev(lg, -1, NULL, q, q, q, q), SPDY_ERR_STATE, "has been destroyed");
    IS(spdy_slot_observe_dev(lg, -1, NULL, q, q, q, q), SPDY_ERR_STATE, "has been destroyed");
    IS(spdy_slot_observe_grid_dev(l, -1, NULL, q, q, q, q), SPDY_ERR_STATE, "slot_observe: spdy_slot_set first");
    IS(spdy_slot_observe_dev(l, -1, NULL, q, q, q, q), SPDY_ERR_STATE, "slot_observe: spdy_slot_set first");
    CHECK(spdy_slot_set(l, 3, three) == SPDY_OK);
    IS(spdy_slot_observe_grid_dev(l, -1, NULL, q, q, q, q), SPDY_ERR_ARG, "slot_observe: slot=-1 outside [0, nslots=3)");
    IS(spdy_slot_observe_dev(l, 3, NULL, q, q, q, q), SPDY_ERR_ARG, "slot_observe: slot=3 outside [0, nslots=3)");
    IS(spdy_slot_observe_grid_dev(l, 0, q, q, NULL, q, q), SPDY_ERR_ARG, "null device pointer");
    IS(spdy_slot_observe_dev(l, 1, q, q, q, q, NULL), SPDY_ERR_ARG, "null device pointer");
    for (int s = 0; s < 3; ++s) {
        IS(spdy_slot_observe_grid_dev(l, s, q, q, q, q, q), SPDY_ERR_NO_DEVICE, "host-only plan");
        IS(spdy_slot_observe_dev(l, s, q, q, q, q, q), SPDY_ERR_NO_DEVICE, "host-only plan");
    }
    /* the analysis calls: the plain forms' checks, then the slots, then the device */
    IS(spdy_slot_analyse_grid_dev(NULL, NULL, q, q, q, q, q, q, q, q, q, NULL), SPDY_ERR_ARG, "null analysis object");
    IS(spdy_slot_ens_letkf_dev(NULL, NULL, q, q, q, q, NULL), SPDY_ERR_ARG, "null analysis object");
    IS(spdy_slot_analyse_grid_dev(lg, NULL, q, q, q, q, q, q, q, q, q, NULL), SPDY_ERR_STATE, "has been destroyed");
    IS(spdy_slot_ens_letkf_dev(lg, NULL, q, q, q, q, NULL), SPDY_ERR_STATE, "has been destroyed");
    IS(spdy_slot_analyse_grid_dev(lo, NULL, q, q, q, q, q, q, q, q, q, NULL), SPDY_ERR_STATE, "spdy_letkf_set_localization first");
    IS(spdy_slot_ens_letkf_dev(lo, NULL, q, q, q, q, NULL), SPDY_ERR_STATE, "spdy_letkf_set_localization first");
    IS(spdy_slot_analyse_grid_dev(l, q, q, q, q, q, q, q, q, q, NULL, NULL), SPDY_ERR_ARG, "null device pointer");
    IS(spdy_slot_ens_letkf_dev(l, NULL, q, q, q, q, NULL), SPDY_ERR_ARG, "null device pointer");
    IS(spdy_slot_analyse_grid_dev(l, q, q, q, q, q, q, q, q, q, q, NULL), SPDY_ERR_STATE, "slot analysis: slot 0 has not been observed");
    IS(spdy_slot_ens_letkf_dev(l, q, q, q, q, q, (const int *)q), SPDY_ERR_STATE, "slot analysis: slot 0 has not been observed");
    CHECK(spdy_slot_set(l, 0, NULL) == SPDY_OK);
    IS(spdy_slot_analyse_grid_dev(l, q, q, q, q, q, q, q, q, q, q, NULL), SPDY_ERR_STATE, "slot analysis: spdy_slot_set first");
    IS(spdy_slot_ens_letkf_dev(l, q, q, q, q, q, NULL), SPDY_ERR_STATE, "slot analysis: spdy_slot_set first");
    /* no observation: every slot is empty, nothing has to be observed, the device is all that is missing */
    CHECK(spdy_letkf_set_obs(l, 0, NULL) == SPDY_OK && spdy_slot_set(l, 2, none) == SPDY_OK);
    IS(spdy_slot_analyse_grid_dev(l, q, q, q, q, q, q, q, q, q, q, NULL), SPDY_ERR_NO_DEVICE, "host-only plan");
    IS(spdy_slot_ens_letkf_dev(l, q, q, q, q, q, NULL), SPDY_ERR_NO_DEVICE, "host-only plan");
    /* the nature call: spdy_nature_observe_dev's checks, the slots, the device */
    CHECK(spdy_letkf_set_obs(l, 5, obs) == SPDY_OK);
    IS(spdy_slot_nature_observe_dev(NULL, NULL, -1, -1.0), SPDY_ERR_ARG, "null nature run");
    IS(spdy_slot_nature_observe_dev(n, NULL, -1, -1.0), SPDY_ERR_ARG, "null analysis object");
    IS(spdy_slot_nature_observe_dev(n, lg, -1, -1.0), SPDY_ERR_STATE, "has been destroyed");
    IS(spdy_slot_nature_observe_dev(n, lo, -1, -1.0), SPDY_ERR_ARG, "belongs to another plan");
    IS(spdy_slot_nature_observe_dev(n, l, -1, -1.0), SPDY_ERR_ARG, "slot_nature_observe: noise must be finite and >= 0");
    IS(spdy_slot_nature_observe_dev(n, l, -1, 1.0), SPDY_ERR_STATE, "slot_nature_observe: spdy_slot_set first");
    CHECK(spdy_slot_set(l, 3, three) == SPDY_OK);
    IS(spdy_slot_nature_observe_dev(n, l, -1, 1.0), SPDY_ERR_ARG, "slot_nature_observe: slot=-1 outside [0, nslots=3)");
    IS(spdy_slot_nature_observe_dev(n, l, 3, 1.0), SPDY_ERR_ARG, "slot_nature_observe: slot=3 outside [0, nslots=3)");
    for (int s = 0; s < 3; ++s) IS(spdy_slot_nature_observe_dev(n, l, s, 0.0), SPDY_ERR_NO_DEVICE, "host-only plan");
    /* the device fields exist by name and need a device */
    IS(spdy_letkf_field(l, "slot_ps", &d), SPDY_ERR_NO_DEVICE, "host-only plan");
    IS(spdy_letkf_field(l, "slot_out", &d), SPDY_ERR_NO_DEVICE, "host-only plan");
    CHECK(!d);
    /* the lifetime rule: the object outlives its plan as a dead handle */
    CHECK(spdy_nature_destroy(n) == SPDY_OK && spdy_letkf_destroy(lg) == SPDY_OK && spdy_letkf_destroy(lo) == SPDY_OK);
    CHECK(spdy_plan_destroy(other) == SPDY_OK && spdy_plan_destroy(p) == SPDY_OK);
    IS(spdy_slot_set(l, 3, three), SPDY_ERR_STATE, "has been destroyed");
    IS(spdy_slot_observe_dev(l, 0, q, q, q, q, q), SPDY_ERR_STATE, "has been destroyed");
    IS(spdy_slot_ens_letkf_dev(l, q, q, q, q, q, NULL), SPDY_ERR_STATE, "has been destroyed");
    IS(spdy_letkf_table(l, "slot_first", NULL, 0), SPDY_ERR_STATE, "has been destroyed");
    CHECK(spdy_letkf_destroy(l) == SPDY_OK);
    printf("slot host check ok: every rejection in its order, the ranges, their reset and the lifetime rule on a host-only plan\n");
    return 0;
}
