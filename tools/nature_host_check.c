/* Host check of the nature run's argument paths (include/spdy.h, "nature run") on a host-only plan: every rejection of
 * spdy_nature_* in its documented order, the analysis object of another plan and of a destroyed plan, and SPDY_ERR_NO_DEVICE last.
 * Built by `make hostcheck` in speedy.f90_amd with the address and undefined-behaviour sanitizers on the host code of the plan,
 * the analysis and the nature run; exits 0 when every call returns the documented code and text. */
#include <math.h>
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

int main(void)
{
    enum { KX = 5, IX = 96, IY = 24, NMEM = 3 };
    spdy_plan *p = NULL, *other = NULL, *small = NULL, *gone = NULL;
    spdy_nature *n = NULL, *none = NULL;
    spdy_letkf *l = NULL, *lo = NULL, *lg = NULL;
    double x[4];
    double *q = x, *d = NULL;
    long long count = -1;
    CHECK(spdy_plan_create(30, IX, IY, KX, NMEM * (2 * KX + 1), SPDY_DEVICE_NONE, &p) == SPDY_OK);
    CHECK(spdy_plan_create(30, IX, IY, KX, NMEM * (2 * KX + 1), SPDY_DEVICE_NONE, &other) == SPDY_OK);
    CHECK(spdy_plan_create(30, IX, IY, KX, NMEM * (2 * KX + 1), SPDY_DEVICE_NONE, &gone) == SPDY_OK);
    CHECK(spdy_plan_create(30, IX, IY, KX, 2 * KX, SPDY_DEVICE_NONE, &small) == SPDY_OK);
    /* create, in the order of its checks */
    IS(spdy_nature_create(NULL, 1, 2, &n), SPDY_ERR_ARG, "null plan");
    IS(spdy_nature_create(p, 1, 0, &n), SPDY_ERR_ARG, "capacity=0 < 1");
    IS(spdy_nature_create(p, 1, -3, NULL), SPDY_ERR_ARG, "capacity=-3 < 1");
    IS(spdy_nature_create(p, 1, 2, NULL), SPDY_ERR_ARG, "null result pointer");
    IS(spdy_nature_create(small, 1, 2, &n), SPDY_ERR_ARG, "max_batch");
    CHECK(!n && spdy_plan_destroy(small) == SPDY_OK);
    CHECK(spdy_nature_create(p, 0x5EED0123456789ABull, 2, &n) == SPDY_OK && n);
    CHECK(spdy_letkf_create(p, NMEM, 8, &l) == SPDY_OK && spdy_letkf_create(other, NMEM, 8, &lo) == SPDY_OK);
    CHECK(spdy_letkf_create(gone, NMEM, 8, &lg) == SPDY_OK && spdy_plan_destroy(gone) == SPDY_OK);
    /* a null object first, whatever else is wrong */
    IS(spdy_nature_reset(none, 1), SPDY_ERR_ARG, "null nature run");
    IS(spdy_nature_draws(none, NULL), SPDY_ERR_ARG, "null nature run");
    IS(spdy_nature_field(none, NULL, NULL), SPDY_ERR_ARG, "null nature run");
    IS(spdy_nature_set_state_dev(none, NULL, q, q, q, q), SPDY_ERR_ARG, "null nature run");
    IS(spdy_nature_observe_dev(none, NULL, -1.0), SPDY_ERR_ARG, "null nature run");
    IS(spdy_nature_verify_dev(none, NULL, q, q, q, q, q, 9), SPDY_ERR_ARG, "null nature run");
    IS(spdy_nature_verify_grid_dev(none, 0, q, q, q, q, q, 9), SPDY_ERR_ARG, "null nature run");
    /* then the analysis object: null, of a destroyed plan, of another plan */
    IS(spdy_nature_observe_dev(n, NULL, -1.0), SPDY_ERR_ARG, "null analysis object");
    IS(spdy_nature_verify_dev(n, NULL, q, q, q, q, q, 9), SPDY_ERR_ARG, "null analysis object");
    IS(spdy_nature_observe_dev(n, lg, -1.0), SPDY_ERR_STATE, "has been destroyed");
    IS(spdy_nature_verify_dev(n, lg, q, q, q, q, q, 9), SPDY_ERR_STATE, "has been destroyed");
    IS(spdy_nature_observe_dev(n, lo, -1.0), SPDY_ERR_ARG, "another plan");
    IS(spdy_nature_verify_dev(n, lo, q, q, q, q, q, 9), SPDY_ERR_ARG, "another plan");
    /* then the arguments */
    IS(spdy_nature_observe_dev(n, l, -1.0), SPDY_ERR_ARG, "noise must be finite and >= 0");
    IS(spdy_nature_observe_dev(n, l, NAN), SPDY_ERR_ARG, "noise must be finite and >= 0");
    IS(spdy_nature_observe_dev(n, l, INFINITY), SPDY_ERR_ARG, "noise must be finite and >= 0");
    IS(spdy_nature_verify_dev(n, l, NULL, q, q, q, q, 2), SPDY_ERR_ARG, "slot=2 outside [0, capacity=2)");
    IS(spdy_nature_verify_dev(n, l, NULL, q, q, q, q, -1), SPDY_ERR_ARG, "slot=-1 outside");
    IS(spdy_nature_verify_dev(n, l, q, q, NULL, q, q, 1), SPDY_ERR_ARG, "null device pointer");
    IS(spdy_nature_verify_grid_dev(n, 1, q, q, q, q, q, 9), SPDY_ERR_ARG, "nmem=1 outside [2, 32]");
    IS(spdy_nature_verify_grid_dev(n, 33, q, q, q, q, q, 0), SPDY_ERR_ARG, "nmem=33 outside [2, 32]");
    IS(spdy_nature_verify_grid_dev(n, 2, NULL, q, q, q, q, 2), SPDY_ERR_ARG, "slot=2 outside");
    IS(spdy_nature_verify_grid_dev(n, 2, q, q, q, q, NULL, 0), SPDY_ERR_ARG, "null device pointer");
    IS(spdy_nature_set_state_dev(n, q, NULL, q, q, q), SPDY_ERR_ARG, "null device pointer");
    IS(spdy_nature_draws(n, NULL), SPDY_ERR_ARG, "null result pointer");
    IS(spdy_nature_field(n, NULL, &d), SPDY_ERR_ARG, "null name or result pointer");
    IS(spdy_nature_field(n, "truth", NULL), SPDY_ERR_ARG, "null name or result pointer");
    IS(spdy_nature_field(n, "nothing", &d), SPDY_ERR_ARG, "unknown nature field 'nothing'");
    /* and the device last */
    IS(spdy_nature_reset(n, 1), SPDY_ERR_NO_DEVICE, "host-only plan");
    IS(spdy_nature_draws(n, &count), SPDY_ERR_NO_DEVICE, "host-only plan");
    IS(spdy_nature_field(n, "truth", &d), SPDY_ERR_NO_DEVICE, "host-only plan");
    IS(spdy_nature_field(n, "scores", &d), SPDY_ERR_NO_DEVICE, "host-only plan");
    IS(spdy_nature_field(n, "state", &d), SPDY_ERR_NO_DEVICE, "host-only plan");
    IS(spdy_nature_set_state_dev(n, q, q, q, q, q), SPDY_ERR_NO_DEVICE, "host-only plan");
    IS(spdy_nature_observe_dev(n, l, 0.0), SPDY_ERR_NO_DEVICE, "host-only plan");
    IS(spdy_nature_observe_dev(n, l, 1.5), SPDY_ERR_NO_DEVICE, "host-only plan");
    IS(spdy_nature_verify_dev(n, l, q, q, q, q, q, 1), SPDY_ERR_NO_DEVICE, "host-only plan");
    IS(spdy_nature_verify_grid_dev(n, 32, q, q, q, q, q, 0), SPDY_ERR_NO_DEVICE, "host-only plan");
    CHECK(count == -1 && !d);
    /* the nature run's own plan goes first: dead, and says so before it looks at anything else */
    CHECK(spdy_plan_destroy(p) == SPDY_OK);
    IS(spdy_nature_observe_dev(n, NULL, -1.0), SPDY_ERR_STATE, "has been destroyed");
    IS(spdy_nature_verify_grid_dev(n, 0, NULL, q, q, q, q, 9), SPDY_ERR_STATE, "has been destroyed");
    CHECK(spdy_nature_destroy(n) == SPDY_OK && spdy_nature_destroy(NULL) == SPDY_OK);
    CHECK(spdy_letkf_destroy(l) == SPDY_OK && spdy_letkf_destroy(lg) == SPDY_OK && spdy_letkf_destroy(lo) == SPDY_OK);
    CHECK(spdy_plan_destroy(other) == SPDY_OK);
    printf("nature host check ok: every rejection in its order on a host-only plan\n");
    return 0;
}
