/* Host check of the lifetime rule of the objects made on a plan (include/spdy.h, the plan section): a surface model, an SPPT
 * pattern, a diagnostics object, an analysis object and a nature run on a host-only plan, in both teardown orders; every entry point on a dead
 * handle; creates that fail after the object has joined its plan; and 100 create/destroy rounds on one plan.  Built by
 * `make hostcheck` in speedy.f90_amd with the address and undefined-behaviour sanitizers on the host code of the plan and of the
 * five kinds; exits 0 when every call returns the documented code, and the sanitizers' leak check sees whether an object stayed
 * on its plan. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spdy.h"

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "line %d: %s -- %s\n", __LINE__, #cond, spdy_last_error()); \
            return 1;                                                        \
        }                                                                    \
    } while (0)
/* a call on a dead handle: SPDY_ERR_STATE, and the message names the destroyed plan */
#define DEAD(call) CHECK((call) == SPDY_ERR_STATE && strstr(spdy_last_error(), "has been destroyed"))

enum { KX = 8, IX = 96, IY = 24, NCOL = IX * 2 * IY, MAX_BATCH = 64, NMEM = 2 };

static double fields[12 * NCOL];      /* every climatology: 0.5 everywhere (a land fraction, an albedo, twelve months of anything) */
static const spdy_surface_clim clim = {fields, fields, fields, fields, fields, fields, fields, fields};

typedef struct {
    spdy_surface_model *m;
    spdy_sppt *s;
    spdy_diagnostics *d, *d1;         /* NMEM members; one member, for the calls that take no member */
    spdy_letkf *l;
    spdy_nature *n;
} objects;

static int create(spdy_plan *p, objects *o)
{
    const unsigned long long seeds[NMEM] = {1, 2};
    CHECK(spdy_ens_surface_model_create(p, NMEM, &clim, 2400.0, SPDY_SURFACE_DEFAULT, &o->m) == SPDY_OK);
    CHECK(spdy_ens_sppt_create(p, NMEM, 36, NULL, seeds, &o->s) == SPDY_OK);
    CHECK(spdy_ens_diagnostics_create(p, NMEM, 4, 0, &o->d) == SPDY_OK && spdy_diagnostics_create(p, 4, 0, &o->d1) == SPDY_OK);
    CHECK(spdy_letkf_create(p, NMEM, 4, &o->l) == SPDY_OK && spdy_letkf_set_localization(o->l, 1.0e6, 0.0, 1.0) == SPDY_OK);
    CHECK(spdy_nature_create(p, 7, 2, &o->n) == SPDY_OK);
    return 0;
}

static int destroy(objects *o)
{
    CHECK(spdy_surface_model_destroy(o->m) == SPDY_OK && spdy_sppt_destroy(o->s) == SPDY_OK);
    CHECK(spdy_diagnostics_destroy(o->d) == SPDY_OK && spdy_diagnostics_destroy(o->d1) == SPDY_OK);
    CHECK(spdy_letkf_destroy(o->l) == SPDY_OK && spdy_nature_destroy(o->n) == SPDY_OK);
    return 0;
}

/* every entry point but _destroy, with arguments that pass every check but the device's while the plan lives */
static int every_call(const objects *o, int want)
{
    int bad = 0;                          /* every failing call is reported, not only the first */
#define CALL(call)                                                                                                   \
    do {                                                                                                             \
        const int rc_ = (call);                                                                                      \
        if (want == SPDY_ERR_STATE ? !(rc_ == want && strstr(spdy_last_error(), "has been destroyed")) : !(rc_ >= 0 || rc_ == want)) { \
            fprintf(stderr, "line %d: %s returned %d, expected %d -- %s\n", __LINE__, #call, rc_, want, spdy_last_error()); \
            ++bad;                                                                                                   \
        }                                                                                                            \
    } while (0)
    double x[3 * KX];
    double *q = x, *ptr = NULL;
    const double *cptr = NULL;
    void *vptr = NULL;
    long long a = 0, b = 0, both[NMEM];
    int i = 0, j = 0;
    spdy_sfc_boundary bnd;
    const spdy_obs obs = {SPDY_OBS_T, 3, 10.0, 20.0, 250.0, 1.0};
    CALL(spdy_surface_model_members(o->m, NULL));
    CALL(spdy_surface_model_table(o->m, "fmask_l", NULL, 0));
    CALL(spdy_surface_model_set_date(o->m, 1, 0.5, 0.04));
    CALL(spdy_surface_model_set_sst_anomaly(o->m, fields));
    CALL(spdy_surface_model_couple_dev(o->m, 0, NULL, NULL, NULL, NULL));
    CALL(spdy_surface_model_forcing_dev(o->m, q));
    CALL(spdy_surface_model_boundary(o->m, &bnd, &cptr));
    CALL(spdy_surface_model_field(o->m, "sst_am", &ptr));
    CALL(spdy_sppt_members(o->s));
    CALL(spdy_sppt_reset(o->s, 7));
    CALL(spdy_ens_sppt_reset(o->s, 1, 7));
    CALL(spdy_sppt_table(o->s, "sigma", NULL, 0));
    CALL(spdy_sppt_field(o->s, "pattern", &ptr));
    CALL(spdy_sppt_draws(o->s, &a));
    CALL(spdy_ens_sppt_draws(o->s, 1, &a));
    CALL(spdy_sppt_advance_dev(o->s, NULL));
    CALL(spdy_diagnostics_set_limits(o->d, NULL));
    CALL(spdy_diagnostics_reset(o->d, 0));
    CALL(spdy_diagnostics_check_dev(o->d, q, q, q));
    CALL(spdy_diagnostics_status(o->d1, &a, &b, &i, &j, x));
    CALL(spdy_ens_diagnostics_status(o->d, 1, &a, &b, &i, &j, x));
    CALL(spdy_diagnostics_read(o->d1, 0, 1, x));
    CALL(spdy_ens_diagnostics_read(o->d, 1, 0, 1, x));
    CALL(spdy_ens_diagnostics_stopped(o->d, both));
    CALL(spdy_diagnostics_field(o->d, "history", &vptr));
    CALL(spdy_letkf_set_localization(o->l, 1.0e6, 0.0, 1.0));
    CALL(spdy_letkf_set_obs(o->l, 1, &obs));
    CALL(spdy_letkf_set_weight_stride(o->l, 2, 2));
    CALL(spdy_letkf_table(o->l, "unit", NULL, 0));
    CALL(spdy_letkf_field(o->l, "hx", &ptr));
    CALL(spdy_letkf_analyse_grid_dev(o->l, q, q, q, q, q, q, q, q, q, q));
    CALL(spdy_ens_letkf_dev(o->l, q, q, q, q, q));
    CALL(spdy_nature_reset(o->n, 7));
    CALL(spdy_nature_draws(o->n, &a));
    CALL(spdy_nature_field(o->n, "truth", &ptr));
    CALL(spdy_nature_set_state_dev(o->n, q, q, q, q, q));
    CALL(spdy_nature_observe_dev(o->n, o->l, 1.0));
    CALL(spdy_nature_verify_dev(o->n, o->l, q, q, q, q, q, 1));
    CALL(spdy_nature_verify_grid_dev(o->n, NMEM, q, q, q, q, q, 1));
#undef CALL
    return bad;
}

int main(void)
{
    spdy_plan *p = NULL, *small = NULL;
    objects o;
    for (int n = 0; n < 12 * NCOL; ++n) fields[n] = 0.5;
    /* the objects first, then the plan */
    CHECK(spdy_plan_create(30, IX, IY, KX, MAX_BATCH, SPDY_DEVICE_NONE, &p) == SPDY_OK);
    if (create(p, &o) || every_call(&o, SPDY_ERR_NO_DEVICE) || destroy(&o)) return 1;
    CHECK(spdy_plan_destroy(p) == SPDY_OK);
    /* the plan first: the handles are dead, every call says so, _destroy frees them */
    CHECK(spdy_plan_create(30, IX, IY, KX, MAX_BATCH, SPDY_DEVICE_NONE, &p) == SPDY_OK);
    if (create(p, &o)) return 1;
    CHECK(spdy_letkf_set_weight_stride(o.l, 3, 5) == SPDY_OK);
    CHECK(spdy_plan_destroy(p) == SPDY_OK);
    if (every_call(&o, SPDY_ERR_STATE)) return 1;
    /* a dead pattern in the physics calls of a live plan */
    CHECK(spdy_plan_create(30, IX, IY, KX, MAX_BATCH, SPDY_DEVICE_NONE, &p) == SPDY_OK);
    CHECK(spdy_radiation_set_date(p, 0.0) == SPDY_OK && spdy_surface_set_orography(p, fields) == SPDY_OK);
    {
        double *q = fields;
        const spdy_sfc_boundary bnd = {q, q, q, q, q, q, q};
        DEAD(spdy_ens_physics_sppt_dev(p, NMEM, o.s, 1, q, q, q, q, q, q, &bnd, q, q, q, q, q, q, NULL));
    }
    /* a live nature run with the analysis object of the destroyed plan */
    {
        spdy_nature *live = NULL;
        CHECK(spdy_nature_create(p, 7, 1, &live) == SPDY_OK);
        DEAD(spdy_nature_observe_dev(live, o.l, 1.0));
        DEAD(spdy_nature_verify_dev(live, o.l, fields, fields, fields, fields, fields, 0));
        CHECK(spdy_nature_destroy(live) == SPDY_OK);
    }
    if (destroy(&o)) return 1;
    /* creates that fail after the object has joined its plan */
    spdy_sppt *s = NULL;
    spdy_surface_model *m = NULL;
    spdy_letkf *l = NULL;
    const unsigned long long seed = 1;
    CHECK(spdy_ens_sppt_create(p, 1, 0, NULL, &seed, &s) == SPDY_ERR_ARG && !s);
    CHECK(spdy_surface_model_create(p, &clim, 0.0, SPDY_SURFACE_DEFAULT, &m) == SPDY_ERR_ARG && !m);
    CHECK(spdy_plan_create(30, IX, IY, KX, NMEM * (2 * KX + 1) - 1, SPDY_DEVICE_NONE, &small) == SPDY_OK);
    CHECK(spdy_letkf_create(small, NMEM, 4, &l) == SPDY_ERR_ARG && !l && spdy_plan_destroy(small) == SPDY_OK);
    /* null handles keep their code and text */
    CHECK(spdy_surface_model_members(NULL, NULL) == SPDY_ERR_ARG && !strcmp(spdy_last_error(), "null surface model"));
    CHECK(spdy_sppt_members(NULL) == SPDY_ERR_ARG && !strcmp(spdy_last_error(), "null SPPT pattern"));
    CHECK(spdy_diagnostics_reset(NULL, 0) == SPDY_ERR_ARG && !strcmp(spdy_last_error(), "null diagnostics object"));
    CHECK(spdy_letkf_table(NULL, "unit", NULL, 0) == SPDY_ERR_ARG && !strcmp(spdy_last_error(), "null analysis object"));
    CHECK(spdy_nature_reset(NULL, 7) == SPDY_ERR_ARG && !strcmp(spdy_last_error(), "null nature run"));
    {
        spdy_nature *n = NULL;
        CHECK(spdy_nature_create(p, 7, 0, &n) == SPDY_ERR_ARG && !n);
    }
    /* 100 rounds on the plan the failed creates left: an object that stayed on the plan's list would be written to at the end */
    for (int r = 0; r < 100; ++r)
        if (create(p, &o) || destroy(&o)) return 1;
    if (create(p, &o)) return 1;
    CHECK(spdy_plan_destroy(p) == SPDY_OK);
    if (every_call(&o, SPDY_ERR_STATE) || destroy(&o)) return 1;
    printf("object lifetime check ok: 5 kinds, both teardown orders, 100 rounds\n");
    return 0;
}
