/* Host check of observations given at a pressure (include/spdy.h, "ensemble analysis, observations at a pressure") on a host-only
 * plan: every rejection of spdy_pobs_set in its documented order, a rejected call changes no table, the tables of a mixed set and
 * of a set without pressures, spdy_letkf_set_obs after it, and the lifetime rule on a destroyed plan.  Built by `make hostcheck`
 * in speedy.f90_amd with the address and undefined-behaviour sanitizers on the host code of the plan and the analysis; exits 0
 * when every call returns the documented code and text. */
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

enum { KX = 5, IX = 96, IY = 24, NMEM = 3, MAXOBS = 4 };

static int same_tables(spdy_letkf *l, const double *lns, const double *lnp, const double *w, int n)
{
    double a[MAXOBS], b[MAXOBS], c[4 * MAXOBS];
    if (spdy_letkf_table(l, "lnsigma", a, MAXOBS) != n || spdy_letkf_table(l, "lnp", b, MAXOBS) != n ||
        spdy_letkf_table(l, "stencil_weight", c, 4 * MAXOBS) != 4 * n)
        return 0;
    return !memcmp(a, lns, sizeof(double) * n) && !memcmp(b, lnp, sizeof(double) * n) && !memcmp(c, w, sizeof(double) * 4 * n);
}

int main(void)
{
    spdy_plan *p = NULL, *flat = NULL, *gone = NULL;
    spdy_letkf *l = NULL, *l1 = NULL, *lg = NULL;
    const double sigma1[2] = {0.0, 1.0};
    double fsg[KX], lns[MAXOBS], lnp[MAXOBS], w[4 * MAXOBS], buf[4 * MAXOBS];
    /* T at 500 hPa; PS, whose lev and p are ignored; U on level 2, whose p is ignored */
    const spdy_pobs good[3] = {{SPDY_OBS_T, SPDY_OBS_AT_P, 50000.0, 10.0, 5.0, 1.0, 1.0}, {SPDY_OBS_PS, SPDY_OBS_AT_P, NAN, 20.0, -5.0, 2.0, 0.5},
                               {SPDY_OBS_U, 2, -1.0, 30.0, 0.0, 3.0, 2.0}};
    const spdy_obs plain[2] = {{SPDY_OBS_T, 1, 10.0, 5.0, 1.0, 1.0}, {SPDY_OBS_PS, 99, 20.0, -5.0, 2.0, 0.5}};
    spdy_pobs same[2], bad[2], many[MAXOBS + 1];
    CHECK(spdy_plan_create(30, IX, IY, KX, NMEM * (2 * KX + 1), SPDY_DEVICE_NONE, &p) == SPDY_OK);
    CHECK(spdy_plan_create(30, IX, IY, KX, NMEM * (2 * KX + 1), SPDY_DEVICE_NONE, &gone) == SPDY_OK);
    CHECK(spdy_letkf_create(p, NMEM, MAXOBS, &l) == SPDY_OK && spdy_letkf_create(gone, NMEM, MAXOBS, &lg) == SPDY_OK);
    CHECK(spdy_get_table(p, "fsg", fsg, KX) == KX);
    /* a mixed set and its tables */
    CHECK(spdy_pobs_set(l, 3, good) == SPDY_OK);
    CHECK(spdy_letkf_table(l, "lnsigma", lns, MAXOBS) == 3 && spdy_letkf_table(l, "lnp", lnp, MAXOBS) == 3);
    CHECK(spdy_letkf_table(l, "stencil_weight", w, 4 * MAXOBS) == 12 && spdy_letkf_table(l, "rinv", buf, MAXOBS) == 3);
    CHECK(lnp[0] == log(50000.0 / 1.0e5) && lnp[1] == 0.0 && lnp[2] == 0.0);
    CHECK(lns[0] == lnp[0] && lns[1] == 0.0 && lns[2] == log(fsg[2]));
    CHECK(buf[0] == 1.0 && buf[1] == 4.0 && buf[2] == 0.25);
    /* the rejections, in the order of the checks; each later field is invalid too */
    IS(spdy_pobs_set(NULL, -1, NULL), SPDY_ERR_ARG, "null analysis object");
    IS(spdy_pobs_set(l, -1, NULL), SPDY_ERR_ARG, "pobs_set: nobs=-1 outside [0, max_obs=4]");
    memset(many, 0, sizeof(many));
    IS(spdy_pobs_set(l, MAXOBS + 1, many), SPDY_ERR_ARG, "nobs=5 outside");
    IS(spdy_pobs_set(l, 2, NULL), SPDY_ERR_ARG, "null observations");
    bad[0] = good[0];
#define BAD(field, value, text)                                                   \
    do {                                                                          \
        bad[1] = good[0];                                                         \
        bad[1].error = -1.0;                                                      \
        bad[1].field = (value);                                                   \
        IS(spdy_pobs_set(l, 2, bad), SPDY_ERR_ARG, "pobs_set: observation 1: " text); \
    } while (0)
    BAD(var, 5, "var=5");
    BAD(var, -1, "var=-1");
    BAD(lev, KX, "lev=5 outside [0, 5)");
    BAD(lev, -2, "lev=-2 outside");
    BAD(p, 0.0, "p must be finite and > 0");
    BAD(p, -50000.0, "p must be finite and > 0");
    BAD(p, NAN, "p must be finite and > 0");
    BAD(p, INFINITY, "p must be finite and > 0");
    BAD(lon, INFINITY, "lon is not finite");
    BAD(lat, 90.5, "lat outside [-90, 90]");
    BAD(value, NAN, "value is not finite");
    BAD(error, 0.0, "error must be finite and > 0");
    CHECK(same_tables(l, lns, lnp, w, 3));
    /* one level: no bracket exists; a model-level observation is taken */
    CHECK(spdy_plan_create(30, IX, IY, 1, 8, SPDY_DEVICE_NONE, &flat) == SPDY_OK && spdy_plan_set_sigma(flat, sigma1) == SPDY_OK);
    CHECK(spdy_letkf_create(flat, 2, MAXOBS, &l1) == SPDY_OK);
    IS(spdy_pobs_set(l1, 1, good), SPDY_ERR_ARG, "needs kx >= 2");
    bad[0].lev = 0;
    CHECK(spdy_pobs_set(l1, 1, bad) == SPDY_OK && spdy_letkf_table(l1, "lnp", buf, MAXOBS) == 1 && buf[0] == 0.0);
    /* without a pressure the tables are set_obs', and set_obs empties "lnp" */
    same[0] = (spdy_pobs){plain[0].var, plain[0].lev, NAN, plain[0].lon, plain[0].lat, plain[0].value, plain[0].error};
    same[1] = (spdy_pobs){plain[1].var, plain[1].lev, -1.0, plain[1].lon, plain[1].lat, plain[1].value, plain[1].error};
    CHECK(spdy_pobs_set(l, 2, same) == SPDY_OK);
    CHECK(spdy_letkf_table(l, "lnsigma", lns, MAXOBS) == 2 && spdy_letkf_table(l, "stencil_weight", w, 4 * MAXOBS) == 8);
    CHECK(spdy_letkf_table(l, "lnp", lnp, MAXOBS) == 2 && lnp[0] == 0.0 && lnp[1] == 0.0);
    CHECK(spdy_letkf_set_obs(l, 2, plain) == SPDY_OK && spdy_letkf_table(l, "lnp", NULL, 0) == 0);
    CHECK(spdy_letkf_table(l, "lnsigma", buf, MAXOBS) == 2 && !memcmp(buf, lns, 2 * sizeof(double)));
    CHECK(spdy_letkf_table(l, "stencil_weight", buf, 4 * MAXOBS) == 8 && !memcmp(buf, w, 8 * sizeof(double)));
    CHECK(spdy_pobs_set(l, 0, NULL) == SPDY_OK && spdy_letkf_table(l, "lnp", NULL, 0) == 0 && spdy_letkf_table(l, "rinv", NULL, 0) == 0);
    /* the device fields exist by name and need a device */
    {
        double *d = NULL;
        IS(spdy_letkf_field(l, "obs_lnsigma", &d), SPDY_ERR_NO_DEVICE, "host-only plan");
        IS(spdy_letkf_field(l, "obs_used", &d), SPDY_ERR_NO_DEVICE, "host-only plan");
        CHECK(!d);
    }
    /* the lifetime rule: the object outlives its plan as a dead handle */
    CHECK(spdy_plan_destroy(gone) == SPDY_OK);
    IS(spdy_pobs_set(lg, 3, good), SPDY_ERR_STATE, "has been destroyed");
    IS(spdy_pobs_set(lg, -1, NULL), SPDY_ERR_STATE, "analysis object");
    CHECK(spdy_letkf_destroy(lg) == SPDY_OK && spdy_letkf_destroy(l1) == SPDY_OK && spdy_plan_destroy(flat) == SPDY_OK);
    CHECK(spdy_plan_destroy(p) == SPDY_OK);
    IS(spdy_pobs_set(l, 3, good), SPDY_ERR_STATE, "has been destroyed");
    CHECK(spdy_letkf_destroy(l) == SPDY_OK);
    printf("pobs host check ok: every rejection in its order, the tables and the lifetime rule on a host-only plan\n");
    return 0;
}
