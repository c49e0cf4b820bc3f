/* Host check of the observation ingestion (include/spdy.h, "ensemble analysis"): spdy_letkf_set_obs and spdy_letkf_table on a
 * host-only plan, fed the operator's edge cases, nobs = 0 and nobs = max_obs; and of the tables of weight interpolation
 * (spdy_letkf_set_weight_stride) at the smallest and largest strides and with a short last latitude interval; and of
 * spdy_relax_set's rejections and its setting on a host-only plan; and of spdy_qc_set and spdy_qc_set_slot, their rejections in
 * the documented order, a grouping of the whole network and of an empty one, and the stats-only call's refusals.  Built by `make hostcheck` in speedy.f90_amd with
 * the address and undefined-behaviour sanitizers on the host code of the plan, the tables and the analysis; exits 0 when every
 * stencil is a convex combination of four grid points and every rejection is the documented code. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "spdy.h"

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "line %d: %s -- %s\n", __LINE__, #cond, spdy_last_error()); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static int tables_ok(spdy_letkf *l, int nobs, int ncol)
{
    static const char *const names[5] = {"stencil_index", "stencil_weight", "unit", "lnsigma", "rinv"};
    static const int per[5] = {4, 4, 3, 1, 1};
    for (int t = 0; t < 5; ++t) {
        const int n = spdy_letkf_table(l, names[t], NULL, 0);
        if (n != per[t] * nobs) return 0;
        double *buf = malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
        if (spdy_letkf_table(l, names[t], buf, n) != n) { free(buf); return 0; }
        if (n > 0 && spdy_letkf_table(l, names[t], buf, n - 1) != SPDY_ERR_ARG) { free(buf); return 0; }
        for (int o = 0; o < nobs; ++o) {
            double sum = 0.0;
            for (int c = 0; c < per[t]; ++c) {
                const double v = buf[per[t] * o + c];
                if (!isfinite(v)) { free(buf); return 0; }
                if (t == 0 && (v < 0 || v >= ncol || v != floor(v))) { free(buf); return 0; }
                if (t == 1 && (v < 0.0 || v > 1.0)) { free(buf); return 0; }
                sum += t == 2 ? v * v : v;
            }
            if ((t == 1 || t == 2) && fabs(sum - 1.0) > 1e-14) { free(buf); return 0; }
        }
        free(buf);
    }
    return 1;
}

/* the coarse list ascending and inside the grid; every stencil entry inside the list, every weight in [0, 1], their sum 1 */
static int interp_ok(spdy_letkf *l, int si, int sj, int ix, int il)
{
    const int ncol = ix * il, nc = spdy_letkf_table(l, "coarse_columns", NULL, 0);
    if (si == 1 && sj == 1)
        return nc == 0 && spdy_letkf_table(l, "interp_index", NULL, 0) == 0 && spdy_letkf_table(l, "interp_weight", NULL, 0) == 0;
    if (nc != (ix / si) * ((il - 2) / sj + 2)) return 0;
    double *c = malloc(sizeof(double) * (size_t)nc), *idx = malloc(sizeof(double) * 4 * (size_t)ncol),
           *w = malloc(sizeof(double) * 4 * (size_t)ncol);
    int ok = spdy_letkf_table(l, "coarse_columns", c, nc) == nc && spdy_letkf_table(l, "interp_index", idx, 4 * ncol) == 4 * ncol &&
             spdy_letkf_table(l, "interp_weight", w, 4 * ncol) == 4 * ncol && spdy_letkf_table(l, "interp_weight", w, 4 * ncol - 1) == SPDY_ERR_ARG;
    for (int n = 0; ok && n < nc; ++n) ok = c[n] >= 0 && c[n] < ncol && (n == 0 || c[n] > c[n - 1]);
    for (int n = 0; ok && n < ncol; ++n) {
        double sum = 0.0;
        for (int t = 0; t < 4; ++t) {
            ok = ok && idx[4 * n + t] >= 0 && idx[4 * n + t] < nc && w[4 * n + t] >= 0.0 && w[4 * n + t] <= 1.0;
            sum += w[4 * n + t];
        }
        ok = ok && fabs(sum - 1.0) <= 1e-15;
    }
    free(c); free(idx); free(w);
    return ok;
}

int main(void)
{
    enum { KX = 5, IX = 96, IY = 24, MAXOBS = 64 };
    spdy_plan *p = NULL;
    spdy_letkf *l = NULL;
    CHECK(spdy_plan_create(30, IX, IY, KX, 3 * (2 * KX + 1), SPDY_DEVICE_NONE, &p) == SPDY_OK);
    CHECK(spdy_letkf_create(p, 3, MAXOBS, &l) == SPDY_OK);
    CHECK(spdy_letkf_set_localization(l, 5.0e5, 0.1, 1.1) == SPDY_OK);
    /* on a grid point's longitude, between columns ix-1 and 0, poleward of the outermost rows, the poles, lon = 360, negative
     * and large longitudes, the equator */
    static const double pts[][2] = {{18.75, 12.0}, {359.0, 12.3}, {358.1, -33.0}, {10.0, 89.9}, {200.0, -89.5}, {77.0, 90.0},
                                    {300.0, -90.0}, {360.0, 45.0}, {-12.5, -5.0}, {-360.0, 0.0}, {725.0, 60.0}, {-1e-20, 1.0},
                                    {1e6, -1.0}, {0.0, 0.0}};
    const int npts = (int)(sizeof(pts) / sizeof(pts[0]));
    spdy_obs obs[MAXOBS];
    for (int o = 0; o < MAXOBS; ++o) {
        obs[o].var = o % 5; obs[o].lev = obs[o].var == SPDY_OBS_PS ? 99 : (3 * o) % KX;      /* lev is ignored for PS */
        obs[o].lon = pts[o % npts][0] + 0.37 * (o / npts); obs[o].lat = pts[o % npts][1];
        obs[o].value = 1.0 + o; obs[o].error = 0.5 + o;
    }
    CHECK(spdy_letkf_set_obs(l, 0, NULL) == SPDY_OK && tables_ok(l, 0, IX * 2 * IY));
    CHECK(spdy_letkf_set_obs(l, npts, obs) == SPDY_OK && tables_ok(l, npts, IX * 2 * IY));
    CHECK(spdy_letkf_set_obs(l, MAXOBS, obs) == SPDY_OK && tables_ok(l, MAXOBS, IX * 2 * IY));
    /* rejections leave the tables alone */
    CHECK(spdy_letkf_set_obs(l, MAXOBS + 1, obs) == SPDY_ERR_ARG);
    CHECK(spdy_letkf_set_obs(l, -1, obs) == SPDY_ERR_ARG && spdy_letkf_set_obs(l, 1, NULL) == SPDY_ERR_ARG);
    spdy_obs bad = obs[0];
    bad.var = 5; CHECK(spdy_letkf_set_obs(l, 1, &bad) == SPDY_ERR_ARG); bad = obs[0];
    bad.lev = KX; CHECK(spdy_letkf_set_obs(l, 1, &bad) == SPDY_ERR_ARG); bad = obs[0];
    bad.lat = 90.0001; CHECK(spdy_letkf_set_obs(l, 1, &bad) == SPDY_ERR_ARG); bad = obs[0];
    bad.lon = INFINITY; CHECK(spdy_letkf_set_obs(l, 1, &bad) == SPDY_ERR_ARG); bad = obs[0];
    bad.value = NAN; CHECK(spdy_letkf_set_obs(l, 1, &bad) == SPDY_ERR_ARG); bad = obs[0];
    bad.error = 0.0; CHECK(spdy_letkf_set_obs(l, 1, &bad) == SPDY_ERR_ARG); bad = obs[0];
    bad.error = NAN; CHECK(spdy_letkf_set_obs(l, 1, &bad) == SPDY_ERR_ARG);
    CHECK(tables_ok(l, MAXOBS, IX * 2 * IY));
    CHECK(spdy_letkf_table(l, "nothing", NULL, 0) == SPDY_ERR_ARG);
    double *d = NULL;
    CHECK(spdy_letkf_field(l, "hx", &d) == SPDY_ERR_NO_DEVICE);
    CHECK(spdy_ens_letkf_dev(l, (double *)obs, (double *)obs, (double *)obs, (double *)obs, (double *)obs) == SPDY_ERR_NO_DEVICE);
    /* weight interpolation: the tables of every kind of stride, the rejections, back to (1, 1) */
    static const int strides[][2] = {{1, 1}, {2, 2}, {3, 5}, {4, 47}, {1, 3}, {48, 1}, {48, 47}, {1, 1}};
    CHECK(interp_ok(l, 1, 1, IX, 2 * IY) && spdy_letkf_field(l, "weights", &d) == SPDY_ERR_STATE);
    for (int n = 0; n < (int)(sizeof(strides) / sizeof(strides[0])); ++n) {
        CHECK(spdy_letkf_set_weight_stride(l, strides[n][0], strides[n][1]) == SPDY_OK);
        CHECK(interp_ok(l, strides[n][0], strides[n][1], IX, 2 * IY));
    }
    CHECK(spdy_letkf_set_weight_stride(l, 3, 5) == SPDY_OK && spdy_letkf_field(l, "weights", &d) == SPDY_ERR_NO_DEVICE);
    CHECK(spdy_letkf_set_weight_stride(NULL, 2, 2) == SPDY_ERR_ARG && spdy_letkf_set_weight_stride(l, 5, 1) == SPDY_ERR_ARG);
    CHECK(spdy_letkf_set_weight_stride(l, 96, 1) == SPDY_ERR_ARG && spdy_letkf_set_weight_stride(l, 0, 1) == SPDY_ERR_ARG);
    CHECK(spdy_letkf_set_weight_stride(l, 2, 0) == SPDY_ERR_ARG && spdy_letkf_set_weight_stride(l, 2, 2 * IY) == SPDY_ERR_ARG);
    CHECK(interp_ok(l, 3, 5, IX, 2 * IY));
    /* relaxation: a host-only plan stores a setting and allocates nothing; each argument alone is refused outside [0, 1] */
    static const double outside[4] = {NAN, -0.1, 1.5, INFINITY};
    CHECK(spdy_relax_set(NULL, 0.5, 0.5) == SPDY_ERR_ARG);
    CHECK(spdy_relax_set(l, 0.3, 0.9) == SPDY_OK && spdy_relax_set(l, 1.0, 1.0) == SPDY_OK);
    for (int n = 0; n < 4; ++n) {
        CHECK(spdy_relax_set(l, outside[n], 0.5) == SPDY_ERR_ARG);
        CHECK(spdy_relax_set(l, 0.5, outside[n]) == SPDY_ERR_ARG);
    }
    CHECK(spdy_relax_set(l, 0.0, 0.0) == SPDY_OK);
    CHECK(spdy_letkf_field(l, "inflation", &d) == SPDY_ERR_NO_DEVICE);
    /* background check: a host-only plan stores a setting and allocates nothing; gross, then ngroups, then the entries; the table
     * is copied, so the caller's may go at once; set_obs returns the grouping to the default */
    int *group = malloc(sizeof(int) * MAXOBS);
    for (int o = 0; o < MAXOBS; ++o) group[o] = o % SPDY_QC_MAX_GROUPS;
    CHECK(spdy_qc_set(NULL, 5.0, 0, NULL) == SPDY_ERR_ARG);
    CHECK(spdy_qc_stats_dev(l, d, d, d, d, d, NULL, 0) == SPDY_ERR_STATE);                  /* off: spdy_qc_set first */
    for (int n = 0; n < 4; ++n)
        if (n != 2) CHECK(spdy_qc_set(l, outside[n], SPDY_QC_MAX_GROUPS, group) == SPDY_ERR_ARG);
    CHECK(spdy_qc_set(l, 5.0, 0, group) == SPDY_ERR_ARG && spdy_qc_set(l, 5.0, SPDY_QC_MAX_GROUPS + 1, group) == SPDY_ERR_ARG);
    CHECK(spdy_qc_set(l, 5.0, SPDY_QC_MAX_GROUPS - 1, group) == SPDY_ERR_ARG);             /* entry 63 is out of [0, 63) */
    group[MAXOBS - 1] = -1;
    CHECK(spdy_qc_set(l, 5.0, SPDY_QC_MAX_GROUPS, group) == SPDY_ERR_ARG);
    group[MAXOBS - 1] = 0;
    CHECK(spdy_qc_stats_dev(l, d, d, d, d, d, NULL, 0) == SPDY_ERR_STATE);                  /* still off: nothing was accepted */
    CHECK(spdy_qc_set(l, 0.0, SPDY_QC_MAX_GROUPS, group) == SPDY_OK);                      /* statistics without rejection */
    free(group);
    CHECK(spdy_qc_set(l, 5.0, 0, NULL) == SPDY_OK && spdy_qc_set(l, 1.5, 1, NULL) == SPDY_OK);
    CHECK(spdy_qc_set_slot(NULL, 0) == SPDY_ERR_ARG && spdy_qc_set_slot(l, -1) == SPDY_ERR_ARG);
    CHECK(spdy_qc_set_slot(l, SPDY_QC_SLOTS) == SPDY_ERR_ARG && spdy_qc_set_slot(l, SPDY_QC_SLOTS - 1) == SPDY_OK);
    CHECK(spdy_qc_stats_grid_dev(l, NULL, NULL, NULL, NULL, NULL, NULL, 9) == SPDY_ERR_STATE);      /* on, but nothing analysed */
    CHECK(spdy_letkf_field(l, "obs_check", &d) == SPDY_ERR_NO_DEVICE && spdy_letkf_field(l, "obs_stats", &d) == SPDY_ERR_NO_DEVICE);
    CHECK(spdy_letkf_set_obs(l, 0, NULL) == SPDY_OK);
    int none = 7;                                      /* a grouping of an empty network: no entry is read */
    CHECK(spdy_qc_set(l, 0.0, 1, &none) == SPDY_OK && spdy_qc_stats_dev(l, d, d, d, d, d, NULL, 0) == SPDY_ERR_STATE);
    CHECK(spdy_letkf_set_obs(l, npts, obs) == SPDY_OK && spdy_qc_set(l, 0.0, 0, NULL) == SPDY_OK);
    CHECK(spdy_letkf_destroy(l) == SPDY_OK && spdy_plan_destroy(p) == SPDY_OK);
    printf("letkf host check ok: %d edge observations, 0 and %d observations\n", npts, (int)MAXOBS);
    return 0;
}
