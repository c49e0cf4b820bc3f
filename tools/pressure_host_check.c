/* Host check of the pressure-level output's argument paths (include/spdy.h, "pressure-level output") on a host-only plan: every
 * rejection of spdy_ens_output_pressure_dev, spdy_ens_output_pressure_grid_dev and spdy_output_pressure_dev in the documented
 * order, with its text, and SPDY_ERR_NO_DEVICE last.  Built by `make hostcheck` in speedy.f90_amd with the address and
 * undefined-behaviour sanitizers on the host code of the plan and of the step and output calls; exits 0 when every call returns
 * the documented code and text. */
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
    enum { KX = 8, IX = 96, IY = 24, NMEM = 2 };
    spdy_plan *p = NULL, *nosig = NULL;
    _Alignas(16) double x[4];                       /* a dummy, 16-byte aligned where it stands for the grids: no check reads it */
    double *q = x;
    float *f = (float *)x, *odd = (float *)x + 1;
    double lev[SPDY_MAX_PLEV + 1], bad[3] = {50000.0, 0.0, 85000.0};
    spdy_output_fields all = {f, f, f, f, f, f}, hole = {f, f, f, NULL, f, f}, skew = {f, f, odd, f, f, f};
    const int P = SPDY_PLEV_LINEAR_P, L = SPDY_PLEV_LOG_P;
    for (int l = 0; l <= SPDY_MAX_PLEV; ++l) lev[l] = 1000.0 * (l + 1);
    CHECK(spdy_plan_create(30, IX, IY, KX, NMEM * (3 * KX + 1), SPDY_DEVICE_NONE, &p) == SPDY_OK);
    CHECK(spdy_plan_create(30, IX, IY, 6, NMEM * 19, SPDY_DEVICE_NONE, &nosig) == SPDY_OK);      /* kx = 6: no default sigma levels */
    /* the ensemble output's first checks */
    IS(spdy_ens_output_pressure_dev(NULL, 1, q, q, q, q, q, q, NULL, 1, lev, P, &all, NULL, NULL, NULL), SPDY_ERR_ARG, "null plan");
    IS(spdy_ens_output_pressure_grid_dev(NULL, 1, q, NULL, 1, lev, P, &all, NULL, NULL, NULL), SPDY_ERR_ARG, "null plan");
    IS(spdy_output_pressure_dev(NULL, q, q, q, q, q, q, 1, lev, P, f, f, f, f, f, f), SPDY_ERR_ARG, "null plan");
    IS(spdy_ens_output_pressure_dev(p, 0, q, q, q, q, q, q, NULL, 0, NULL, 7, NULL, NULL, NULL, NULL), SPDY_ERR_ARG, "nmem=0 < 1");
    IS(spdy_ens_output_pressure_grid_dev(p, -2, NULL, NULL, 0, NULL, 7, NULL, NULL, NULL, NULL), SPDY_ERR_ARG, "nmem=-2 < 1");
    IS(spdy_ens_output_pressure_dev(p, NMEM + 1, q, q, q, q, q, q, NULL, 0, NULL, 7, NULL, NULL, NULL, NULL), SPDY_ERR_ARG, "max_batch");
    /* then the levels and the coordinate */
    IS(spdy_ens_output_pressure_dev(p, NMEM, NULL, q, q, q, q, q, NULL, 0, NULL, 7, NULL, NULL, NULL, NULL), SPDY_ERR_ARG, "nlev=0 outside [1, 32]");
    IS(spdy_ens_output_pressure_dev(p, NMEM, NULL, q, q, q, q, q, NULL, SPDY_MAX_PLEV + 1, lev, P, &all, NULL, NULL, NULL), SPDY_ERR_ARG,
       "nlev=33 outside [1, 32]");
    IS(spdy_ens_output_pressure_grid_dev(p, NMEM + 5, NULL, NULL, -1, lev, P, NULL, NULL, NULL, NULL), SPDY_ERR_ARG, "nlev=-1 outside");
    IS(spdy_ens_output_pressure_dev(p, NMEM, NULL, q, q, q, q, q, NULL, 3, NULL, 7, NULL, NULL, NULL, NULL), SPDY_ERR_ARG, "null plev");
    IS(spdy_ens_output_pressure_dev(p, NMEM, NULL, q, q, q, q, q, NULL, 3, bad, 7, NULL, NULL, NULL, NULL), SPDY_ERR_ARG,
       "plev[1]=0 must be finite and > 0");
    bad[1] = -85000.0;
    IS(spdy_ens_output_pressure_grid_dev(p, NMEM, NULL, NULL, 3, bad, 7, NULL, NULL, NULL, NULL), SPDY_ERR_ARG, "plev[1]=-85000 must be");
    bad[1] = 70000.0; bad[2] = NAN;
    IS(spdy_output_pressure_dev(p, NULL, q, q, q, q, q, 3, bad, 7, f, f, f, f, f, f), SPDY_ERR_ARG, "plev[2]=nan must be");
    bad[2] = INFINITY;
    IS(spdy_ens_output_pressure_dev(p, NMEM, NULL, q, q, q, q, q, NULL, 3, bad, 7, NULL, NULL, NULL, NULL), SPDY_ERR_ARG, "plev[2]=inf must be");
    IS(spdy_ens_output_pressure_dev(p, NMEM, NULL, q, q, q, q, q, NULL, 2, bad, 7, NULL, NULL, NULL, NULL), SPDY_ERR_ARG, "unknown coord=7");
    IS(spdy_ens_output_pressure_grid_dev(p, NMEM, NULL, NULL, SPDY_MAX_PLEV, lev, -1, NULL, NULL, NULL, NULL), SPDY_ERR_ARG, "unknown coord=-1");
    /* then the sigma levels */
    IS(spdy_ens_output_pressure_dev(nosig, NMEM, NULL, q, q, q, q, q, NULL, 2, lev, L, NULL, NULL, NULL, NULL), SPDY_ERR_STATE, "needs sigma levels");
    IS(spdy_ens_output_pressure_grid_dev(nosig, NMEM, NULL, NULL, 2, lev, P, NULL, NULL, NULL, NULL), SPDY_ERR_STATE, "needs sigma levels");
    IS(spdy_output_pressure_dev(nosig, NULL, q, q, q, q, q, 2, lev, P, f, f, f, f, f, f), SPDY_ERR_STATE, "needs sigma levels");
    /* then the pointers, the groups and their alignment */
    IS(spdy_ens_output_pressure_dev(p, NMEM, q, q, q, NULL, q, q, NULL, 2, lev, L, NULL, NULL, NULL, NULL), SPDY_ERR_ARG, "null device pointer");
    IS(spdy_ens_output_pressure_grid_dev(p, NMEM, NULL, NULL, 2, lev, P, NULL, NULL, NULL, NULL), SPDY_ERR_ARG, "null device pointer");
    IS(spdy_ens_output_pressure_grid_dev(p, NMEM, q + 1, NULL, 2, lev, P, NULL, NULL, NULL, NULL), SPDY_ERR_ARG, "16-byte aligned");
    IS(spdy_ens_output_pressure_dev(p, NMEM, q, q, q, q, q, q, NULL, 2, lev, L, NULL, NULL, NULL, f), SPDY_ERR_ARG, "no output group");
    IS(spdy_ens_output_pressure_grid_dev(p, NMEM, q, NULL, 2, lev, P, NULL, NULL, NULL, f), SPDY_ERR_ARG, "no output group");
    IS(spdy_ens_output_pressure_dev(p, NMEM, q, q, q, q, q, q, NULL, 2, lev, L, &all, &hole, NULL, NULL), SPDY_ERR_ARG, "null device pointer");
    IS(spdy_output_pressure_dev(p, q, q, q, q, q, q, 2, lev, P, f, f, f, f, NULL, f), SPDY_ERR_ARG, "null device pointer");
    IS(spdy_ens_output_pressure_dev(p, NMEM, q, q, q, q, q, q, NULL, 2, lev, L, &all, NULL, &skew, NULL), SPDY_ERR_ARG, "8-byte aligned");
    IS(spdy_ens_output_pressure_grid_dev(p, NMEM, q, NULL, 2, lev, P, NULL, &all, NULL, odd), SPDY_ERR_ARG, "8-byte aligned");
    IS(spdy_output_pressure_dev(p, q, q, q, q, q, q, 2, lev, P, f, odd, f, f, f, f), SPDY_ERR_ARG, "8-byte aligned");
    /* and the device last */
    IS(spdy_ens_output_pressure_dev(p, NMEM, q, q, q, q, q, q, NULL, SPDY_MAX_PLEV, lev, P, &all, &all, &all, f), SPDY_ERR_NO_DEVICE, "host-only plan");
    IS(spdy_ens_output_pressure_dev(p, 1, q, q, q, q, q, q, (const int *)x, 1, lev, L, NULL, &all, NULL, NULL), SPDY_ERR_NO_DEVICE, "host-only plan");
    IS(spdy_ens_output_pressure_grid_dev(p, NMEM + 7, q, NULL, 3, lev, L, &all, NULL, &all, f), SPDY_ERR_NO_DEVICE, "host-only plan");
    IS(spdy_output_pressure_dev(p, q, q, q, q, q, q, 8, lev, P, f, f, f, f, f, f), SPDY_ERR_NO_DEVICE, "host-only plan");
    /* the ensemble output itself, whose front the new calls share: unchanged */
    IS(spdy_ens_output_batch_dev(p, NMEM, q, q, q, q, q, q, NULL, NULL, NULL, NULL), SPDY_ERR_ARG, "no output group");
    IS(spdy_ens_output_batch_dev(p, NMEM, q, q, q, q, q, q, NULL, &all, &all, &all), SPDY_ERR_NO_DEVICE, "host-only plan");
    CHECK(spdy_plan_destroy(nosig) == SPDY_OK && spdy_plan_destroy(p) == SPDY_OK);
    printf("pressure host check ok: every rejection in its order on a host-only plan\n");
    return 0;
}
