// C ABI of the column physics (include/spdy.h, "column physics"): the precipitation block (physics.f90:110-138) and the
// radiation schemes (physics.f90:146-166 and :180-186).  Kernels: csrc/spdy_physics.hip, csrc/spdy_radiation.hip.
#include <cstring>

#include "spdy_plan.hpp"

using namespace spdy_detail;
using spdy::HostTables;

namespace {
int check_kx(const spdy_plan *p, const char *scheme)
{
    const int kx = p->tab.kx;
    if (kx < 5 || kx > spdy::COLUMN_KMAX) return fail(SPDY_ERR_ARG, "%s: kx=%d outside [5, %d]", scheme, kx, (int)spdy::COLUMN_KMAX);
    return SPDY_OK;
}

// argument checks that need no device (a host-only plan answers them), in the order include/spdy.h gives
int column_args(const spdy_plan *p, const char *scheme, int nb, bool need_date, bool ok_ptrs)
{
    NEED_PLAN(p);
    RC(check_kx(p, scheme));
    RC(check_batch(p, nb));
    if (!p->tab.sigma_ready) return fail(SPDY_ERR_STATE, "%s needs sigma levels (kx in {5,7,8} or spdy_plan_set_sigma)", scheme);
    if (need_date && !p->tab.date_ready) return fail(SPDY_ERR_STATE, "radiation needs a date (spdy_radiation_set_date)");
    if (!ok_ptrs) return fail(SPDY_ERR_ARG, "null device pointer");
    return SPDY_OK;
}

// the kernel-argument fields every scheme has: the batch, the grid and the model state's fields
template <class Cols>
Cols column_fields(const spdy_plan *p, int nb, const double *tg, const double *qg, const double *phig, const double *pslg,
                   double *ttend)
{
    Cols a{};
    a.nb = nb; a.ncol = p->tab.ix * p->tab.il; a.kx = p->tab.kx;
    a.tg = tg; a.qg = qg; a.phig = phig; a.pslg = pslg; a.ttend = ttend;
    return a;
}

// the kernel's view of the plan's physics tables: bottom up, entry r = level kx - r
spdy::MoistCols moist_cols(const spdy_plan *p, int nb, const double *tg, const double *qg, const double *phig, const double *pslg,
                           double *ttend, double *qtend, const spdy_moist_out *out)
{
    const HostTables &t = p->tab;
    const int kx = t.kx;
    auto a = column_fields<spdy::MoistCols>(p, nb, tg, qg, phig, pslg, ttend);
    a.qtend = qtend;
    if (out) {
        a.precnv = out->precnv; a.precls = out->precls; a.cbmf = out->cbmf; a.iptop = out->iptop; a.icnv = out->icnv;
        a.qsat = out->qsat; a.rh = out->rh; a.se = out->se;
    }
    for (int r = 0; r < kx; ++r) {
        const int k = kx - 1 - r;                     // 0-based level index
        a.fsg[r] = t.fsg[k];
        a.wvi2[r] = t.wvi[kx + k];
        a.entr[r] = k >= 1 && k <= kx - 2 ? t.entr[k - 1] : 0.0;
        a.grdsig[r] = t.grdsig[k];
        a.grdscp[r] = t.grdscp[k];
        a.rhref[r] = t.lsc_rhref[k];
        a.dqmax[r] = t.lsc_dqmax[k];
        a.pfact[r] = t.lsc_pfact[k];
    }
    a.fm0 = t.fm0;
    return a;
}

// the kernel's view of the plan's tables: per level, top down (entry k = the reference's level k + 1)
spdy::RadCols rad_cols(const spdy_plan *p, int nb, const double *tg, const double *qg, const double *phig, const double *pslg,
                       double *ttend, double *state, const spdy_rad_out *out)
{
    const HostTables &t = p->tab;
    const int kx = t.kx;
    auto a = column_fields<spdy::RadCols>(p, nb, tg, qg, phig, pslg, ttend);
    a.ix = t.ix; a.il = t.il; a.state = state; a.zonal = p->d_radzonal;
    if (out) {
        a.cloudc = out->cloudc; a.clstr = out->clstr; a.icltop = out->icltop; a.ssrd = out->ssrd; a.ssr = out->ssr;
        a.tsr = out->tsr; a.slrd = out->slrd; a.slr = out->slr; a.olr = out->olr; a.tt_rsw = out->tt_rsw; a.tt_rlw = out->tt_rlw;
    }
    // shortwave_radiation.f90:121 abs1 = absdry + absaer*fsg(k)**2 (float32 parameters widened), :231 eps1
    const double absdry = static_cast<double>(0.033f), absaer = static_cast<double>(0.033f);
    for (int k = 0; k < kx; ++k) {
        a.dhs[k] = t.dhs[k];
        a.abs1[k] = absdry + absaer * (t.fsg[k] * t.fsg[k]);
        a.wvi2[k] = t.wvi[kx + k];
        a.grdscp[k] = t.grdscp[k];
    }
    a.eps1 = static_cast<double>(0.05f) / (t.dhs[0] + t.dhs[1]);
    return a;
}
}  // namespace

extern "C" {

/* ---------------------------------------------------------------- moist physics (physics.f90:110-138) */
int spdy_moist_columns_dev(spdy_plan *p, int nb, const double *tg, const double *qg, const double *phig, const double *pslg,
                           double *ttend, double *qtend, const spdy_moist_out *out)
{
    RC(column_args(p, "moist physics", nb, false, !nb || (tg && qg && phig && pslg && ttend && qtend)));
    NEED_DEVICE(p);
    KERNEL(spdy::launch_moist_columns(moist_cols(p, nb, tg, qg, phig, pslg, ttend, qtend, out), p->stream));
    return SPDY_OK;
}

int spdy_moist_workspace(spdy_plan *p)
{
    NEED_DEVICE(p);
    if (p->moist_grid) return SPDY_OK;
    NOT_CAPTURING(p, "allocating the moist-physics workspace (call spdy_moist_workspace before the capture)");
    void *ptr;
    RC(dev_alloc(p, (size_t)(3 * p->tab.kx + 1) * grid_elems(p) * sizeof(double), &ptr));
    p->moist_grid = static_cast<double *>(ptr);
    return SPDY_OK;
}

int spdy_moist_physics_dev(spdy_plan *p, const double *t, const double *q, const double *phi, const double *ps, double *ttend,
                           double *qtend, const spdy_moist_out *out)
{
    RC(column_args(p, "moist physics", 1, false, t && q && phi && ps && ttend && qtend));
    const int kx = p->tab.kx;
    if (p->max_batch < 3 * kx + 1) return fail(SPDY_ERR_ARG, "max_batch must be >= 3*kx+1 for the moist physics from spectra");
    NEED_DEVICE(p);
    RC(spdy_moist_workspace(p));
    // physics.f90:102-107 for the fields the block reads: ONE inverse launch of t, q, phi (kx levels each) and ps, kcos 1
    const spdy_spec_seg segs[4] = {{kx, t}, {kx, q}, {kx, phi}, {1, ps}};
    RC(inverse_plain_one(p, 4, segs, p->moist_grid));
    const size_t L = (size_t)kx * grid_elems(p);
    const double *g = p->moist_grid;
    KERNEL(spdy::launch_moist_columns(moist_cols(p, 1, g, g + L, g + 2 * L, g + 3 * L, ttend, qtend, out), p->stream));
    return SPDY_OK;
}

/* ---------------------------------------------------------------- radiation (physics.f90:146-166, :180-186) */
int spdy_radiation_set_date(spdy_plan *p, double tyear)
{
    NEED_PLAN(p);
    NOT_CAPTURING(p, "spdy_radiation_set_date (host table build + upload)");
    const std::string err = p->tab.set_date(tyear);
    if (!err.empty()) return fail(SPDY_ERR_ARG, "radiation_set_date: %s", err.c_str());
    if (p->device < 0) return SPDY_OK;
    HIP_TRY(hipSetDevice(p->device));
    const HostTables &t = p->tab;
    const size_t n = (size_t)5 * t.il;
    if (!p->d_radzonal) {
        void *ptr;
        RC(dev_alloc(p, n * sizeof(double), &ptr));
        p->d_radzonal = static_cast<double *>(ptr);
    }
    // stream-ordered: work enqueued (or a graph replayed) before this call still reads the previous date, work after it the
    // new one.  The synchronisation keeps the host staging vector alive until the copy is done.
    std::vector<double> h(n);
    const std::vector<double> *f[5] = {&t.fsol, &t.ozone, &t.ozupp, &t.zenit, &t.stratz};
    for (int i = 0; i < 5; ++i) std::memcpy(h.data() + (size_t)i * t.il, f[i]->data(), sizeof(double) * t.il);
    HIP_TRY(hipMemcpyAsync(p->d_radzonal, h.data(), n * sizeof(double), hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return SPDY_OK;
}

int spdy_radiation_state_size(const spdy_plan *p)
{
    NEED_PLAN(p);
    RC(check_kx(p, "radiation"));
    return spdy::rad_state_fields(p->tab.kx) * p->tab.ix * p->tab.il;
}

int spdy_radiation_down_dev(spdy_plan *p, int nb, int compute_sw, const double *tg, const double *qg, const double *phig,
                            const double *pslg, const double *rh, const double *precnv, const double *precls, const int *iptop,
                            const spdy_rad_surface *sfc, double *state, const spdy_rad_out *out)
{
    const bool sw_ok = !compute_sw || (rh && precnv && precls && iptop && sfc && sfc->fmask && sfc->albsfc);
    RC(column_args(p, "radiation", nb, true, !nb || (tg && qg && phig && pslg && state && sw_ok)));
    NEED_DEVICE(p);
    spdy::RadCols a = rad_cols(p, nb, tg, qg, phig, pslg, nullptr, state, out);
    a.compute_sw = compute_sw ? 1 : 0;
    if (compute_sw) {
        a.rh = rh; a.precnv = precnv; a.precls = precls; a.iptop = iptop; a.fmask = sfc->fmask; a.albsfc = sfc->albsfc;
    }
    if (compute_sw) KERNEL(spdy::launch_radiation(a, 0, p->stream));
    KERNEL(spdy::launch_radiation(a, 1, p->stream));
    return SPDY_OK;
}

int spdy_radiation_up_dev(spdy_plan *p, int nb, const double *tg, const double *pslg, const double *ts, const double *fsfcu,
                          double *state, double *ttend, const spdy_rad_out *out)
{
    RC(column_args(p, "radiation", nb, true, !nb || (tg && pslg && ts && fsfcu && state && ttend)));
    NEED_DEVICE(p);
    spdy::RadCols a = rad_cols(p, nb, tg, nullptr, nullptr, pslg, ttend, state, out);
    a.ts = ts; a.fsfcu = fsfcu;
    KERNEL(spdy::launch_radiation(a, 2, p->stream));
    return SPDY_OK;
}

}  // extern "C"
