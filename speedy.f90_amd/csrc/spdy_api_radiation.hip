// C ABI of the radiation schemes (include/spdy.h, "column physics: radiation"): the zonal forcing of a date, the radiation
// state's size and the two halves, physics.f90:146-166 (down) and :180-186 (up).  Kernels: csrc/spdy_radiation.hip.
#include <cstring>

#include "spdy_plan.hpp"

using namespace spdy_detail;
using spdy::HostTables;

namespace {
// argument checks that need no device (a host-only plan answers them)
int rad_args(const spdy_plan *p, int nb, bool ok_ptrs)
{
    NEED_PLAN(p);
    const int kx = p->tab.kx;
    if (kx < 5 || kx > spdy::RAD_KMAX) return fail(SPDY_ERR_ARG, "radiation: kx=%d outside [5, %d]", kx, (int)spdy::RAD_KMAX);
    RC(check_batch(p, nb));
    if (!p->tab.sigma_ready) return fail(SPDY_ERR_STATE, "radiation needs sigma levels (kx in {5,7,8} or spdy_plan_set_sigma)");
    if (!p->tab.date_ready) return fail(SPDY_ERR_STATE, "radiation needs a date (spdy_radiation_set_date)");
    if (!ok_ptrs) return fail(SPDY_ERR_ARG, "null device pointer");
    return SPDY_OK;
}

// the kernel's view of the plan's tables: per level, top down (entry k = the reference's level k + 1)
spdy::RadCols rad_cols(const spdy_plan *p, int nb, const double *tg, const double *pslg, double *state, const spdy_rad_out *out)
{
    const HostTables &t = p->tab;
    const int kx = t.kx;
    spdy::RadCols a{};
    a.nb = nb; a.ncol = t.ix * t.il; a.ix = t.ix; a.il = t.il; a.kx = kx;
    a.tg = tg; a.pslg = pslg; a.state = state; a.zonal = p->d_radzonal;
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
    const int kx = p->tab.kx;
    if (kx < 5 || kx > spdy::RAD_KMAX) return fail(SPDY_ERR_ARG, "radiation: kx=%d outside [5, %d]", kx, (int)spdy::RAD_KMAX);
    return spdy::rad_state_fields(kx) * p->tab.ix * p->tab.il;
}

int spdy_radiation_down_dev(spdy_plan *p, int nb, int compute_sw, const double *tg, const double *qg, const double *phig,
                            const double *pslg, const double *rh, const double *precnv, const double *precls, const int *iptop,
                            const spdy_rad_surface *sfc, double *state, const spdy_rad_out *out)
{
    const bool sw_ok = !compute_sw || (rh && precnv && precls && iptop && sfc && sfc->fmask && sfc->albsfc);
    RC(rad_args(p, nb, !nb || (tg && qg && phig && pslg && state && sw_ok)));
    NEED_DEVICE(p);
    spdy::RadCols a = rad_cols(p, nb, tg, pslg, state, out);
    a.compute_sw = compute_sw ? 1 : 0;
    a.qg = qg; a.phig = phig;
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
    RC(rad_args(p, nb, !nb || (tg && pslg && ts && fsfcu && state && ttend)));
    NEED_DEVICE(p);
    spdy::RadCols a = rad_cols(p, nb, tg, pslg, state, out);
    a.ts = ts; a.fsfcu = fsfcu; a.ttend = ttend;
    KERNEL(spdy::launch_radiation(a, 2, p->stream));
    return SPDY_OK;
}

}  // extern "C"
