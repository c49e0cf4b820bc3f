// C ABI of the column physics (include/spdy.h, "column physics"): the precipitation block (physics.f90:110-138), the
// radiation schemes (physics.f90:146-166 and :180-186), the surface fluxes (:169-170), the boundary layer (:193-205) and the
// whole chain, on gridded states and from spectra, without and with SPPT (:207-222).  Kernels: csrc/spdy_sppt.hip, csrc/spdy_physics.hip, csrc/spdy_radiation.hip, csrc/spdy_surface.hip,
// csrc/spdy_column_chain.hip.  The physics from spectra is one body (physics_from_spectra) for one state and nmem members, each without
// and with SPPT; the single state is nmem = 1 on a workspace of its own.
#include <cmath>
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
int column_args(const spdy_plan *p, const char *scheme, int nb, bool need_date, bool ok_ptrs, bool need_orog = false)
{
    NEED_PLAN(p);
    RC(check_kx(p, scheme));
    RC(check_batch(p, nb));
    if (!p->tab.sigma_ready) return fail(SPDY_ERR_STATE, "%s needs sigma levels (kx in {5,7,8} or spdy_plan_set_sigma)", scheme);
    if (need_date && !p->tab.date_ready) return fail(SPDY_ERR_STATE, "radiation needs a date (spdy_radiation_set_date)");
    if (need_orog && !p->tab.orog_ready) return fail(SPDY_ERR_STATE, "%s needs the orography (spdy_surface_set_orography)", scheme);
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

spdy::SfcCols sfc_cols(const spdy_plan *p, int nb, const double *ug, const double *vg, const double *tg, const double *qg,
                       const double *phig, const double *pslg, const double *ssrd, const double *slrd, const spdy_sfc_boundary *b,
                       double *ts, double *fsfcu, double *flux3, const spdy_sfc_out *out)
{
    const HostTables &t = p->tab;
    const int kx = t.kx;
    spdy::SfcCols a{};
    a.nb = nb; a.ncol = t.ix * t.il; a.ix = t.ix; a.kx = kx;
    a.ug = ug; a.vg = vg; a.tg = tg; a.qg = qg; a.phig = phig; a.pslg = pslg; a.ssrd = ssrd; a.slrd = slrd;
    if (b) {
        a.fmask = b->fmask; a.sst = b->sst; a.stl = b->stl; a.soilw = b->soilw; a.snowc = b->snowc; a.alb_l = b->alb_l;
        a.alb_s = b->alb_s;
    }
    a.phis0 = p->d_orog; a.forog = p->d_orog + a.ncol; a.sqcoa = p->d_orog + 2 * (size_t)a.ncol;
    a.ts = ts; a.fsfcu = fsfcu; a.flux3 = flux3;
    if (out) {
        a.ustr = out->ustr; a.vstr = out->vstr; a.shf = out->shf; a.evap = out->evap; a.slru = out->slru; a.hfluxn = out->hfluxn;
        a.tskin = out->tskin; a.u0 = out->u0; a.v0 = out->v0; a.t0 = out->t0;
    }
    a.wvi2_kx = t.wvi[2 * kx - 1]; a.sigl_kx = t.sigl[kx - 1]; a.rgas = t.rgas;
    return a;
}

spdy::PblCols pbl_cols(const spdy_plan *p, int nb, const double *qg, const double *phig, const double *pslg, const double *se,
                       const double *rh, const double *qsat, const int *icnv, const double *flux3, double *utend, double *vtend,
                       double *ttend, double *qtend, const spdy_pbl_out *out)
{
    const HostTables &t = p->tab;
    const int kx = t.kx;
    spdy::PblCols a{};
    a.nb = nb; a.ncol = t.ix * t.il; a.kx = kx;
    a.qg = qg; a.phig = phig; a.pslg = pslg; a.se = se; a.rh = rh; a.qsat = qsat; a.icnv = icnv; a.flux3 = flux3;
    a.utend = utend; a.vtend = vtend; a.ttend = ttend; a.qtend = qtend;
    if (out) { a.ut_pbl = out->ut_pbl; a.vt_pbl = out->vt_pbl; a.tt_pbl = out->tt_pbl; a.qt_pbl = out->qt_pbl; }
    for (int k = 0; k < kx; ++k) {
        a.rsig[k] = t.vd_rsig[k]; a.rsig1[k] = t.vd_rsig1[k]; a.drh0[k] = t.vd_drh0[k]; a.fvdiq2[k] = t.vd_fvdiq2[k];
        if (t.sigh[k + 1] > 0.5) a.diffmask |= 1 << k;               // vertical_diffusion.f90:113, level k + 1
    }
    a.fshcq = t.vd_scalars[2]; a.fshcse = t.vd_scalars[3]; a.fvdise = t.vd_scalars[5];
    a.grdsig_kx = t.grdsig[kx - 1]; a.grdscp_kx = t.grdscp[kx - 1];
    return a;
}

bool boundary_ok(const spdy_sfc_boundary *b)
{
    return b && b->fmask && b->sst && b->stl && b->soilw && b->snowc && b->alb_l && b->alb_s;
}

// SPPT around the chain (physics.f90:85-88, :207-222): the clipped pattern of the nb states, the taper (host, kx values top
// down, null = 1) and the place of the dynamics tendencies, (2 kx + 2) fields each g doubles long like the chain's workspace
struct SpptUse { const double *pattern, *mu; double *save; };

// physics.f90:110-205 on nb gridded states, arguments checked: the five calls, or (fused) the one-launch kernel.  w is the chain's
// workspace of (3 kx + 12) fields, each g doubles long (g >= nb grids).  With sppt the five calls lie between a save and an apply
// kernel, and the one launch is the kernel's SPPT instantiation.
int column_chain(spdy_plan *p, bool fused, int nb, int compute_sw, const double *ug, const double *vg, const double *tg,
                 const double *qg, const double *phig, const double *pslg, const spdy_sfc_boundary *bnd, const double *albsfc,
                 double *rad_state, double *utend, double *vtend, double *ttend, double *qtend, const spdy_column_physics_out *out,
                 double *w, size_t g, const SpptUse *sppt = nullptr)
{
    const size_t L = (size_t)p->tab.kx * g;
    double mu[spdy::COLUMN_KMAX];
    for (int k = 0; k < spdy::COLUMN_KMAX; ++k) mu[k] = sppt && sppt->mu && k < p->tab.kx ? sppt->mu[k] : 1.0;
    double *w2 = w + 3 * L;
    // the caller's optional outputs take the place of the workspace where both exist.  ssrd is written by shortwave calls only
    // and read by every call (the reference holds it in get_physical_tendencies): it stays where the last shortwave call put it
    spdy_moist_out mo{};
    spdy_rad_out ro{};
    spdy_sfc_out so{};
    double *ts = nullptr, *fsfcu = nullptr;
    if (out) { mo = out->moist; ro = out->rad; so = out->sfc; ts = out->ts; fsfcu = out->fsfcu; }
    auto pick = [](auto *&dst, auto *ws) { if (!dst) dst = ws; };
    pick(mo.se, w); pick(mo.rh, w + L); pick(mo.qsat, w + 2 * L);
    pick(ro.ssrd, w2 + 2 * g);
    const spdy_pbl_out *po = out ? &out->pbl : nullptr;
    if (fused) {
        // one launch: what only the next block reads stays in registers and is stored only where the caller asked for it
        if (!nb) return SPDY_OK;
        spdy::ChainCols c{};
        c.nb = nb; c.ncol = p->tab.ix * p->tab.il; c.kx = p->tab.kx;
        c.moist = moist_cols(p, nb, tg, qg, phig, pslg, ttend, qtend, &mo);
        c.rad = rad_cols(p, nb, tg, qg, phig, pslg, ttend, rad_state, &ro);
        c.rad.compute_sw = compute_sw ? 1 : 0;
        c.rad.rh = mo.rh; c.rad.fmask = bnd->fmask; c.rad.albsfc = albsfc;
        c.sfc = sfc_cols(p, nb, ug, vg, tg, qg, phig, pslg, nullptr, nullptr, bnd, ts, fsfcu, nullptr, &so);
        c.pbl = pbl_cols(p, nb, qg, phig, pslg, mo.se, mo.rh, mo.qsat, nullptr, nullptr, utend, vtend, ttend, qtend, po);
        if (!sppt) {
            KERNEL(spdy::launch_column_chain(c, p->stream));
            return SPDY_OK;
        }
        spdy::ChainSpptCols cs{};
        cs.c = c; cs.pattern = sppt->pattern; cs.save_t = sppt->save; cs.save_q = sppt->save + L;
        std::memcpy(cs.mu, mu, sizeof(mu));
        KERNEL(spdy::launch_column_chain_sppt(cs, p->stream));
        return SPDY_OK;
    }
    spdy::SpptCols sc{};
    if (sppt) {
        sc.nb = nb; sc.ncol = p->tab.ix * p->tab.il; sc.kx = p->tab.kx; sc.pattern = sppt->pattern;
        sc.utend = utend; sc.vtend = vtend; sc.ttend = ttend; sc.qtend = qtend; sc.save = sppt->save; sc.g = g;
        std::memcpy(sc.mu, mu, sizeof(mu));
        KERNEL(spdy::launch_sppt_save(sc, p->stream));
    }
    pick(mo.precnv, w2); pick(mo.precls, w2 + g); pick(ro.slrd, w2 + 3 * g);
    pick(ts, w2 + 4 * g); pick(fsfcu, w2 + 5 * g);
    double *flux3 = w2 + 6 * g;
    pick(mo.iptop, reinterpret_cast<int *>(w2 + 10 * g)); pick(mo.icnv, reinterpret_cast<int *>(w2 + 11 * g));
    spdy_rad_surface rs{bnd ? bnd->fmask : nullptr, albsfc};
    RC(spdy_moist_columns_dev(p, nb, tg, qg, phig, pslg, ttend, qtend, &mo));
    RC(spdy_radiation_down_dev(p, nb, compute_sw, tg, qg, phig, pslg, mo.rh, mo.precnv, mo.precls, mo.iptop, &rs, rad_state, &ro));
    RC(spdy_surface_fluxes_dev(p, nb, ug, vg, tg, qg, phig, pslg, ro.ssrd, ro.slrd, bnd, ts, fsfcu, flux3, &so));
    RC(spdy_radiation_up_dev(p, nb, tg, pslg, ts, fsfcu, rad_state, ttend, &ro));
    RC(spdy_pbl_dev(p, nb, qg, phig, pslg, mo.se, mo.rh, mo.qsat, mo.icnv, flux3, utend, vtend, ttend, qtend, po));
    if (sppt) KERNEL(spdy::launch_sppt_apply(sc, p->stream));
    return SPDY_OK;
}

int sppt_workspace(spdy_plan *p, Workspace *w, size_t states, const char *scheme, const char *what)
{
    NEED_PLAN(p);
    RC(check_kx(p, scheme));
    return ensure_workspace(p, w, (size_t)(2 * p->tab.kx + 2) * grid_elems(p) * states, what);
}

// ---- the physics of nmem states from their spectra: one body for spdy_physics_dev, spdy_ens_physics_dev and their SPPT forms ----
struct FromSpectra {   // the arguments the four calls share, in their order
    int compute_sw;
    const double *vor, *div, *t, *q, *phi, *ps;
    const spdy_sfc_boundary *bnd;
    const double *albsfc;
    double *rad_state, *utend, *vtend, *ttend, *qtend;
    const spdy_column_physics_out *out;
};

// The member count against the plan and max_batch against the ONE inverse launch of 3 kx + 1 plain fields per member: the first checks
// of the ensemble calls, the last of the single-state ones.
int physics_members(const spdy_plan *p, int nmem, bool ens)
{
    NEED_PLAN(p);
    if (nmem < 1) return fail(SPDY_ERR_ARG, "ens_physics: nmem=%d < 1", nmem);
    RC(check_kx(p, ens ? "ens_physics" : "physics"));
    const long need = (long)nmem * (3 * p->tab.kx + 1);
    if (p->max_batch >= need) return SPDY_OK;
    if (ens) return fail(SPDY_ERR_ARG, "ens_physics: max_batch=%d must be >= nmem*(3*kx+1)=%ld", p->max_batch, need);
    return fail(SPDY_ERR_ARG, "max_batch must be >= 3*kx+1 for the physics from spectra");
}

// The checks that need no device, in each call's documented order.  With SPPT the pattern is one of the required pointers, and its
// plan and its member count are tested after them.
int physics_args(const spdy_plan *p, int nmem, bool ens, const FromSpectra &a, bool with_sppt = false, const spdy_sppt *sppt = nullptr)
{
    const bool ok = (!with_sppt || sppt) && a.vor && a.div && a.t && a.q && a.phi && a.ps && boundary_ok(a.bnd) &&
                    (!a.compute_sw || a.albsfc) && a.rad_state && a.utend && a.vtend && a.ttend && a.qtend;
    if (ens) RC(physics_members(p, nmem, true));
    RC(column_args(p, ens ? "ens_physics" : "physics", nmem, true, ok, true));
    if (sppt) NEED_LIVE(sppt, "SPPT pattern");
    if (sppt && sppt->plan != p) return fail(SPDY_ERR_ARG, "the SPPT pattern belongs to another plan");
    if (sppt && sppt->nmem != nmem) return fail(SPDY_ERR_ARG, "the SPPT object holds %d patterns, the call has %d states", sppt->nmem, nmem);
    return ens ? SPDY_OK : physics_members(p, 1, false);
}

// the workspace w for at least nmem states; the plan and kx are checked.  With the Fourier workspace: the operator route of the
// T63 inverse launch keeps (vor, div) -> (U, V) in the plan's temporaries
int physics_grids(spdy_plan *p, Workspace *w, int nmem, const char *what)
{
    return ensure_workspace(p, w, (size_t)(8 * p->tab.kx + 13) * grid_elems(p) * nmem, what, true);
}

// physics.f90:94-205 for nmem states, arguments checked and w allocated: ONE inverse launch of time level 1 -- nmem kx (vor, div)
// pairs through uvspec with kcos 2; t, q, phi (nmem kx each) and ps (nmem) with kcos 1 (physics.f90:94-104) -- into w's grids, nmem
// states back to back at state stride kx, then the chain with nb = nmem on w's chain workspace.
int physics_from_spectra(spdy_plan *p, int nmem, const Workspace &w, const SpptUse *sppt, const FromSpectra &a)
{
    const int kx = p->tab.kx, nk = nmem * kx;
    const size_t g1 = grid_elems(p) * nmem, L = (size_t)kx * g1;
    double *ug = w.g, *vg = ug + L, *tg = ug + 2 * L, *qg = ug + 3 * L, *phig = ug + 4 * L, *pslg = ug + 5 * L;
    const spdy_spec_seg segs[SPDY_MAX_SPEC_SEGS] = {{nk, a.t}, {nk, a.q}, {nk, a.phi}, {nmem, a.ps}};
    RC(spdy_inverse_batch_segs_dev(p, nk, a.vor, a.div, ug, vg, 2, SPDY_MAX_SPEC_SEGS, segs, nullptr, 1, tg, 0, nullptr, nullptr, nullptr, 2));
    return column_chain(p, p->physics_fused != 0, nmem, a.compute_sw, ug, vg, tg, qg, phig, pslg, a.bnd, a.albsfc, a.rad_state, a.utend,
                        a.vtend, a.ttend, a.qtend, a.out, pslg + g1, g1, sppt);
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
    NEED_PLAN(p);
    return ensure_workspace(p, &p->moist_grid, (size_t)(3 * p->tab.kx + 1) * grid_elems(p),
                            "allocating the moist-physics workspace (call spdy_moist_workspace before the capture)");
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
    RC(inverse_plain_one(p, 4, segs, p->moist_grid.g));
    const size_t L = (size_t)kx * grid_elems(p);
    const double *g = p->moist_grid.g;
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
    if (!p->d_radzonal) RC(dev_alloc(p, n * sizeof(double), &p->d_radzonal));
    // stream-ordered: work enqueued (or a graph replayed) before this call still reads the previous date, work after it the
    // new one.  The synchronisation keeps the host staging vector alive until the copy is done.
    std::vector<double> h(n);
    const std::vector<double> *f[5] = {&t.fsol, &t.ozone, &t.ozupp, &t.zenit, &t.stratz};
    for (int i = 0; i < 5; ++i) std::memcpy(h.data() + (size_t)i * t.il, f[i]->data(), sizeof(double) * t.il);
    return upload_sync(p, p->d_radzonal, h.data(), n * sizeof(double));
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

/* ---------------------------------------------------------------- surface fluxes (physics.f90:169-170), boundary layer (:193-205) */
int spdy_surface_set_orography(spdy_plan *p, const double *phis0)
{
    NEED_PLAN(p);
    NOT_CAPTURING(p, "spdy_surface_set_orography (host table build + upload)");
    const std::string err = p->tab.set_orography(phis0);
    if (!err.empty()) return fail(SPDY_ERR_ARG, "surface_set_orography: %s", err.c_str());
    if (p->device < 0) return SPDY_OK;
    HIP_TRY(hipSetDevice(p->device));
    const HostTables &t = p->tab;
    const size_t ncol = (size_t)t.ix * t.il, n = 2 * ncol + t.il;
    if (!p->d_orog) RC(dev_alloc(p, n * sizeof(double), &p->d_orog));
    // stream-ordered like spdy_radiation_set_date's fields; sqrt(coa(j)) per latitude, coa symmetric (geometry.f90:68-73)
    std::vector<double> h(n);
    std::memcpy(h.data(), t.phis0.data(), sizeof(double) * ncol);
    std::memcpy(h.data() + ncol, t.forog.data(), sizeof(double) * ncol);
    for (int j = 0; j < t.il; ++j) h[2 * ncol + j] = std::sqrt(t.coa_half[j < t.iy ? j : t.il - 1 - j]);
    return upload_sync(p, p->d_orog, h.data(), n * sizeof(double));
}

int spdy_surface_fluxes_dev(spdy_plan *p, int nb, const double *ug, const double *vg, const double *tg, const double *qg,
                            const double *phig, const double *pslg, const double *ssrd, const double *slrd,
                            const spdy_sfc_boundary *bnd, double *ts, double *fsfcu, double *flux3, const spdy_sfc_out *out)
{
    const bool ok = ug && vg && tg && qg && phig && pslg && ssrd && slrd && boundary_ok(bnd) && ts && fsfcu && flux3;
    RC(column_args(p, "surface fluxes", nb, false, !nb || ok, true));
    NEED_DEVICE(p);
    KERNEL(spdy::launch_surface_fluxes(sfc_cols(p, nb, ug, vg, tg, qg, phig, pslg, ssrd, slrd, bnd, ts, fsfcu, flux3, out), p->stream));
    return SPDY_OK;
}

int spdy_pbl_dev(spdy_plan *p, int nb, const double *qg, const double *phig, const double *pslg, const double *se, const double *rh,
                 const double *qsat, const int *icnv, const double *flux3, double *utend, double *vtend, double *ttend,
                 double *qtend, const spdy_pbl_out *out)
{
    const bool ok = qg && phig && pslg && se && rh && qsat && icnv && flux3 && utend && vtend && ttend && qtend;
    RC(column_args(p, "vertical diffusion", nb, false, !nb || ok));
    NEED_DEVICE(p);
    KERNEL(spdy::launch_pbl(pbl_cols(p, nb, qg, phig, pslg, se, rh, qsat, icnv, flux3, utend, vtend, ttend, qtend, out), p->stream));
    return SPDY_OK;
}

/* ---------------------------------------------------------------- the whole chain (physics.f90:110-205) */
int spdy_column_physics_workspace(spdy_plan *p)
{
    NEED_PLAN(p);
    RC(check_kx(p, "column physics"));
    return ensure_workspace(p, &p->physics_ws, (size_t)(3 * p->tab.kx + 12) * grid_elems(p) * p->max_batch,
                            "allocating the column-physics workspace (call spdy_column_physics_workspace before the capture)");
}

int spdy_column_physics_dev(spdy_plan *p, int nb, int compute_sw, const double *ug, const double *vg, const double *tg,
                            const double *qg, const double *phig, const double *pslg, const spdy_sfc_boundary *bnd,
                            const double *albsfc, double *rad_state, double *utend, double *vtend, double *ttend, double *qtend,
                            const spdy_column_physics_out *out)
{
    const bool ok = ug && vg && tg && qg && phig && pslg && boundary_ok(bnd) && (!compute_sw || albsfc) && rad_state && utend &&
                    vtend && ttend && qtend;
    RC(column_args(p, "column physics", nb, true, !nb || ok, true));
    NEED_DEVICE(p);
    RC(spdy_column_physics_workspace(p));
    // the workspace fields are each max_batch states long, so that a field's place does not depend on nb
    return column_chain(p, p->physics_fused == 1, nb, compute_sw, ug, vg, tg, qg, phig, pslg, bnd, albsfc, rad_state, utend, vtend,
                        ttend, qtend, out, p->physics_ws.g, grid_elems(p) * p->max_batch);
}

int spdy_column_physics_sppt_workspace(spdy_plan *p)
{
    RC(spdy_column_physics_workspace(p));
    return sppt_workspace(p, &p->sppt_ws, p->max_batch, "column physics",
                          "allocating the SPPT workspace (call spdy_column_physics_sppt_workspace before the capture)");
}

int spdy_column_physics_sppt_dev(spdy_plan *p, int nb, const double *d_pattern, const double *mu, int compute_sw, const double *ug,
                                 const double *vg, const double *tg, const double *qg, const double *phig, const double *pslg,
                                 const spdy_sfc_boundary *bnd, const double *albsfc, double *rad_state, double *utend, double *vtend,
                                 double *ttend, double *qtend, const spdy_column_physics_out *out)
{
    const bool ok = d_pattern && ug && vg && tg && qg && phig && pslg && boundary_ok(bnd) && (!compute_sw || albsfc) && rad_state &&
                    utend && vtend && ttend && qtend;
    RC(column_args(p, "column physics", nb, true, !nb || ok, true));
    NEED_DEVICE(p);
    RC(spdy_column_physics_sppt_workspace(p));
    const SpptUse use{d_pattern, mu, p->sppt_ws.g};
    return column_chain(p, p->physics_fused == 1, nb, compute_sw, ug, vg, tg, qg, phig, pslg, bnd, albsfc, rad_state, utend, vtend,
                        ttend, qtend, out, p->physics_ws.g, grid_elems(p) * p->max_batch, &use);
}

/* ---------------------------------------------------------------- the physics from spectra (physics.f90:94-205): one state, nmem members, each with SPPT */
int spdy_physics_workspace(spdy_plan *p)
{
    NEED_PLAN(p);
    RC(check_kx(p, "physics"));
    return physics_grids(p, &p->physics_grid, 1, "allocating the physics workspace (call spdy_physics_workspace before the capture)");
}

int spdy_physics_dev(spdy_plan *p, int compute_sw, const double *vor, const double *div, const double *t, const double *q,
                     const double *phi, const double *ps, const spdy_sfc_boundary *bnd, const double *albsfc, double *rad_state,
                     double *utend, double *vtend, double *ttend, double *qtend, const spdy_column_physics_out *out)
{
    const FromSpectra a{compute_sw, vor, div, t, q, phi, ps, bnd, albsfc, rad_state, utend, vtend, ttend, qtend, out};
    RC(physics_args(p, 1, false, a));
    RC(spdy_physics_workspace(p));
    return physics_from_spectra(p, 1, p->physics_grid, nullptr, a);
}

int spdy_ens_physics_workspace(spdy_plan *p, int nmem)
{
    RC(physics_members(p, nmem, true));
    return physics_grids(p, &p->ens_physics_grid, nmem,
                         "allocating the ensemble physics workspace (call spdy_ens_physics_workspace before the capture)");
}

int spdy_ens_physics_dev(spdy_plan *p, int nmem, int compute_sw, const double *vor, const double *div, const double *t, const double *q,
                         const double *phi, const double *ps, const spdy_sfc_boundary *bnd, const double *albsfc, double *rad_state,
                         double *utend, double *vtend, double *ttend, double *qtend, const spdy_column_physics_out *out)
{
    const FromSpectra a{compute_sw, vor, div, t, q, phi, ps, bnd, albsfc, rad_state, utend, vtend, ttend, qtend, out};
    RC(physics_args(p, nmem, true, a));
    RC(spdy_ens_physics_workspace(p, nmem));
    return physics_from_spectra(p, nmem, p->ens_physics_grid, nullptr, a);
}

int spdy_physics_sppt_workspace(spdy_plan *p)
{
    RC(spdy_physics_workspace(p));
    return sppt_workspace(p, &p->sppt_grid, 1, "physics",
                          "allocating the SPPT workspace (call spdy_physics_sppt_workspace before the capture)");
}

int spdy_physics_sppt_dev(spdy_plan *p, spdy_sppt *sp, int compute_sw, const double *vor, const double *div, const double *t,
                          const double *q, const double *phi, const double *ps, const spdy_sfc_boundary *bnd, const double *albsfc,
                          double *rad_state, double *utend, double *vtend, double *ttend, double *qtend,
                          const spdy_column_physics_out *out)
{
    const FromSpectra a{compute_sw, vor, div, t, q, phi, ps, bnd, albsfc, rad_state, utend, vtend, ttend, qtend, out};
    RC(physics_args(p, 1, false, a, true, sp));
    RC(spdy_physics_sppt_workspace(p));
    const SpptUse use{sp->d_pattern, sp->tab.mu.data(), p->sppt_grid.g};   // the pattern the last spdy_sppt_advance_dev left
    return physics_from_spectra(p, 1, p->physics_grid, &use, a);
}

int spdy_ens_physics_sppt_workspace(spdy_plan *p, int nmem)
{
    RC(spdy_ens_physics_workspace(p, nmem));
    return sppt_workspace(p, &p->ens_sppt_grid, nmem, "ens_physics",
                          "allocating the ensemble SPPT workspace (call spdy_ens_physics_sppt_workspace before the capture)");
}

int spdy_ens_physics_sppt_dev(spdy_plan *p, int nmem, spdy_sppt *sp, int compute_sw, const double *vor, const double *div,
                              const double *t, const double *q, const double *phi, const double *ps, const spdy_sfc_boundary *bnd,
                              const double *albsfc, double *rad_state, double *utend, double *vtend, double *ttend, double *qtend,
                              const spdy_column_physics_out *out)
{
    const FromSpectra a{compute_sw, vor, div, t, q, phi, ps, bnd, albsfc, rad_state, utend, vtend, ttend, qtend, out};
    RC(physics_args(p, nmem, true, a, true, sp));
    RC(spdy_ens_physics_sppt_workspace(p, nmem));
    // the patterns the last spdy_sppt_advance_dev left: nmem states back to back, what the chain takes as nb = nmem
    const SpptUse use{sp->d_pattern, sp->tab.mu.data(), p->ens_sppt_grid.g};
    return physics_from_spectra(p, nmem, p->ens_physics_grid, &use, a);
}

}  // extern "C"
