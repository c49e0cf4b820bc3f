// C ABI (include/spdy.h), second half: the spectral-space tail of a time step (horizontal diffusion, semi-implicit
// solve, spectral tendencies, geopotential, leapfrog/RAW filter) and the output path.  (Multi-GPU: spdy_api_shard.hip.)
// Geopotential, grid tendencies, spectral step and direct batch + spectral step have one body each, taking the member count:
// the single-state call and its ensemble form are one argument check (step_args) and one call of it, with nmem = 1 or nmem.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "spdy_plan.hpp"

using spdy::HostTables;
using namespace spdy_detail;

namespace {
// The argument checks of a step call (ens false: nmem = 1) and of its ensemble form, each in the order it documents.  Single state:
// the device first, then the state, the pointers and j1; neither kx nor max_batch is tested.  Ensemble: include/spdy.h, "ensemble time
// step" -- what needs no device first (a host-only plan answers it), the device last.  no_implicit / no_sigma: the failure's text
// where the call needs spdy_implicit_init / sigma levels, null where it does not.
int step_args(const spdy_plan *p, bool ens, int nmem, const char *what, const char *no_implicit, const char *no_sigma, bool ok_ptrs,
              int j1 = 1)
{
    if (!ens) NEED_DEVICE(p);
    NEED_PLAN(p);
    const int kx = p->tab.kx;
    if (ens) {
        if (nmem < 1) return fail(SPDY_ERR_ARG, "%s: nmem=%d < 1", what, nmem);
        if (nmem > 1 && kx > 16) return fail(SPDY_ERR_ARG, "%s: more than one member needs kx <= 16 (kx=%d)", what, kx);
        if ((long)p->max_batch < (long)nmem * (3 * kx + 1))
            return fail(SPDY_ERR_ARG, "%s: max_batch=%d must be >= nmem*(3*kx+1)=%ld", what, p->max_batch, (long)nmem * (3 * kx + 1));
    }
    if (no_implicit && !p->tab.implicit_ready) return fail(SPDY_ERR_STATE, "%s", no_implicit);
    if (no_sigma && !p->tab.sigma_ready) return fail(SPDY_ERR_STATE, "%s", no_sigma);
    if (!ok_ptrs) return fail(SPDY_ERR_ARG, "null device pointer");
    if (j1 != 1 && j1 != 2) return fail(SPDY_ERR_ARG, "j1 must be 1 or 2");
    if (ens) NEED_DEVICE(p);
    return SPDY_OK;
}

// The operations on nmem members, arguments checked (step_args): what the extern "C" pairs below enqueue.
int geopotential(spdy_plan *p, int nmem, const double *t, const double *phis, double *phi)
{
    KERNEL(spdy::launch_geopotential(p->dev, nmem, t, phis, phi, p->stream));
    return SPDY_OK;
}

int grid_tendencies(spdy_plan *p, int nmem, const double *ug, const double *vg, const double *tg, const double *vorg, const double *divg,
                    const double *trg, const double *px, const double *py, double *u_out, double *v_out, double *plain_out)
{
    const spdy::GridTend g{ug, vg, tg, vorg, divg, trg, px, py, u_out, v_out, plain_out, spdy::LevelShard{}, 0, 0, nullptr, nmem};
    KERNEL(spdy::launch_grid_tendencies(p->dev, g, p->stream));
    return SPDY_OK;
}

// what the spectral step takes behind the plan (and the member count), in the calls' order
struct StepFields {
    double *pvor, *pdiv, *pspec, *vor, *div, *t, *tr, *ps;
    const double *phis, *d_tcorh, *d_qcorh;
    double sdrag;
    int j1;
    double dt, eps, wil, *phi;
    bool ptrs() const { return pvor && pdiv && pspec && vor && div && t && tr && ps && phis && d_tcorh && d_qcorh && phi; }
};

// raw_u / raw_v: SpecStep (the pairs' spectra before vds, or null).  The plan option "ens_member_qcorh" is read here, when the call
// is enqueued; one member's qcorh is the same field either way.
int spectral_step(spdy_plan *p, int nmem, const StepFields &f, const double *raw_u, const double *raw_v)
{
    const int kx = p->tab.kx;
    if (kx > 16) {   // the fused kernel holds one level per thread row (64 x kx <= 1024 threads): issue the separate kernels.
                     // One member only (step_args), and never the raw spectra (use_raw63)
        RC(spdy_tendency_combine_dev(p, f.pdiv, f.pspec));
        const size_t L = (size_t)kx * spec_elems(p);
        double *divdt = f.pdiv, *tdt = f.pdiv + L, *trdt = f.pdiv + 2 * L, *psdt = f.pspec + 3 * L;
        RC(spdy_spectral_tendencies_dev(p, f.div, f.t, f.ps, f.phis, divdt, tdt, psdt, f.phi));
        RC(spdy_implicit_terms_dev(p, divdt, tdt, psdt));
        RC(spdy_hdiff_step_dev(p, f.vor, f.div, f.t, f.tr, f.d_tcorh, f.d_qcorh, f.sdrag, f.pvor, divdt, tdt, trdt));
        const spdy_step_op ops[5] = {{1, f.ps, psdt}, {kx, f.vor, f.pvor}, {kx, f.div, divdt}, {kx, f.t, tdt}, {kx, f.tr, trdt}};
        return spdy_step_fields_dev(p, 5, ops, f.j1, f.dt, f.eps, f.wil);
    }
    const spdy::SpecStep a{f.pvor, f.pdiv, f.pspec, f.vor, f.div, f.t, f.tr, f.ps, f.phis, f.d_tcorh, f.d_qcorh, f.phi, f.sdrag, f.dt,
                           f.eps, f.wil, f.j1, p->tab.ix == 4 * p->tab.iy, raw_u, raw_v, spdy::LevelShard{}, nullptr, 0, 0, nmem,
                           nmem > 1 && p->ens_member_qcorh};
    KERNEL(spdy::launch_spectral_step(p->dev, a, p->stream));
    return SPDY_OK;
}

// the direct batch of nmem members (3 nmem kx pairs, 3 nmem kx + nmem plain fields) and their spectral step
int direct_batch_spectral_step(spdy_plan *p, int nmem, const double *ug, const double *vg, const double *grid, int kcos,
                               const StepFields &f)
{
    const int P = 3 * nmem * p->tab.kx;
    // T63: the transform kernel leaves the pairs' spectra un-vds'ed in the plan's temporaries; the spectral step applies vds
    // where it reads them -- direct batch + everything after it = 2 launches instead of 3.  Every other plan and batch: the plain
    // direct batch, whatever form its size takes, then the spectral step
    const bool raw = use_raw63(p, P);
    RC(raw ? direct_batch_raw63(p, P, ug, vg, kcos, P + nmem, grid, f.pspec)
           : spdy_direct_batch_dev(p, P, ug, vg, f.pvor, f.pdiv, kcos, P + nmem, grid, f.pspec));
    return spectral_step(p, nmem, f, raw ? p->tmp_c : nullptr, raw ? p->tmp_d : nullptr);   // (they exist once the raw batch is enqueued)
}

// the first checks of the two ensemble output calls: what needs no device
int ens_output_members(const spdy_plan *p, int nmem)
{
    NEED_PLAN(p);
    if (nmem < 1) return fail(SPDY_ERR_ARG, "ens_output: nmem=%d < 1", nmem);
    const long need = (long)nmem * (3 * p->tab.kx + 1);
    if (p->max_batch < need) return fail(SPDY_ERR_ARG, "ens_output: max_batch=%d must be >= nmem*(3*kx+1)=%ld", p->max_batch, need);
    return SPDY_OK;
}

// the output groups of the ensemble output calls into a kernel's pointer tables: at least one, and in a given one all six fields,
// 8-byte aligned (a pair of floats per store)
int ens_output_groups(const spdy_output_fields *members, const spdy_output_fields *mean, const spdy_output_fields *spread, float **dm,
                      float **da, float **ds)
{
    if (!members && !mean && !spread) return fail(SPDY_ERR_ARG, "ens_output: no output group (members, mean, spread all NULL)");
    const spdy_output_fields *grp[3] = {members, mean, spread};
    float **dst[3] = {dm, da, ds};
    for (int g = 0; g < 3; ++g) {
        if (!grp[g]) continue;
        float *f[6] = {grp[g]->u, grp[g]->v, grp[g]->t, grp[g]->q, grp[g]->phi, grp[g]->ps};
        for (int i = 0; i < 6; ++i) {
            if (!f[i]) return fail(SPDY_ERR_ARG, "null device pointer");
            if (reinterpret_cast<uintptr_t>(f[i]) % 8) return fail(SPDY_ERR_ARG, "ens_output: output fields must be 8-byte aligned");
            dst[g][i] = f[i];
        }
    }
    return SPDY_OK;
}

// What the two ensemble output calls share in front of their epilogue kernel: the workspace (the device is checked here, last), then
// time level 1 of all members to the grid as ONE inverse batch, read in place: nmem*kx pairs, the segments t | q | phi | ps, into
// ens_out_grid as u | v | t | q | phi (nmem*kx grids each) | ps (nmem)
int ens_output_inverse(spdy_plan *p, int nmem, const double *vor, const double *div, const double *t, const double *q, const double *phi,
                       const double *ps)
{
    RC(spdy_ens_output_workspace(p, nmem));
    const int nk = nmem * p->tab.kx;
    const size_t L = (size_t)nk * grid_elems(p);
    double *ug = p->ens_out_grid.g, *vg = ug + L, *tg = ug + 2 * L;
    const spdy_spec_seg segs[SPDY_MAX_SPEC_SEGS] = {{nk, t}, {nk, q}, {nk, phi}, {nmem, ps}};
    return spdy_inverse_batch_segs_dev(p, nk, vor, div, ug, vg, 2, SPDY_MAX_SPEC_SEGS, segs, nullptr, 1, tg, 0, nullptr, nullptr, nullptr, 2);
}

// the pressure-level calls' own checks, in the header's order, and what they give the kernel: the targets (the logarithms of the
// log-p coordinate are formed here, on the host: the values a captured call keeps) and the plan's level table
int plev_levels(const spdy_plan *p, int nlev, const double *plev, int coord, spdy::PlevOutput *c)
{
    const double p0 = static_cast<double>(1.e+5f);
    if (nlev < 1 || nlev > SPDY_MAX_PLEV) return fail(SPDY_ERR_ARG, "ens_output_pressure: nlev=%d outside [1, %d]", nlev, (int)SPDY_MAX_PLEV);
    if (!plev) return fail(SPDY_ERR_ARG, "ens_output_pressure: null plev");
    for (int l = 0; l < nlev; ++l)
        if (!std::isfinite(plev[l]) || !(plev[l] > 0.0))
            return fail(SPDY_ERR_ARG, "ens_output_pressure: plev[%d]=%g must be finite and > 0", l, plev[l]);
    if (coord != SPDY_PLEV_LINEAR_P && coord != SPDY_PLEV_LOG_P) return fail(SPDY_ERR_ARG, "ens_output_pressure: unknown coord=%d", coord);
    if (!p->tab.sigma_ready) return fail(SPDY_ERR_STATE, "ens_output_pressure needs sigma levels");
    const bool log_p = coord == SPDY_PLEV_LOG_P;
    c->nlev = nlev; c->log_p = log_p ? 1 : 0;
    c->qfac = static_cast<double>(1.0e-3f); c->grav = p->tab.grav; c->p0 = p0;
    c->lv.kx = p->tab.kx;
    for (int k = 0; k < p->tab.kx; ++k) c->lv.lev[k] = log_p ? std::log(p->tab.fsg[k]) : p->tab.fsg[k];
    for (int l = 0; l < nlev; ++l) c->x[l] = log_p ? std::log(plev[l] / p0) : plev[l];
    return SPDY_OK;
}

int plev_outputs(const spdy_output_fields *members, const spdy_output_fields *mean, const spdy_output_fields *spread, float *below,
                 spdy::PlevOutput *c)
{
    RC(ens_output_groups(members, mean, spread, c->members, c->mean, c->spread));
    if (reinterpret_cast<uintptr_t>(below) % 8) return fail(SPDY_ERR_ARG, "ens_output: output fields must be 8-byte aligned");
    c->below = below;
    return SPDY_OK;
}
}  // namespace

extern "C" {

/* ---------------------------------------------------------------- sigma levels */
int spdy_plan_set_sigma(spdy_plan *p, const double *hsg)
{
    NEED_PLAN(p);
    NOT_CAPTURING(p, "spdy_plan_set_sigma");
    const std::string err = p->tab.set_sigma(hsg);
    if (!err.empty()) return fail(SPDY_ERR_ARG, "set_sigma: %s", err.c_str());
    if (p->device < 0) return SPDY_OK;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return upload_level_tables(p);
}

/* ---------------------------------------------------------------- horizontal diffusion */
int spdy_hdiff_dev(spdy_plan *p, int nlev, const double *field, const double *fdt_in, const double *d_dmp,
                   const double *d_dmp1, double *fdt_out)
{
    NEED_DEVICE(p);
    if (nlev < 0) return fail(SPDY_ERR_ARG, "nlev < 0");
    if (nlev && (!field || !fdt_in || !d_dmp || !d_dmp1 || !fdt_out)) return fail(SPDY_ERR_ARG, "null device pointer");
    KERNEL(spdy::launch_hdiff(p->dev, nlev, field, fdt_in, d_dmp, d_dmp1, fdt_out, p->stream));
    return SPDY_OK;
}

int spdy_hdiff_multi_dev(spdy_plan *p, int nops, const spdy_hdiff_op *ops)
{
    NEED_DEVICE(p);
    if (nops < 0 || nops > SPDY_HDIFF_MAX_OPS || (nops && !ops)) return fail(SPDY_ERR_ARG, "nops=%d outside [0, %d]", nops, (int)SPDY_HDIFF_MAX_OPS);
    spdy::HdiffOps h{};
    h.nops = nops;
    for (int i = 0; i < nops; ++i) {
        if (ops[i].nlev < 0 || (ops[i].nlev && (!ops[i].field || !ops[i].fdt_in || !ops[i].d_dmp || !ops[i].d_dmp1 || !ops[i].fdt_out)))
            return fail(SPDY_ERR_ARG, "hdiff op %d: bad argument", i);
        h.nlev[i] = ops[i].nlev; h.field[i] = ops[i].field; h.fdt[i] = ops[i].fdt_in;
        h.dmp[i] = ops[i].d_dmp; h.dmp1[i] = ops[i].d_dmp1; h.out[i] = ops[i].fdt_out;
    }
    KERNEL(spdy::launch_hdiff_multi(p->dev, h, p->stream));
    return SPDY_OK;
}

int spdy_hdiff(spdy_plan *p, int nlev, const double *field, const double *fdt_in, const double *dmp,
               const double *dmp1, double *fdt_out)
{
    NEED_DEVICE(p);
    RC(check_batch(p, nlev));
    if (nlev && (!field || !fdt_in || !dmp || !dmp1 || !fdt_out)) return fail(SPDY_ERR_ARG, "null pointer");
    HostCall c(p);
    RC(c.open());
    const size_t n = nlev * spec_elems(p), tn = (size_t)p->tab.mx * p->tab.nx;
    RC(c.in(0, field, n));
    RC(c.in(1, fdt_in, n));
    RC(c.in(2, dmp, tn));                       // both damping tables share slot 2 (2*mx*nx <= ix*il) ...
    RC(c.in(2, dmp1, tn, tn));
    RC(spdy_hdiff_dev(p, nlev, c[0], c[1], c[2], c[2] + tn, c[3]));   // ... so the result has its own buffer
    RC(c.out(fdt_out, 3, n));
    return c.finish();
}

int spdy_device_table(spdy_plan *p, const char *name, const double **d_ptr)
{
    NEED_DEVICE(p);
    if (!name || !d_ptr) return fail(SPDY_ERR_ARG, "null argument");
    static const char *names[6] = {"dmp", "dmpd", "dmps", "dmp1", "dmp1d", "dmp1s"};
    for (int i = 0; i < 6; ++i)
        if (!std::strcmp(name, names[i])) {
            if (i >= 3 && !p->tab.implicit_ready) return fail(SPDY_ERR_STATE, "%s needs implicit_init first", name);
            *d_ptr = p->d_dmp[i];
            return SPDY_OK;
        }
    return fail(SPDY_ERR_ARG, "no device table '%s'", name);
}

/* ---------------------------------------------------------------- semi-implicit solve */
int spdy_implicit_init(spdy_plan *p, double dt)
{
    NEED_PLAN(p);
    NOT_CAPTURING(p, "spdy_implicit_init (host table build + blocking upload)");
    const std::string err = p->tab.build_implicit(dt);
    if (!err.empty()) return fail(SPDY_ERR_UNSUPPORTED, "implicit_init: %s", err.c_str());
    if (p->device < 0) return SPDY_OK;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    const HostTables &t = p->tab;
    const size_t tn = sizeof(double) * t.mx * t.nx;
    const std::vector<double> *d1[3] = {&t.dmp1, &t.dmp1d, &t.dmp1s};
    for (int i = 0; i < 3; ++i) HIP_TRY(hipMemcpy(p->d_dmp[3 + i], d1[i]->data(), tn, hipMemcpyHostToDevice));
    struct { double *dst; const std::vector<double> *src; } up[6] = {
        {p->d_xd, &t.xd}, {p->d_xc, &t.xc}, {p->d_xj, &t.xj}, {p->d_tref1, &t.tref1}, {p->d_dhsx, &t.dhsx}, {p->d_elz, &t.elz}};
    for (auto &u : up) HIP_TRY(hipMemcpy(u.dst, u.src->data(), u.src->size() * sizeof(double), hipMemcpyHostToDevice));
    {   // row-major, row-padded copies: element (k, k1) of a column-major kx x kx matrix at [k][k1]
        const int kx = t.kx, kxp = (kx + 1) & ~1, nl = t.mx + t.nx + 1;
        std::vector<double> xt((size_t)kx * kxp * (2 + nl), 0.0);
        auto tr = [&](const double *src, double *dst) {
            for (int k = 0; k < kx; ++k)
                for (int k1 = 0; k1 < kx; ++k1) dst[(size_t)k * kxp + k1] = src[k + (size_t)kx * k1];
        };
        tr(t.xd.data(), xt.data());
        tr(t.xc.data(), xt.data() + (size_t)kx * kxp);
        for (int l = 0; l < nl; ++l) tr(t.xj.data() + (size_t)kx * kx * l, xt.data() + (size_t)kx * kxp * (2 + l));
        HIP_TRY(hipMemcpy(p->d_xt, xt.data(), xt.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    return upload_level_tables(p);
}

int spdy_implicit_terms_dev(spdy_plan *p, double *divdt, double *tdt, double *psdt)
{
    NEED_DEVICE(p);
    if (!p->tab.implicit_ready) return fail(SPDY_ERR_STATE, "implicit_terms before implicit_init");
    if (!divdt || !tdt || !psdt) return fail(SPDY_ERR_ARG, "null pointer");
    KERNEL(spdy::launch_implicit(p->dev, divdt, tdt, psdt, p->stream));
    return SPDY_OK;
}

int spdy_implicit_terms(spdy_plan *p, double *divdt, double *tdt, double *psdt)
{
    NEED_DEVICE(p);
    if (p->max_batch < p->tab.kx) return fail(SPDY_ERR_ARG, "max_batch must be >= kx for the host implicit_terms");
    if (!divdt || !tdt || !psdt) return fail(SPDY_ERR_ARG, "null pointer");
    HostCall c(p);
    RC(c.open());
    double *const arr[3] = {divdt, tdt, psdt};
    const size_t n[3] = {p->tab.kx * spec_elems(p), p->tab.kx * spec_elems(p), spec_elems(p)};
    for (int i = 0; i < 3; ++i) RC(c.in(i, arr[i], n[i]));
    RC(spdy_implicit_terms_dev(p, c[0], c[1], c[2]));
    for (int i = 0; i < 3; ++i) RC(c.out(arr[i], i, n[i]));
    return c.finish();
}

/* ---------------------------------------------------------------- spectral side of a time step */
int spdy_geopotential_dev(spdy_plan *p, const double *t, const double *phis, double *phi)
{
    RC(step_args(p, false, 1, "geopotential", nullptr, "geopotential needs sigma levels (kx in {5,7,8} or spdy_plan_set_sigma)",
                 t && phis && phi));
    return geopotential(p, 1, t, phis, phi);
}

int spdy_ens_geopotential_dev(spdy_plan *p, int nmem, const double *t, const double *phis, double *phi)
{
    RC(step_args(p, true, nmem, "ens_geopotential", nullptr, "ens_geopotential needs sigma levels", t && phis && phi));
    return geopotential(p, nmem, t, phis, phi);
}

int spdy_geopotential(spdy_plan *p, const double *t, const double *phis, double *phi)
{
    NEED_DEVICE(p);
    if (p->max_batch < p->tab.kx) return fail(SPDY_ERR_ARG, "max_batch must be >= kx for the host get_geopotential");
    if (!t || !phis || !phi) return fail(SPDY_ERR_ARG, "null pointer");
    HostCall c(p);
    RC(c.open());
    const size_t n = p->tab.kx * spec_elems(p);
    RC(c.in(0, t, n));
    RC(c.in(1, phis, spec_elems(p)));
    RC(spdy_geopotential_dev(p, c[0], c[1], c[2]));
    RC(c.out(phi, 2, n));
    return c.finish();
}

int spdy_spectral_tendencies_dev(spdy_plan *p, const double *div, const double *t, const double *ps, const double *phis,
                                 double *divdt, double *tdt, double *psdt, double *phi)
{
    NEED_DEVICE(p);
    if (!p->tab.implicit_ready) return fail(SPDY_ERR_STATE, "spectral_tendencies needs the reference temperature profile: call spdy_implicit_init first");
    if (!div || !t || !ps || !phis || !divdt || !tdt || !psdt || !phi) return fail(SPDY_ERR_ARG, "null device pointer");
    KERNEL(spdy::launch_spectral_tendencies(p->dev, div, t, ps, phis, divdt, tdt, psdt, phi, p->stream));
    return SPDY_OK;
}

int spdy_hdiff_step_dev(spdy_plan *p, const double *vor, const double *div, const double *t, const double *tr,
                        const double *d_tcorh, const double *d_qcorh, double sdrag,
                        double *vordt, double *divdt, double *tdt, double *trdt)
{
    NEED_DEVICE(p);
    if (!p->tab.implicit_ready) return fail(SPDY_ERR_STATE, "hdiff_step needs dmp1*: call spdy_implicit_init first");
    if (!p->tab.sigma_ready) return fail(SPDY_ERR_STATE, "hdiff_step needs sigma levels");
    if (!vor || !div || !t || !d_tcorh || !vordt || !divdt || !tdt) return fail(SPDY_ERR_ARG, "null device pointer");
    if ((tr != nullptr) != (trdt != nullptr) || (tr && !d_qcorh)) return fail(SPDY_ERR_ARG, "tracer arguments: tr, trdt and qcorh go together");
    spdy::HdiffStep h{vor, div, t, tr, vordt, divdt, tdt, trdt, d_tcorh, d_qcorh,
                      p->d_dmp[0], p->d_dmp[1], p->d_dmp[2], p->d_dmp[3], p->d_dmp[4], p->d_dmp[5], sdrag};
    KERNEL(spdy::launch_hdiff_step(p->dev, h, p->stream));
    return SPDY_OK;
}

int spdy_step_fields_dev(spdy_plan *p, int nops, const spdy_step_op *ops, int j1, double dt, double eps, double wil)
{
    NEED_DEVICE(p);
    if (nops < 0 || nops > SPDY_STEP_MAX_OPS || (nops && !ops)) return fail(SPDY_ERR_ARG, "nops=%d outside [0, %d]", nops, (int)SPDY_STEP_MAX_OPS);
    if (j1 != 1 && j1 != 2) return fail(SPDY_ERR_ARG, "j1 must be 1 or 2");
    spdy::StepOps s{};
    s.nops = nops;
    for (int i = 0; i < nops; ++i) {
        if (ops[i].nlev < 0 || (ops[i].nlev && (!ops[i].field || !ops[i].fdt))) return fail(SPDY_ERR_ARG, "step op %d: bad argument", i);
        s.nlev[i] = ops[i].nlev; s.field[i] = ops[i].field; s.fdt[i] = ops[i].fdt;
    }
    // time_stepping.f90:155-157: the tendency is truncated first whenever ix == 4*iy (true for T30 and T63)
    const int do_trunct = p->tab.ix == 4 * p->tab.iy;
    KERNEL(spdy::launch_step_fields(p->dev, s, j1, dt, eps, wil, do_trunct, p->stream));
    return SPDY_OK;
}

int spdy_step_field(spdy_plan *p, int nlev, int j1, double dt, double eps, double wil, double *field, double *fdt)
{
    NEED_DEVICE(p);
    RC(check_batch(p, 2 * nlev));
    if (nlev && (!field || !fdt)) return fail(SPDY_ERR_ARG, "null pointer");
    HostCall c(p);
    RC(c.open());
    const size_t n = nlev * spec_elems(p);
    RC(c.in(0, field, 2 * n));
    RC(c.in(1, fdt, n));
    const spdy_step_op op{nlev, c[0], c[1]};
    RC(spdy_step_fields_dev(p, 1, &op, j1, dt, eps, wil));
    RC(c.out(field, 0, 2 * n));
    RC(c.out(fdt, 1, n));
    return c.finish();
}


/* ---------------------------------------------------------------- grid-space dynamical tendencies */
int spdy_grid_tendencies_dev(spdy_plan *p, const double *ug, const double *vg, const double *tg, const double *vorg, const double *divg,
                             const double *trg, const double *px, const double *py, double *u_out, double *v_out, double *plain_out)
{
    RC(step_args(p, false, 1, "grid_tendencies", "grid_tendencies needs the reference temperature profile: call spdy_implicit_init first",
                 nullptr, ug && vg && tg && vorg && divg && trg && px && py && u_out && v_out && plain_out));
    return grid_tendencies(p, 1, ug, vg, tg, vorg, divg, trg, px, py, u_out, v_out, plain_out);
}

int spdy_ens_grid_tendencies_dev(spdy_plan *p, int nmem, const double *ug, const double *vg, const double *tg, const double *vorg,
                                 const double *divg, const double *trg, const double *px, const double *py, double *u_out,
                                 double *v_out, double *plain_out)
{
    RC(step_args(p, true, nmem, "ens_grid_tendencies", "ens_grid_tendencies needs spdy_implicit_init first", nullptr,
                 ug && vg && tg && vorg && divg && trg && px && py && u_out && v_out && plain_out));
    return grid_tendencies(p, nmem, ug, vg, tg, vorg, divg, trg, px, py, u_out, v_out, plain_out);
}

int spdy_tendency_combine_dev(spdy_plan *p, double *pdiv, double *pspec)
{
    NEED_DEVICE(p);
    if (!pdiv || !pspec) return fail(SPDY_ERR_ARG, "null device pointer");
    KERNEL(spdy::launch_tendency_combine(p->dev, pdiv, pspec, p->stream));
    return SPDY_OK;
}

int spdy_spectral_step_dev(spdy_plan *p, double *pvor, double *pdiv, double *pspec, double *vor, double *div, double *t, double *tr,
                           double *ps, const double *phis, const double *d_tcorh, const double *d_qcorh, double sdrag, int j1, double dt,
                           double eps, double wil, double *phi)
{
    const StepFields f{pvor, pdiv, pspec, vor, div, t, tr, ps, phis, d_tcorh, d_qcorh, sdrag, j1, dt, eps, wil, phi};
    RC(step_args(p, false, 1, "spectral_step", "spectral_step needs spdy_implicit_init first", "spectral_step needs sigma levels",
                 f.ptrs(), j1));
    return spectral_step(p, 1, f, nullptr, nullptr);
}

int spdy_ens_spectral_step_dev(spdy_plan *p, int nmem, double *pvor, double *pdiv, double *pspec, double *vor, double *div, double *t,
                               double *tr, double *ps, const double *phis, const double *d_tcorh, const double *d_qcorh, double sdrag,
                               int j1, double dt, double eps, double wil, double *phi)
{
    const StepFields f{pvor, pdiv, pspec, vor, div, t, tr, ps, phis, d_tcorh, d_qcorh, sdrag, j1, dt, eps, wil, phi};
    RC(step_args(p, true, nmem, "ens_spectral_step", "ens_spectral_step needs spdy_implicit_init first",
                 "ens_spectral_step needs sigma levels", f.ptrs(), j1));
    return spectral_step(p, nmem, f, nullptr, nullptr);
}

// The device, then the spectral step's state, every pointer and j1 are checked before the direct batch is enqueued (its own batch-size
// checks follow): a call that fails has put nothing on the stream, or into a capture.
int spdy_direct_batch_spectral_step_dev(spdy_plan *p, const double *ug, const double *vg, const double *grid, int kcos, double *pvor,
                                        double *pdiv, double *pspec, double *vor, double *div, double *t, double *tr, double *ps,
                                        const double *phis, const double *d_tcorh, const double *d_qcorh, double sdrag, int j1, double dt,
                                        double eps, double wil, double *phi)
{
    const StepFields f{pvor, pdiv, pspec, vor, div, t, tr, ps, phis, d_tcorh, d_qcorh, sdrag, j1, dt, eps, wil, phi};
    RC(step_args(p, false, 1, "spectral_step", "spectral_step needs spdy_implicit_init first", "spectral_step needs sigma levels",
                 ug && vg && grid && f.ptrs(), j1));
    return direct_batch_spectral_step(p, 1, ug, vg, grid, kcos, f);
}

int spdy_ens_direct_batch_spectral_step_dev(spdy_plan *p, int nmem, const double *ug, const double *vg, const double *grid, int kcos,
                                            double *pvor, double *pdiv, double *pspec, double *vor, double *div, double *t, double *tr,
                                            double *ps, const double *phis, const double *d_tcorh, const double *d_qcorh, double sdrag,
                                            int j1, double dt, double eps, double wil, double *phi)
{
    const StepFields f{pvor, pdiv, pspec, vor, div, t, tr, ps, phis, d_tcorh, d_qcorh, sdrag, j1, dt, eps, wil, phi};
    RC(step_args(p, true, nmem, "ens_direct_batch_spectral_step", "ens_direct_batch_spectral_step needs spdy_implicit_init first",
                 "ens_direct_batch_spectral_step needs sigma levels", ug && vg && grid && f.ptrs(), j1));
    return direct_batch_spectral_step(p, nmem, ug, vg, grid, kcos, f);
}

/* ---------------------------------------------------------------- output path */
int spdy_output_workspace(spdy_plan *p)
{
    NEED_PLAN(p);
    const char *what = "allocating the output workspace (call spdy_output_workspace before the capture)";
    const int kx = p->tab.kx;
    RC(ensure_workspace(p, &p->out_grid, (size_t)(5 * kx + 1) * grid_elems(p), what));
    return ensure_workspace(p, &p->out_spec, (size_t)(3 * kx + 1) * spec_elems(p), what);
}

int spdy_output_batch_dev(spdy_plan *p, const double *vor, const double *div, const double *t, const double *q, const double *phi,
                          const double *ps, float *u_out, float *v_out, float *t_out, float *q_out, float *phi_out, float *ps_out)
{
    NEED_DEVICE(p);
    if (!vor || !div || !t || !q || !phi || !ps || !u_out || !v_out || !t_out || !q_out || !phi_out || !ps_out)
        return fail(SPDY_ERR_ARG, "null device pointer");
    const int kx = p->tab.kx;
    if (p->max_batch < 3 * kx + 1) return fail(SPDY_ERR_ARG, "max_batch must be >= 3*kx+1 for the output batch");
    RC(spdy_output_workspace(p));
    const size_t gs = grid_elems(p), ss = spec_elems(p);
    // t, q, phi levels and ps into one stack: the whole snapshot is then one transform launch
    spdy::GatherOps g{};
    g.nops = 4;
    const double *src[4] = {t, q, phi, ps};
    for (int i = 0; i < 4; ++i) { g.nfld[i] = i < 3 ? kx : 1; g.src[i] = src[i]; g.dst[i] = p->out_spec.g + (size_t)i * kx * ss; }
    KERNEL(spdy::launch_gather_spectra(p->dev, g, p->stream));
    double *ug = p->out_grid.g, *vg = ug + (size_t)kx * gs, *plain = vg + (size_t)kx * gs;
    RC(spdy_inverse_batch_dev(p, kx, vor, div, ug, vg, 2, 3 * kx + 1, p->out_spec.g, nullptr, 1, plain));
    // input_output.f90:200-206: u, v, t as they are; q*1.0e-3; phi/grav; p0*exp(ps) -- then real(., sp)
    spdy::OutputCast c{};
    c.nops = 6;
    float *dst[6] = {u_out, v_out, t_out, q_out, phi_out, ps_out};
    const int kind[6] = {0, 0, 0, 1, 2, 3};
    const double fac[6] = {1.0, 1.0, 1.0, static_cast<double>(1.0e-3f), p->tab.grav, static_cast<double>(1.e+5f)};
    for (int i = 0; i < 6; ++i) {
        c.nfld[i] = i < 5 ? kx : 1; c.kind[i] = kind[i]; c.factor[i] = fac[i];
        c.src[i] = p->out_grid.g + (size_t)i * kx * gs; c.dst[i] = dst[i];
    }
    KERNEL(spdy::launch_output_cast(p->dev, c, p->stream));
    return SPDY_OK;
}

/* ---------------------------------------------------------------- ensemble output (include/spdy.h, "ensemble output") */
int spdy_ens_output_workspace(spdy_plan *p, int nmem)
{
    RC(ens_output_members(p, nmem));
    // with the Fourier workspace: the operator route of the T63 inverse launch keeps (vor, div) -> (U, V) in the plan's temporaries
    return ensure_workspace(p, &p->ens_out_grid, (size_t)(5 * p->tab.kx + 1) * grid_elems(p) * nmem,
                            "allocating the ensemble output workspace (call spdy_ens_output_workspace before the capture)", true);
}

int spdy_ens_output_batch_dev(spdy_plan *p, int nmem, const double *vor, const double *div, const double *t, const double *q,
                              const double *phi, const double *ps, const int *d_use, const spdy_output_fields *members,
                              const spdy_output_fields *mean, const spdy_output_fields *spread)
{
    RC(ens_output_members(p, nmem));
    if (!vor || !div || !t || !q || !phi || !ps) return fail(SPDY_ERR_ARG, "null device pointer");
    spdy::EnsOutput c{};
    RC(ens_output_groups(members, mean, spread, c.members, c.mean, c.spread));
    RC(ens_output_inverse(p, nmem, vor, div, t, q, phi, ps));
    // input_output.f90:200-206, as spdy_output_batch_dev: u, v, t as they are; q*1.0e-3; phi/grav; p0*exp(ps) -- then real(., sp)
    const int kind[6] = {0, 0, 0, 1, 2, 3};
    const double fac[6] = {1.0, 1.0, 1.0, static_cast<double>(1.0e-3f), p->tab.grav, static_cast<double>(1.e+5f)};
    for (int i = 0; i < 6; ++i) { c.kind[i] = kind[i]; c.factor[i] = fac[i]; }
    c.nmem = nmem; c.kx = p->tab.kx; c.src = p->ens_out_grid.g; c.use = d_use;
    KERNEL(spdy::launch_ens_output(p->dev, c, p->stream));
    return SPDY_OK;
}

/* ---------------------------------------------------------------- pressure-level output (include/spdy.h, "pressure-level output") */
int spdy_ens_output_pressure_grid_dev(spdy_plan *p, int nmem, const double *grid, const int *d_use, int nlev, const double *plev, int coord,
                                      const spdy_output_fields *members, const spdy_output_fields *mean,
                                      const spdy_output_fields *spread, float *below)
{
    NEED_PLAN(p);
    if (nmem < 1) return fail(SPDY_ERR_ARG, "ens_output_pressure: nmem=%d < 1", nmem);
    spdy::PlevOutput c{};
    RC(plev_levels(p, nlev, plev, coord, &c));
    if (!grid) return fail(SPDY_ERR_ARG, "null device pointer");
    if (reinterpret_cast<uintptr_t>(grid) % 16) return fail(SPDY_ERR_ARG, "ens_output_pressure: the grids must be 16-byte aligned");
    RC(plev_outputs(members, mean, spread, below, &c));
    NEED_DEVICE(p);
    c.nmem = nmem; c.src = grid; c.use = d_use;
    KERNEL(spdy::launch_plev_output(p->dev, c, p->stream));
    return SPDY_OK;
}

int spdy_ens_output_pressure_dev(spdy_plan *p, int nmem, const double *vor, const double *div, const double *t, const double *q,
                                 const double *phi, const double *ps, const int *d_use, int nlev, const double *plev, int coord,
                                 const spdy_output_fields *members, const spdy_output_fields *mean, const spdy_output_fields *spread,
                                 float *below)
{
    RC(ens_output_members(p, nmem));
    spdy::PlevOutput c{};
    RC(plev_levels(p, nlev, plev, coord, &c));
    if (!vor || !div || !t || !q || !phi || !ps) return fail(SPDY_ERR_ARG, "null device pointer");
    RC(plev_outputs(members, mean, spread, below, &c));
    RC(ens_output_inverse(p, nmem, vor, div, t, q, phi, ps));
    c.nmem = nmem; c.src = p->ens_out_grid.g; c.use = d_use;
    KERNEL(spdy::launch_plev_output(p->dev, c, p->stream));
    return SPDY_OK;
}

// The single state: the one-member case of the ensemble call with the `members` group only, as every single-state call of the
// step is the one-member case of its ensemble form.
int spdy_output_pressure_dev(spdy_plan *p, const double *vor, const double *div, const double *t, const double *q, const double *phi,
                             const double *ps, int nlev, const double *plev, int coord, float *u_out, float *v_out, float *t_out,
                             float *q_out, float *phi_out, float *ps_out)
{
    const spdy_output_fields one{u_out, v_out, t_out, q_out, phi_out, ps_out};
    return spdy_ens_output_pressure_dev(p, 1, vor, div, t, q, phi, ps, nullptr, nlev, plev, coord, &one, nullptr, nullptr, nullptr);
}

}  // extern "C"
