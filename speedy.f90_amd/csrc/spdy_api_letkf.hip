// C ABI of the ensemble analysis (include/spdy.h, "ensemble analysis"): the observation ingestion on the host, the
// analysis of a gridded ensemble, the five-launch analysis of an ensemble's spectral state, and the tables and the buffer of weight
// interpolation (one launch more).  Kernels: csrc/spdy_letkf.hip.
#include <cmath>
#include <cstring>
#include <vector>

#include "spdy_plan.hpp"

using namespace spdy_detail;

namespace {
constexpr double kPi = 3.14159265358979323846;
constexpr size_t kLdsLimit = 160 * 1024;      // LDS of a gfx950 compute unit

// bilinear stencil of one observation: four grid points (j0,i0) (j0,i1) (j1,i0) (j1,i1) and their weights.  Columns are
// periodic; poleward of the outermost row that row has weight 1.
void stencil(const spdy_letkf *l, double lon, double lat, int *idx, double *wgt)
{
    const int ix = l->plan->tab.ix, il = l->plan->tab.il;
    double x = std::fmod(lon, 360.0);
    if (x < 0.0) x += 360.0;
    x = x / (360.0 / ix);
    int i0 = (int)std::floor(x);
    double a = x - i0;
    if (i0 >= ix) { i0 = 0; a = 0.0; }        // -1e-20 + 360 rounds to 360
    const int i1 = (i0 + 1) % ix;
    int j0, j1;
    double b = 0.0;
    const std::vector<double> &lt = l->lat;
    if (lat <= lt[0]) j0 = j1 = 0;
    else if (lat >= lt[il - 1]) j0 = j1 = il - 1;
    else {
        j0 = 0;
        while (j0 + 2 < il && lat >= lt[j0 + 1]) ++j0;
        j1 = j0 + 1;
        b = (lat - lt[j0]) / (lt[j1] - lt[j0]);
    }
    idx[0] = j0 * ix + i0; idx[1] = j0 * ix + i1; idx[2] = j1 * ix + i0; idx[3] = j1 * ix + i1;
    wgt[0] = (1.0 - a) * (1.0 - b); wgt[1] = a * (1.0 - b); wgt[2] = (1.0 - a) * b; wgt[3] = a * b;
}

void unit_vector(double lon, double lat, double *u)
{
    const double rl = lon * (kPi / 180.0), rp = lat * (kPi / 180.0);
    u[0] = std::cos(rp) * std::cos(rl); u[1] = std::cos(rp) * std::sin(rl); u[2] = std::sin(rp);
}

int upload(spdy_plan *p, void *dst, const void *src, size_t bytes)
{
    if (bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, p->stream));
    return SPDY_OK;
}

// the argument checks the two analysis calls share, in the documented order; the device last
int analysis_ready(spdy_letkf *l, bool ptrs_ok)
{
    NEED_LIVE(l, "analysis object");
    if (!l->loc_set) return fail(SPDY_ERR_STATE, "letkf: spdy_letkf_set_localization first");
    if (!ptrs_ok) return fail(SPDY_ERR_ARG, "null device pointer");
    NEED_DEVICE(l->plan);
    return SPDY_OK;
}

int analyse_grid(spdy_letkf *l, const double *const *x, double *const *dx)
{
    spdy_plan *p = l->plan;
    const int kx = p->tab.kx, ncol = (int)grid_elems(p);
    spdy::LetkfObs o{};
    o.nobs = l->nobs; o.nmem = l->nmem; o.kx = kx; o.ncol = ncol;
    o.var = l->d_var; o.lev = l->d_lev; o.sidx = l->d_sidx; o.swgt = l->d_swgt; o.value = l->d_value;
    o.hx = l->d_hx; o.hxmean = l->d_hxmean; o.y = l->d_y; o.dep = l->d_dep;
    spdy::LetkfCols c{};
    c.nobs = l->nobs; c.nmem = l->nmem; c.kx = kx; c.ncol = ncol; c.nlv = l->nlv;
    c.ch = l->sigma_h * std::sqrt(10.0 / 3.0); c.cv = l->sigma_v > 0.0 ? l->sigma_v * std::sqrt(10.0 / 3.0) : 0.0;
    c.diag = (double)(l->nmem - 1) / l->rho;
    c.colunit = l->d_colunit; c.lnfsg = l->d_lnfsg; c.ounit = l->d_ounit; c.olns = l->d_olns; c.rinv = l->d_rinv;
    c.y = l->d_y; c.dep = l->d_dep;
    for (int v = 0; v < spdy::LETKF_VARS; ++v) { o.x[v] = x[v]; c.x[v] = x[v]; c.dx[v] = dx[v]; }
    if (l->npobs) {
        // observations at a pressure: the kernel that interpolates per member, in letkf_obs_kernel's place; it writes ln sigma_o of
        // those observations into olns and this call's copy of rinv, 0 where an observation is out of its column
        spdy::LetkfPObs po{};
        po.o = o; po.atp = l->d_atp; po.lnp = l->d_lnp; po.rinv = l->d_rinv; po.olns = l->d_olns; po.used = l->d_used; po.reff = l->d_reff;
        po.lv.kx = kx;
        for (int k = 0; k < kx; ++k) po.lv.lev[k] = l->lnfsg[k];
        c.rinv = l->d_reff;
        KERNEL(spdy::launch_letkf_pobs(po, p->stream));
    } else {
        KERNEL(spdy::launch_letkf_obs(o, p->stream));
    }
    if (!l->d_tw) {
        KERNEL(spdy::launch_letkf_transform(c, l->lds, p->stream));
        return SPDY_OK;
    }
    // weight interpolation: T of the coarse columns, then the increments of every column from them
    c.nlist = (int)l->h_coarse.size(); c.cols = l->d_coarse; c.tw = l->d_tw;
    spdy::LetkfApply ap{};
    ap.nmem = l->nmem; ap.kx = kx; ap.ncol = ncol; ap.nlist = c.nlist;
    ap.iidx = l->d_iidx; ap.iwgt = l->d_iwgt; ap.tw = l->d_tw;
    for (int v = 0; v < spdy::LETKF_VARS; ++v) { ap.x[v] = x[v]; ap.dx[v] = dx[v]; }
    KERNEL(spdy::launch_letkf_transform(c, l->lds, p->stream));
    KERNEL(spdy::launch_letkf_apply(ap, p->stream));
    return SPDY_OK;
}

// the coarse columns of a stride and every grid column's stencil in them (include/spdy.h, "ensemble analysis": weight interpolation)
void interp_tables(int ix, int il, int si, int sj, std::vector<int> &coarse, std::vector<int> &idx, std::vector<double> &wgt)
{
    std::vector<int> rows;                    // the coarse rows, ascending: 0, sj, 2 sj, ... and il - 1
    for (int j = 0; j < il - 1; j += sj) rows.push_back(j);
    rows.push_back(il - 1);
    const int ni = ix / si;
    coarse.clear();
    for (int j : rows)
        for (int i = 0; i < ix; i += si) coarse.push_back(j * ix + i);
    idx.assign((size_t)4 * ix * il, 0);
    wgt.assign((size_t)4 * ix * il, 0.0);
    size_t r0 = 0;                            // rows[r0] is the largest coarse row <= j
    for (int j = 0; j < il; ++j) {
        while (r0 + 1 < rows.size() && rows[r0 + 1] <= j) ++r0;
        const size_t r1 = j == il - 1 ? r0 : r0 + 1;
        const int j0 = rows[r0], j1 = rows[r1];
        const double b = j1 == j0 ? 0.0 : (double)(j - j0) / (double)(j1 - j0);
        for (int i = 0; i < ix; ++i) {
            const int c0 = i / si, c1 = (c0 + 1) % ni;
            const double a = (double)(i - c0 * si) / (double)si;
            const int e[4] = {(int)r0 * ni + c0, (int)r0 * ni + c1, (int)r1 * ni + c0, (int)r1 * ni + c1};
            const double w[4] = {(1.0 - a) * (1.0 - b), a * (1.0 - b), (1.0 - a) * b, a * b};
            const size_t at = 4 * ((size_t)j * ix + i);
            int first = -1;
            for (int n = 0; n < 4 && first < 0; ++n)
                if (w[n] != 0.0) first = e[n];
            for (int n = 0; n < 4; ++n) {
                wgt[at + n] = w[n];
                idx[at + n] = w[n] != 0.0 ? e[n] : first;      // an entry that is not read repeats the first one that is
            }
        }
    }
}

void drop_interp(spdy_letkf *l)
{
    (void)dev_release(l->plan, l->d_wbase);
    l->d_wbase = l->d_tw = l->d_iwgt = nullptr;
    l->d_iidx = l->d_coarse = nullptr;
    l->si = l->sj = 1;
    l->h_coarse.clear(); l->h_iidx.clear(); l->h_iwgt.clear();
}

// an observation of either entry point as the ingestion reads it
inline double pressure_of(const spdy_obs &) { return 0.0; }
inline double pressure_of(const spdy_pobs &b) { return b.p; }
constexpr bool takes_pressure(const spdy_obs *) { return false; }
constexpr bool takes_pressure(const spdy_pobs *) { return true; }

// spdy_letkf_set_obs and spdy_pobs_set: every field of every observation is validated before anything changes; then the tables
// are built on the host and uploaded.  OBS = spdy_obs: no observation is at a pressure, and the object is left as it always was.
template <class OBS>
int ingest(spdy_letkf *l, int nobs, const OBS *host, const char *call, const char *what)
{
    NEED_LIVE(l, "analysis object");
    if (nobs < 0 || nobs > l->max_obs) return fail(SPDY_ERR_ARG, "%s: nobs=%d outside [0, max_obs=%d]", call, nobs, l->max_obs);
    if (nobs && !host) return fail(SPDY_ERR_ARG, "null observations");
    spdy_plan *p = l->plan;
    const int kx = p->tab.kx;
    constexpr bool PRES = takes_pressure(static_cast<const OBS *>(nullptr));
    auto at_p = [&](const OBS &b) { return PRES && b.var != SPDY_OBS_PS && b.lev == SPDY_OBS_AT_P; };
    for (int o = 0; o < nobs; ++o) {
        const OBS &b = host[o];
        if (b.var < SPDY_OBS_U || b.var > SPDY_OBS_PS) return fail(SPDY_ERR_ARG, "%s: observation %d: var=%d", call, o, b.var);
        if (at_p(b)) {
            if (kx < 2) return fail(SPDY_ERR_ARG, "%s: observation %d: an observation at a pressure needs kx >= 2", call, o);
            const double pr = pressure_of(b);
            if (!(pr > 0.0) || !std::isfinite(pr)) return fail(SPDY_ERR_ARG, "%s: observation %d: p must be finite and > 0", call, o);
        } else if (b.var != SPDY_OBS_PS && (b.lev < 0 || b.lev >= kx))
            return fail(SPDY_ERR_ARG, "%s: observation %d: lev=%d outside [0, %d)", call, o, b.lev, kx);
        if (!std::isfinite(b.lon)) return fail(SPDY_ERR_ARG, "%s: observation %d: lon is not finite", call, o);
        if (!(std::fabs(b.lat) <= 90.0)) return fail(SPDY_ERR_ARG, "%s: observation %d: lat outside [-90, 90]", call, o);
        if (!std::isfinite(b.value)) return fail(SPDY_ERR_ARG, "%s: observation %d: value is not finite", call, o);
        if (!(b.error > 0.0) || !std::isfinite(b.error))
            return fail(SPDY_ERR_ARG, "%s: observation %d: error must be finite and > 0", call, o);
    }
    NOT_CAPTURING(p, what);
    const size_t n = (size_t)nobs;
    const double p0 = static_cast<double>(1.e+5f);
    std::vector<int> sidx(4 * n), var(n), lev(n), atp(PRES ? n : 0);
    std::vector<double> swgt(4 * n), unit(3 * n), lns(n), rinv(n), err(n), value(n), lnp(PRES ? n : 0);
    // obs_used is all ones from create on; only an analysis of a network with at-pressure observations writes anything else
    const bool reset_used = p->device >= 0 && (PRES || l->npobs > 0);
    std::vector<double> ones(reset_used ? n : 0, 1.0);
    int npobs = 0;
    for (size_t o = 0; o < n; ++o) {
        const OBS &b = host[o];
        stencil(l, b.lon, b.lat, &sidx[4 * o], &swgt[4 * o]);
        unit_vector(b.lon, b.lat, &unit[3 * o]);
        var[o] = b.var;
        if (at_p(b)) {
            lev[o] = 0;                                   // the device's level stays a level: atp marks the observation
            atp[o] = 1;
            lnp[o] = lns[o] = std::log(pressure_of(b) / p0);      // ln sigma_o at ps = 0; the analysis call forms its own
            ++npobs;
        } else {
            lev[o] = b.var == SPDY_OBS_PS ? 0 : b.lev;
            lns[o] = b.var == SPDY_OBS_PS ? 0.0 : l->lnfsg[b.lev];
        }
        rinv[o] = 1.0 / (b.error * b.error);
        err[o] = b.error;
        value[o] = b.value;
    }
    if (p->device >= 0) {
        HIP_TRY(hipSetDevice(p->device));
        auto all = [&]() -> int {
            RC(upload(p, l->d_sidx, sidx.data(), 4 * n * sizeof(int)));
            RC(upload(p, l->d_var, var.data(), n * sizeof(int)));
            RC(upload(p, l->d_lev, lev.data(), n * sizeof(int)));
            RC(upload(p, l->d_swgt, swgt.data(), 4 * n * sizeof(double)));
            RC(upload(p, l->d_ounit, unit.data(), 3 * n * sizeof(double)));
            RC(upload(p, l->d_olns, lns.data(), n * sizeof(double)));
            RC(upload(p, l->d_rinv, rinv.data(), n * sizeof(double)));
            RC(upload(p, l->d_err, err.data(), n * sizeof(double)));
            RC(upload(p, l->d_value, value.data(), n * sizeof(double)));
            if (reset_used) { RC(upload(p, l->d_used, ones.data(), n * sizeof(double))); }
            if (PRES) {
                RC(upload(p, l->d_lnp, lnp.data(), n * sizeof(double)));
                RC(upload(p, l->d_atp, atp.data(), n * sizeof(int)));
            }
            HIP_TRY(hipStreamSynchronize(p->stream));
            return SPDY_OK;
        };
        if (const int rc = all()) {
            // the device tables may be partly new: the object holds no observations now, and no copy is still reading the host
            // arrays when they go
            (void)hipStreamSynchronize(p->stream);
            l->nobs = 0; l->npobs = 0;
            l->h_sidx.clear(); l->h_swgt.clear(); l->h_unit.clear(); l->h_lns.clear(); l->h_rinv.clear(); l->h_lnp.clear();
            return rc;
        }
    }
    l->nobs = nobs; l->npobs = npobs;
    l->h_sidx.swap(sidx); l->h_swgt.swap(swgt); l->h_unit.swap(unit); l->h_lns.swap(lns); l->h_rinv.swap(rinv); l->h_lnp.swap(lnp);
    return SPDY_OK;
}
}  // namespace

extern "C" {

int spdy_letkf_create(spdy_plan *p, int nmem, int max_obs, spdy_letkf **out)
{
    NEED_PLAN(p);
    if (nmem < 2 || nmem > spdy::LETKF_MAX_MEMBERS)
        return fail(SPDY_ERR_ARG, "letkf_create: nmem=%d outside [2, %d]", nmem, spdy::LETKF_MAX_MEMBERS);
    if (max_obs < 0) return fail(SPDY_ERR_ARG, "letkf_create: max_obs=%d < 0", max_obs);
    if (!out) return fail(SPDY_ERR_ARG, "null result pointer");
    const spdy::HostTables &t = p->tab;
    const int kx = t.kx, il = t.il, ix = t.ix;
    const long need = (long)nmem * (2 * kx + 1);
    if (p->max_batch < need)
        return fail(SPDY_ERR_ARG, "letkf_create: max_batch=%d must be >= nmem*(2*kx+1)=%ld", p->max_batch, need);
    int nlv = 4;
    while (nlv > 1 && spdy::letkf_lds_bytes(nmem, kx, nlv) > kLdsLimit) nlv /= 2;
    if (spdy::letkf_lds_bytes(nmem, kx, nlv) > kLdsLimit)
        return fail(SPDY_ERR_ARG, "letkf_create: nmem=%d at kx=%d needs %zu bytes of LDS, a compute unit has %zu", nmem, kx,
                    spdy::letkf_lds_bytes(nmem, kx, nlv), kLdsLimit);
    if (!t.sigma_ready) return fail(SPDY_ERR_STATE, "letkf_create needs sigma levels");
    NOT_CAPTURING(p, "spdy_letkf_create (allocation + upload)");
    spdy_letkf *l = new spdy_letkf;
    adopt(p, l);
    l->nmem = nmem; l->max_obs = max_obs; l->nlv = nlv; l->lds = spdy::letkf_lds_bytes(nmem, kx, nlv);
    // geometry.f90:70-75: sia(j) = -sia_half(j), sia(il+1-j) = sia_half(j), radang = asin(sia); in degrees, south first
    l->lat.resize(il);
    for (int j = 0; j < il; ++j) {
        const int h = j < t.iy ? j : il - 1 - j;
        l->lat[j] = (j < t.iy ? -std::asin(t.sia_half[h]) : std::asin(t.sia_half[h])) * (180.0 / kPi);
    }
    l->lnfsg.resize(kx);
    for (int k = 0; k < kx; ++k) l->lnfsg[k] = std::log(t.fsg[k]);
    *out = l;
    if (p->device < 0) return SPDY_OK;
    auto cleanup = [&](int rc) { spdy_letkf_destroy(l); *out = nullptr; return rc; };
    if (hipSetDevice(p->device) != hipSuccess) return cleanup(fail(SPDY_ERR_HIP, "hipSetDevice failed"));
    const size_t ncol = grid_elems(p), nf = (size_t)(4 * kx + 1) * nmem, M = (size_t)(max_obs > 0 ? max_obs : 1), E = (size_t)nmem;
    // doubles: grids | spectra | colunit | lnfsg | swgt | ounit | olns | rinv | err | value | hx | hxmean | y | dep | lnp | used |
    // reff ; then the ints
    const size_t nd = nf * ncol + nf * spec_elems(p) + 3 * ncol + (size_t)kx + M * (4 + 3 + 1 + 1 + 1 + 1 + 1 + 1 + 2 * E + 3), ni = 7 * M;
    if (int rc = dev_alloc(p, nd * sizeof(double) + ni * sizeof(int), &l->d_base)) return cleanup(rc);
    double *d = l->d_base;
    l->d_grid = d; d += nf * ncol;
    l->d_spec = d; d += nf * spec_elems(p);
    l->d_colunit = d; d += 3 * ncol;
    l->d_lnfsg = d; d += kx;
    l->d_swgt = d; d += 4 * M;
    l->d_ounit = d; d += 3 * M;
    l->d_olns = d; d += M;
    l->d_rinv = d; d += M;
    l->d_err = d; d += M;
    l->d_value = d; d += M;
    l->d_hx = d; d += M * E;
    l->d_hxmean = d; d += M;
    l->d_y = d; d += M * E;
    l->d_dep = d; d += M;
    l->d_lnp = d; d += M;
    l->d_used = d; d += M;
    l->d_reff = d; d += M;
    int *q = reinterpret_cast<int *>(d);
    l->d_sidx = q; q += 4 * M;
    l->d_var = q; q += M;
    l->d_lev = q; q += M;
    l->d_atp = q;
    std::vector<double> cu(3 * ncol);
    for (int j = 0; j < il; ++j)
        for (int i = 0; i < ix; ++i) {
            double u[3];
            unit_vector(i * (360.0 / ix), l->lat[j], u);
            for (int c = 0; c < 3; ++c) cu[c * ncol + (size_t)j * ix + i] = u[c];
        }
    const std::vector<double> ones(M, 1.0);   // obs_used: spdy_letkf_set_obs never has to write it
    if (hipMemsetAsync(l->d_base, 0, nd * sizeof(double) + ni * sizeof(int), p->stream) != hipSuccess ||
        hipMemcpyAsync(l->d_used, ones.data(), M * sizeof(double), hipMemcpyHostToDevice, p->stream) != hipSuccess ||
        hipMemcpyAsync(l->d_colunit, cu.data(), cu.size() * sizeof(double), hipMemcpyHostToDevice, p->stream) != hipSuccess ||
        hipMemcpyAsync(l->d_lnfsg, l->lnfsg.data(), kx * sizeof(double), hipMemcpyHostToDevice, p->stream) != hipSuccess ||
        hipStreamSynchronize(p->stream) != hipSuccess)
        return cleanup(fail(SPDY_ERR_HIP, "letkf_create: upload failed"));
    if (spdy::letkf_prepare(l->lds) != hipSuccess) return cleanup(fail(SPDY_ERR_HIP, "letkf_create: %zu bytes of LDS refused", l->lds));
    // one inverse and one direct batch of the zero workspace, in the shapes spdy_ens_letkf_dev uses: whatever the plan's two
    // transform paths allocate on their first call of this size exists before a capture
    const int nk = nmem * kx;
    const size_t L = (size_t)nk * ncol, LS = (size_t)nk * spec_elems(p);
    double *g = l->d_grid, *s = l->d_spec;
    int rc = ensure_four(p);
    const spdy_spec_seg segs[3] = {{nk, s + 2 * LS}, {nk, s + 3 * LS}, {nmem, s + 4 * LS}};
    if (!rc) rc = spdy_inverse_batch_segs_dev(p, nk, s, s + LS, g, g + L, 2, 3, segs, nullptr, 1, g + 2 * L, 0, nullptr, nullptr, nullptr, 2);
    if (!rc) rc = spdy_direct_batch_dev(p, nk, g, g + L, s, s + LS, 2, 2 * nk + nmem, g + 2 * L, s + 2 * LS);
    if (!rc && hipStreamSynchronize(p->stream) != hipSuccess) rc = fail(SPDY_ERR_HIP, "letkf_create: the first transforms failed");
    return rc ? cleanup(rc) : SPDY_OK;
}

int spdy_letkf_destroy(spdy_letkf *l)
{
    if (!l) return SPDY_OK;
    retire(l, {l->d_wbase, l->d_base});
    delete l;
    return SPDY_OK;
}

int spdy_letkf_set_localization(spdy_letkf *l, double sigma_h, double sigma_v, double rho)
{
    NEED_LIVE(l, "analysis object");
    if (!(sigma_h > 0.0) || !std::isfinite(sigma_h)) return fail(SPDY_ERR_ARG, "letkf: sigma_h must be finite and > 0");
    if (!std::isfinite(sigma_v)) return fail(SPDY_ERR_ARG, "letkf: sigma_v must be finite (<= 0: no vertical localisation)");
    if (!(rho > 0.0) || !std::isfinite(rho)) return fail(SPDY_ERR_ARG, "letkf: rho must be finite and > 0");
    l->sigma_h = sigma_h; l->sigma_v = sigma_v; l->rho = rho; l->loc_set = true;
    return SPDY_OK;
}

int spdy_letkf_set_obs(spdy_letkf *l, int nobs, const spdy_obs *host)
{
    return ingest(l, nobs, host, "letkf_set_obs", "spdy_letkf_set_obs (upload)");
}

int spdy_pobs_set(spdy_letkf *l, int nobs, const spdy_pobs *host)
{
    return ingest(l, nobs, host, "pobs_set", "spdy_pobs_set (upload)");
}

int spdy_letkf_set_weight_stride(spdy_letkf *l, int si, int sj)
{
    NEED_LIVE(l, "analysis object");
    spdy_plan *p = l->plan;
    const int ix = p->tab.ix, il = p->tab.il, kx = p->tab.kx;
    if (si < 1 || si > ix / 2 || ix % si) return fail(SPDY_ERR_ARG, "letkf_set_weight_stride: si=%d must divide ix=%d and lie in [1, %d]", si, ix, ix / 2);
    if (sj < 1 || sj > il - 1) return fail(SPDY_ERR_ARG, "letkf_set_weight_stride: sj=%d outside [1, %d]", sj, il - 1);
    NOT_CAPTURING(p, "spdy_letkf_set_weight_stride (allocation + upload)");
    drop_interp(l);
    if (si == 1 && sj == 1) return SPDY_OK;
    std::vector<int> coarse, idx;
    std::vector<double> wgt;
    interp_tables(ix, il, si, sj, coarse, idx, wgt);
    if (p->device >= 0) {
        HIP_TRY(hipSetDevice(p->device));
        const size_t nc = coarse.size(), ncol = grid_elems(p), ntw = nc * kx * l->nmem * l->nmem;
        const size_t bytes = (ntw + 4 * ncol) * sizeof(double) + (4 * ncol + nc) * sizeof(int);
        RC(dev_alloc(p, bytes, &l->d_wbase));
        l->d_tw = l->d_wbase;
        l->d_iwgt = l->d_tw + ntw;
        l->d_iidx = reinterpret_cast<int *>(l->d_iwgt + 4 * ncol);
        l->d_coarse = l->d_iidx + 4 * ncol;
        auto all = [&]() -> int {
            HIP_TRY(hipMemsetAsync(l->d_tw, 0, ntw * sizeof(double), p->stream));
            RC(upload(p, l->d_iwgt, wgt.data(), 4 * ncol * sizeof(double)));
            RC(upload(p, l->d_iidx, idx.data(), 4 * ncol * sizeof(int)));
            RC(upload(p, l->d_coarse, coarse.data(), nc * sizeof(int)));
            HIP_TRY(hipStreamSynchronize(p->stream));
            return SPDY_OK;
        };
        if (const int rc = all()) {
            drop_interp(l);                   // back at stride (1, 1); no copy is still reading the host arrays when they go
            return rc;
        }
    }
    l->si = si; l->sj = sj;
    l->h_coarse.swap(coarse); l->h_iidx.swap(idx); l->h_iwgt.swap(wgt);
    return SPDY_OK;
}

int spdy_letkf_table(const spdy_letkf *l, const char *name, double *buf, int cap)
{
    NEED_LIVE(l, "analysis object");
    if (!name) return fail(SPDY_ERR_ARG, "null table name");
    const std::vector<int> *index = !std::strcmp(name, "stencil_index") ? &l->h_sidx : !std::strcmp(name, "coarse_columns") ? &l->h_coarse
                                    : !std::strcmp(name, "interp_index") ? &l->h_iidx : nullptr;
    const std::vector<double> *v = !std::strcmp(name, "stencil_weight") ? &l->h_swgt : !std::strcmp(name, "unit") ? &l->h_unit
                                   : !std::strcmp(name, "lnsigma") ? &l->h_lns : !std::strcmp(name, "rinv") ? &l->h_rinv
                                   : !std::strcmp(name, "interp_weight") ? &l->h_iwgt : !std::strcmp(name, "lnp") ? &l->h_lnp : nullptr;
    if (!index && !v) return fail(SPDY_ERR_ARG, "unknown analysis table '%s'", name);
    const int n = static_cast<int>(index ? index->size() : v->size());
    if (buf && cap < n) return fail(SPDY_ERR_ARG, "analysis table '%s' has %d values, the buffer %d", name, n, cap);
    if (buf && index)
        for (int i = 0; i < n; ++i) buf[i] = (*index)[i];
    else if (buf && n)
        std::memcpy(buf, v->data(), sizeof(double) * (size_t)n);
    return n;
}

int spdy_letkf_field(spdy_letkf *l, const char *name, double **d_ptr)
{
    NEED_LIVE(l, "analysis object");
    if (!name || !d_ptr) return fail(SPDY_ERR_ARG, "null name or result pointer");
    double *const *f = !std::strcmp(name, "hx") ? &l->d_hx : !std::strcmp(name, "hxmean") ? &l->d_hxmean
                       : !std::strcmp(name, "y") ? &l->d_y : !std::strcmp(name, "departure") ? &l->d_dep
                       : !std::strcmp(name, "weights") ? &l->d_tw : !std::strcmp(name, "value") ? &l->d_value
                       : !std::strcmp(name, "grid") ? &l->d_grid : !std::strcmp(name, "obs_lnsigma") ? &l->d_olns
                       : !std::strcmp(name, "obs_used") ? &l->d_used : nullptr;
    if (!f) return fail(SPDY_ERR_ARG, "unknown analysis field '%s'", name);
    if (f == &l->d_tw && l->si == 1 && l->sj == 1) return fail(SPDY_ERR_STATE, "letkf: no weight buffer at stride (1, 1)");
    NEED_DEVICE(l->plan);
    *d_ptr = *f;
    return SPDY_OK;
}

int spdy_letkf_analyse_grid_dev(spdy_letkf *l, const double *ug, const double *vg, const double *tg, const double *qg, const double *psg,
                                double *du, double *dv, double *dt, double *dq, double *dps)
{
    RC(analysis_ready(l, ug && vg && tg && qg && psg && du && dv && dt && dq && dps));
    const double *x[spdy::LETKF_VARS] = {ug, vg, tg, qg, psg};
    double *dx[spdy::LETKF_VARS] = {du, dv, dt, dq, dps};
    return analyse_grid(l, x, dx);
}

int spdy_ens_letkf_dev(spdy_letkf *l, double *vor, double *div, double *t, double *q, double *ps)
{
    RC(analysis_ready(l, vor && div && t && q && ps));
    spdy_plan *p = l->plan;
    const int kx = p->tab.kx, nmem = l->nmem, nk = nmem * kx;
    const size_t L = (size_t)nk * grid_elems(p), LS = (size_t)nk * spec_elems(p);
    double *g = l->d_grid, *s = l->d_spec;
    // time level 1 of all members to the grid, read in place: nmem*kx pairs (true wind), the segments t | q | ps
    const spdy_spec_seg segs[3] = {{nk, t}, {nk, q}, {nmem, ps}};
    RC(spdy_inverse_batch_segs_dev(p, nk, vor, div, g, g + L, 2, 3, segs, nullptr, 1, g + 2 * L, 0, nullptr, nullptr, nullptr, 2));
    // the increments take the place of the gridded ensemble
    double *x[spdy::LETKF_VARS] = {g, g + L, g + 2 * L, g + 3 * L, g + 4 * L};
    RC(analyse_grid(l, x, x));
    // vdspec(du, dv, 2) next to grid_to_spec(dt | dq | dps), then into the prognostics
    RC(spdy_direct_batch_dev(p, nk, g, g + L, s, s + LS, 2, 2 * nk + nmem, g + 2 * L, s + 2 * LS));
    spdy::LetkfAdd a{};
    a.nops = spdy::LETKF_VARS;
    double *dst[spdy::LETKF_VARS] = {vor, div, t, q, ps};
    for (int v = 0; v < spdy::LETKF_VARS; ++v) {
        a.dst[v] = dst[v]; a.src[v] = s + (size_t)v * LS;
        a.n[v] = (long)(v < 4 ? LS : (size_t)nmem * spec_elems(p));
    }
    KERNEL(spdy::launch_spec_add(a, p->stream));
    return SPDY_OK;
}

}  // extern "C"
