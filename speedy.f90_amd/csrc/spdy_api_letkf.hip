// C ABI of the ensemble analysis (include/spdy.h, "ensemble analysis"): the observation ingestion on the host, the
// analysis of a gridded ensemble, the five-launch analysis of an ensemble's spectral state, and the tables and the buffer of weight
// interpolation (one launch more), and observations in time slots: the ranges on the host, the observe calls and the
// two analysis calls that finish what the slots kept.  Kernels: csrc/spdy_letkf.hip.
#include <algorithm>
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

// An optional allocation of an object's, made once: carved by `arrays` (one of the object's *_arrays visitors with its sizes; base:
// the first array), zeroed, so that no call ever reads what it did not write, then the caller's uploads and one synchronisation.
// On any failure: synchronise -- no copy still reads a host array when the caller's go out of scope --, release, forget the
// pointers, the code: nothing is left.  The caller has checked that no capture is open
template <class T, class ARRAYS, class UPLOADS>
int optional_block(spdy_plan *p, T *&base, ARRAYS &&arrays, UPLOADS &&uploads)
{
    size_t bytes = 0;
    auto all = [&]() -> int {
        RC(dev_carve(p, arrays, &bytes));
        HIP_TRY(hipMemsetAsync(base, 0, bytes, p->stream));
        RC(uploads());
        HIP_TRY(hipStreamSynchronize(p->stream));
        return SPDY_OK;
    };
    const int rc = all();
    if (rc) {
        (void)hipStreamSynchronize(p->stream);
        (void)dev_release(p, base);
        arrays(Carve{});
    }
    return rc;
}
const auto no_uploads = []() -> int { return SPDY_OK; };

// the object's grid workspace as the five fields of a gridded ensemble: u | v | t | q (nmem kx grids each, member-major) | ps
void grid_workspace(spdy_letkf *l, double **x)
{
    const size_t L = (size_t)l->nmem * l->plan->tab.kx * grid_elems(l->plan);
    for (int v = 0; v < spdy::LETKF_VARS; ++v) x[v] = l->d_grid + (size_t)v * L;
}

// d_use: NULL, or the member mask -- one launch in front, which builds the table the masked forms of the kernels read (*umap: that
// table, or NULL); the object remembers which kind of call was enqueued last
int mask_table(spdy_letkf *l, const int *d_use, const int **umap)
{
    if (d_use) KERNEL(spdy::launch_letkf_mask(d_use, l->nmem, l->d_umap, l->d_nused + 1, l->plan->stream));
    l->masked_last = d_use != nullptr;
    *umap = d_use ? l->d_umap : nullptr;
    return SPDY_OK;
}

// the argument checks the analysis calls share, in the documented order; slots: a slot analysis, which needs before the device
// every non-empty slot observed since the latest spdy_slot_set; the device last
int analysis_ready(spdy_letkf *l, bool ptrs_ok, bool slots)
{
    NEED_LIVE(l, "analysis object");
    if (!l->loc_set) return fail(SPDY_ERR_STATE, "letkf: spdy_letkf_set_localization first");
    if (!ptrs_ok) return fail(SPDY_ERR_ARG, "null device pointer");
    if (slots) {
        if (!l->nslots) return fail(SPDY_ERR_STATE, "slot analysis: spdy_slot_set first");
        for (int s = 0; s < l->nslots; ++s)
            if (l->slot_first[s + 1] > l->slot_first[s] && !l->slot_observed[s])
                return fail(SPDY_ERR_STATE, "slot analysis: slot %d has not been observed since spdy_slot_set", s);
    }
    NEED_DEVICE(l->plan);
    return SPDY_OK;
}

// the two observe calls' checks in the documented order, the device last
int observe_ready(spdy_letkf *l, int slot, bool ptrs_ok)
{
    NEED_LIVE(l, "analysis object");
    if (!l->nslots) return fail(SPDY_ERR_STATE, "slot_observe: spdy_slot_set first");
    if (slot < 0 || slot >= l->nslots) return fail(SPDY_ERR_ARG, "slot_observe: slot=%d outside [0, nslots=%d)", slot, l->nslots);
    if (!ptrs_ok) return fail(SPDY_ERR_ARG, "null device pointer");
    NEED_DEVICE(l->plan);
    return SPDY_OK;
}

// the observation stage's argument for the observations [first, last) of l's network on the gridded ensemble x: the tables, the
// outputs and, for a network that holds an observation at a pressure, the pressure part
spdy::LetkfObserve observe_args(spdy_letkf *l, const double *const *x, int first, int last)
{
    spdy_plan *p = l->plan;
    spdy::LetkfObserve o{};
    o.first = first; o.last = last; o.nmem = l->nmem; o.kx = p->tab.kx; o.ncol = (int)grid_elems(p);
    o.var = l->d_var; o.lev = l->d_lev; o.sidx = l->d_sidx; o.swgt = l->d_swgt; o.value = l->d_value;
    for (int v = 0; v < spdy::LETKF_VARS; ++v) o.x[v] = x[v];
    o.hx = l->d_hx; o.hxmean = l->d_hxmean; o.y = l->d_y; o.dep = l->d_dep;
    if (l->npobs) {
        o.atp = l->d_atp; o.lnp = l->d_lnp; o.rinv = l->d_rinv; o.olns = l->d_olns; o.used = l->d_used; o.reff = l->d_reff;
        o.slot_ps = l->d_slot_ps; o.slot_out = l->d_slot_out; o.lv = l->lv;
    }
    return o;
}

// the slot kernel on a gridded ensemble: ONE launch, none for an empty slot; the slot is marked observed
int observe_grid(spdy_letkf *l, int slot, const double *const *x)
{
    KERNEL(spdy::launch_letkf_slot_obs(observe_args(l, x, l->slot_first[slot], l->slot_first[slot + 1]), l->plan->stream));
    l->slot_observed[slot] = true;
    return SPDY_OK;
}

// the check's launch on what the observation stage has just written (include/spdy.h, "background check and observation
// statistics"): decide -- an analysis call; otherwise the stats-only call.  The row of the statistics is that of `slot`
int check_obs(spdy_letkf *l, const int *umap, bool decide, int slot)
{
    if (!l->d_qc_stats) return fail(SPDY_ERR_STATE, "letkf: the background check is on without its block");
    spdy::LetkfQc q{};
    q.nobs = l->nobs; q.nmem = l->nmem; q.ngroups = l->qc_ngroups; q.g2 = l->gross * l->gross;
    q.group = l->qc_group.empty() ? nullptr : l->d_qc_group; q.var = l->d_var;
    q.y = l->d_y; q.dep = l->d_dep; q.err = l->d_err; q.rinv = l->d_rinv;
    q.incol = l->npobs ? l->d_used : nullptr;
    q.used = l->d_used; q.reff = l->d_reff; q.check = l->d_qc_check; q.depb = l->d_qc_depb;
    q.stats = l->d_qc_stats + (size_t)slot * SPDY_QC_MAX_GROUPS * spdy::QC_STATS;
    q.umap = umap;
    KERNEL(spdy::launch_letkf_qc(q, decide, l->plan->stream));
    return SPDY_OK;
}

// d_use: mask_table's.  slots: the finish kernel of "observations in time slots" in the observation kernel's place, everything else as it is.
// The observation stage's argument is filled once (observe_args); one branch: observe now, or finish what the slots kept
int analyse_grid(spdy_letkf *l, const double *const *x, double *const *dx, const int *d_use = nullptr, bool slots = false)
{
    spdy_plan *p = l->plan;
    const int *umap = nullptr;
    RC(mask_table(l, d_use, &umap));
    const int kx = p->tab.kx, ncol = (int)grid_elems(p);
    spdy::LetkfObserve o = observe_args(l, x, 0, l->nobs);
    o.umap = umap;
    spdy::LetkfCols c{};
    c.nobs = l->nobs; c.nmem = l->nmem; c.kx = kx; c.ncol = ncol; c.nlv = l->nlv;
    c.ch = l->sigma_h * std::sqrt(10.0 / 3.0); c.cv = l->sigma_v > 0.0 ? l->sigma_v * std::sqrt(10.0 / 3.0) : 0.0;
    c.diag = (double)(l->nmem - 1) / l->rho;
    c.colunit = l->d_colunit; c.lnfsg = l->d_lnfsg; c.ounit = l->d_ounit; c.olns = l->d_olns; c.rinv = l->d_rinv;
    c.y = l->d_y; c.dep = l->d_dep;
    // relaxation: the transform or apply kernel writes the raw increments into the object's workspace, one launch more relaxes
    // them into dx (which may be x).  Both values 0: dx is written as always and nothing more is enqueued.
    const bool relaxed = l->rtpp != 0.0 || l->rtps != 0.0;
    if (relaxed && !l->d_raw) return fail(SPDY_ERR_STATE, "letkf: relaxation is on without its workspace");
    double *raw[spdy::LETKF_VARS];
    for (int v = 0; v < spdy::LETKF_VARS; ++v) raw[v] = relaxed ? l->d_raw + (size_t)v * l->nmem * kx * ncol : dx[v];
    auto relax = [&]() -> int {
        if (!relaxed) return SPDY_OK;
        spdy::LetkfRelax r{};
        r.nmem = l->nmem; r.kx = kx; r.ncol = ncol; r.omr = 1.0 - l->rtpp; r.rtps = l->rtps;
        r.inflation = l->d_infl; r.umap = umap;
        for (int v = 0; v < spdy::LETKF_VARS; ++v) { r.x[v] = x[v]; r.raw[v] = raw[v]; r.dx[v] = dx[v]; }
        KERNEL(spdy::launch_letkf_relax(r, p->stream));
        return SPDY_OK;
    };
    for (int v = 0; v < spdy::LETKF_VARS; ++v) { c.x[v] = x[v]; c.dx[v] = raw[v]; }
    // A network that holds an observation at a pressure: the observation stage writes ln sigma_o of those observations into olns and
    // this call's copy of rinv, 0 where an observation is out of its column.  slots: hx (and the stencils' ps and out-of-column
    // flags) are the slots', and only what couples members is formed here.
    if (l->npobs) c.rinv = l->d_reff;
    if (slots) {
        KERNEL(spdy::launch_letkf_slot_finish(o, p->stream));
    } else {
        KERNEL(spdy::launch_letkf_observe(o, p->stream));
    }
    // the background check: one launch more, and the transform reads the per-call 1 / error^2 whatever the network's kind
    if (l->qc_on()) {
        RC(check_obs(l, umap, true, l->qc_slot));
        c.rinv = l->d_reff;
        l->qc_analysed = true;
    }
    // adaptive inflation: the transform reads the field as it is before this call; the estimate's two launches come last and
    // write it in place for the next call (include/spdy.h, "adaptive inflation")
    const bool adaptive = l->infl_on;
    if (adaptive && !l->d_rho) return fail(SPDY_ERR_STATE, "letkf: adaptive inflation is on without its block");
    auto transform = [&]() -> int {
        KERNEL(spdy::launch_letkf_transform(c, l->rho, adaptive ? l->d_rho : nullptr, umap, l->lds, p->stream));
        return SPDY_OK;
    };
    auto finish = [&]() -> int {
        RC(relax());
        if (!adaptive) return SPDY_OK;
        spdy::LetkfInfl e{};
        e.nobs = l->nobs; e.nmem = l->nmem; e.kx = kx; e.ncol = ncol; e.ch = c.ch; e.cv = c.cv;
        e.vb = l->infl_sigma_b * l->infl_sigma_b; e.rho_min = l->infl_min; e.rho_max = l->infl_max;
        e.colunit = c.colunit; e.lnfsg = c.lnfsg; e.ounit = c.ounit; e.olns = c.olns; e.reff = c.rinv; e.y = c.y; e.dep = c.dep;
        e.s2 = l->d_obs_s2; e.rho = l->d_rho; e.parm = l->d_infl_parm; e.umap = umap;
        KERNEL(spdy::launch_letkf_infl(e, p->stream));
        return SPDY_OK;
    };
    if (!l->d_tw) {
        RC(transform());
        return finish();
    }
    // weight interpolation: T of the coarse columns, then the increments of every column from them
    c.nlist = (int)l->interp.coarse.size(); c.cols = l->d_coarse; c.tw = l->d_tw;
    spdy::LetkfApply ap{};
    ap.nmem = l->nmem; ap.kx = kx; ap.ncol = ncol; ap.nlist = c.nlist;
    ap.iidx = l->d_iidx; ap.iwgt = l->d_iwgt; ap.tw = l->d_tw;
    for (int v = 0; v < spdy::LETKF_VARS; ++v) { ap.x[v] = x[v]; ap.dx[v] = raw[v]; }
    RC(transform());
    KERNEL(spdy::launch_letkf_apply(ap, p->stream, umap));
    return finish();
}

// the block of adaptive inflation of a device plan's object, made once: the field filled with the object's scalar rho, the sums
// and s2 zero
int infl_block(spdy_letkf *l)
{
    if (l->d_rho) return SPDY_OK;
    spdy_plan *p = l->plan;
    const size_t n = (size_t)p->tab.kx * grid_elems(p);
    const std::vector<double> fill(n, l->rho);
    return optional_block(p, l->d_rho, [&](auto &&v) { l->infl_arrays(v, grid_elems(p), (size_t)p->tab.kx, (size_t)(l->max_obs > 0 ? l->max_obs : 1)); },
                          [&]() -> int { return upload(p, l->d_rho, fill.data(), n * sizeof(double)); });
}

// the qc block of a device plan's object, made once: the statistics, the record, the kept departure and the grouping
int qc_block(spdy_letkf *l)
{
    if (l->d_qc_stats) return SPDY_OK;
    return optional_block(l->plan, l->d_qc_stats, [&](auto &&v) { l->qc_arrays(v, (size_t)(l->max_obs > 0 ? l->max_obs : 1)); }, no_uploads);
}

// the stats-only calls' checks in the documented order, the device last
int stats_ready(spdy_letkf *l, bool ptrs_ok, int slot)
{
    NEED_LIVE(l, "analysis object");
    if (!l->qc_on()) return fail(SPDY_ERR_STATE, "qc_stats: spdy_qc_set first");
    if (!l->qc_analysed) return fail(SPDY_ERR_STATE, "qc_stats: no analysis call with the check on since the network was set");
    if (!ptrs_ok) return fail(SPDY_ERR_ARG, "null device pointer");
    if (slot < 0 || slot >= SPDY_QC_SLOTS) return fail(SPDY_ERR_ARG, "qc_stats: slot=%d outside [0, %d)", slot, SPDY_QC_SLOTS);
    NEED_DEVICE(l->plan);
    return SPDY_OK;
}

// the stats-only call on a gridded ensemble: [the mask's launch,] the observation stage on every observation, the check's launch
// in the mode that decides nothing
int stats_grid(spdy_letkf *l, const double *const *x, const int *d_use, int slot)
{
    const int *umap = nullptr;
    RC(mask_table(l, d_use, &umap));
    spdy::LetkfObserve o = observe_args(l, x, 0, l->nobs);
    o.umap = umap;
    KERNEL(spdy::launch_letkf_observe(o, l->plan->stream));
    return check_obs(l, umap, false, slot);
}

// the coarse columns of a stride and every grid column's stencil in them (include/spdy.h, "ensemble analysis": weight interpolation)
spdy_letkf::InterpTables interp_tables(int ix, int il, int si, int sj)
{
    spdy_letkf::InterpTables tab;
    std::vector<int> rows;                    // the coarse rows, ascending: 0, sj, 2 sj, ... and il - 1
    for (int j = 0; j < il - 1; j += sj) rows.push_back(j);
    rows.push_back(il - 1);
    const int ni = ix / si;
    for (int j : rows)
        for (int i = 0; i < ix; i += si) tab.coarse.push_back(j * ix + i);
    tab.iidx.assign((size_t)4 * ix * il, 0);
    tab.iwgt.assign((size_t)4 * ix * il, 0.0);
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
                tab.iwgt[at + n] = w[n];
                tab.iidx[at + n] = w[n] != 0.0 ? e[n] : first;      // an entry that is not read repeats the first one that is
            }
        }
    }
    return tab;
}

void drop_interp(spdy_letkf *l)
{
    (void)dev_release(l->plan, l->d_tw);
    l->interp_arrays(Carve{});
    l->si = l->sj = 1;
    l->interp = {};
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
    std::vector<int> var(n), lev(n), atp(PRES ? n : 0);
    std::vector<double> err(n), value(n);
    spdy_letkf::ObsTables tab;                // the object's next tables: moved in once every copy has succeeded
    tab.sidx.resize(4 * n); tab.swgt.resize(4 * n); tab.unit.resize(3 * n); tab.lns.resize(n); tab.rinv.resize(n); tab.lnp.resize(PRES ? n : 0);
    // obs_used is all ones from create on; only an analysis of a network with at-pressure observations writes anything else
    const bool reset_used = p->device >= 0 && (PRES || l->npobs > 0 || l->d_qc_stats);
    std::vector<double> ones(reset_used ? n : 0, 1.0);
    int npobs = 0;
    for (size_t o = 0; o < n; ++o) {
        const OBS &b = host[o];
        stencil(l, b.lon, b.lat, &tab.sidx[4 * o], &tab.swgt[4 * o]);
        unit_vector(b.lon, b.lat, &tab.unit[3 * o]);
        var[o] = b.var;
        if (at_p(b)) {
            lev[o] = 0;                                   // the device's level stays a level: atp marks the observation
            atp[o] = 1;
            tab.lnp[o] = tab.lns[o] = std::log(pressure_of(b) / p0);      // ln sigma_o at ps = 0; the analysis call forms its own
            ++npobs;
        } else {
            lev[o] = b.var == SPDY_OBS_PS ? 0 : b.lev;
            tab.lns[o] = b.var == SPDY_OBS_PS ? 0.0 : l->lv.lev[b.lev];
        }
        tab.rinv[o] = 1.0 / (b.error * b.error);
        err[o] = b.error;
        value[o] = b.value;
    }
    if (p->device >= 0) {
        HIP_TRY(hipSetDevice(p->device));
        auto all = [&]() -> int {
            RC(upload(p, l->d_sidx, tab.sidx.data(), 4 * n * sizeof(int)));
            RC(upload(p, l->d_var, var.data(), n * sizeof(int)));
            RC(upload(p, l->d_lev, lev.data(), n * sizeof(int)));
            RC(upload(p, l->d_swgt, tab.swgt.data(), 4 * n * sizeof(double)));
            RC(upload(p, l->d_ounit, tab.unit.data(), 3 * n * sizeof(double)));
            RC(upload(p, l->d_olns, tab.lns.data(), n * sizeof(double)));
            RC(upload(p, l->d_rinv, tab.rinv.data(), n * sizeof(double)));
            RC(upload(p, l->d_err, err.data(), n * sizeof(double)));
            RC(upload(p, l->d_value, value.data(), n * sizeof(double)));
            if (reset_used) { RC(upload(p, l->d_used, ones.data(), n * sizeof(double))); }
            if (PRES) {
                RC(upload(p, l->d_lnp, tab.lnp.data(), n * sizeof(double)));
                RC(upload(p, l->d_atp, atp.data(), n * sizeof(int)));
            }
            HIP_TRY(hipStreamSynchronize(p->stream));
            return SPDY_OK;
        };
        if (const int rc = all()) {
            // the device tables may be partly new: the object holds no observations now, and no copy is still reading the host
            // arrays when they go
            (void)hipStreamSynchronize(p->stream);
            l->nobs = 0; l->npobs = 0; l->obs = {}; l->nslots = 0;
            l->qc_group.clear(); l->qc_ngroups = spdy::LETKF_VARS; l->qc_analysed = false;
            return rc;
        }
    }
    l->nobs = nobs; l->npobs = npobs;
    l->obs = std::move(tab);
    l->nslots = 0;                            // the ranges were of the network that has just gone
    l->qc_group.clear(); l->qc_ngroups = spdy::LETKF_VARS; l->qc_analysed = false;      // and so were the grouping and what the check kept
    return SPDY_OK;
}
}  // namespace

int spdy_detail::ens_to_grid(spdy_plan *p, int nmem, const double *vor, const double *div, const double *t, const double *q, const double *ps, double *g)
{
    const int nk = nmem * p->tab.kx;
    const size_t L = (size_t)nk * grid_elems(p);
    const spdy_spec_seg segs[3] = {{nk, t}, {nk, q}, {nmem, ps}};
    return spdy_inverse_batch_segs_dev(p, nk, vor, div, g, g + L, 2, 3, segs, nullptr, 1, g + 2 * L, 0, nullptr, nullptr, nullptr, 2);
}

static int ens_analyse(spdy_letkf *l, double *vor, double *div, double *t, double *q, double *ps, const int *d_use, bool slots);

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
    l->lv.kx = kx;
    for (int k = 0; k < kx; ++k) l->lv.lev[k] = std::log(t.fsg[k]);
    *out = l;
    if (p->device < 0) return SPDY_OK;
    auto cleanup = [&](int rc) { spdy_letkf_destroy(l); *out = nullptr; return rc; };
    if (hipSetDevice(p->device) != hipSuccess) return cleanup(fail(SPDY_ERR_HIP, "hipSetDevice failed"));
    const size_t ncol = grid_elems(p), M = (size_t)(max_obs > 0 ? max_obs : 1);
    size_t bytes = 0;
    if (int rc = dev_carve(p, [&](auto &&v) { l->arrays(v, ncol, spec_elems(p), kx); }, &bytes)) return cleanup(rc);
    std::vector<double> cu(3 * ncol);
    for (int j = 0; j < il; ++j)
        for (int i = 0; i < ix; ++i) {
            double u[3];
            unit_vector(i * (360.0 / ix), l->lat[j], u);
            for (int c = 0; c < 3; ++c) cu[c * ncol + (size_t)j * ix + i] = u[c];
        }
    const std::vector<double> ones(M, 1.0);   // obs_used: spdy_letkf_set_obs never has to write it
    const double nused[2] = {(double)nmem, (double)nmem};      // members_used: all of them until a masked call says otherwise
    if (hipMemsetAsync(l->d_grid, 0, bytes, p->stream) != hipSuccess ||
        hipMemcpyAsync(l->d_nused, nused, sizeof(nused), hipMemcpyHostToDevice, p->stream) != hipSuccess ||
        hipMemcpyAsync(l->d_used, ones.data(), M * sizeof(double), hipMemcpyHostToDevice, p->stream) != hipSuccess ||
        hipMemcpyAsync(l->d_colunit, cu.data(), cu.size() * sizeof(double), hipMemcpyHostToDevice, p->stream) != hipSuccess ||
        hipMemcpyAsync(l->d_lnfsg, l->lv.lev, kx * sizeof(double), hipMemcpyHostToDevice, p->stream) != hipSuccess ||
        hipStreamSynchronize(p->stream) != hipSuccess)
        return cleanup(fail(SPDY_ERR_HIP, "letkf_create: upload failed"));
    if (spdy::letkf_prepare(l->lds) != hipSuccess) return cleanup(fail(SPDY_ERR_HIP, "letkf_create: %zu bytes of LDS refused", l->lds));
    // one inverse and one direct batch of the zero workspace, in the shapes spdy_ens_letkf_dev uses: whatever the plan's two
    // transform paths allocate on their first call of this size exists before a capture
    const int nk = nmem * kx;
    const size_t L = (size_t)nk * ncol, LS = (size_t)nk * spec_elems(p);
    double *g = l->d_grid, *s = l->d_spec;
    int rc = ensure_four(p);
    if (!rc) rc = ens_to_grid(p, nmem, s, s + LS, s + 2 * LS, s + 3 * LS, s + 4 * LS, g);
    if (!rc) rc = spdy_direct_batch_dev(p, nk, g, g + L, s, s + LS, 2, 2 * nk + nmem, g + 2 * L, s + 2 * LS);
    if (!rc && hipStreamSynchronize(p->stream) != hipSuccess) rc = fail(SPDY_ERR_HIP, "letkf_create: the first transforms failed");
    return rc ? cleanup(rc) : SPDY_OK;
}

int spdy_letkf_destroy(spdy_letkf *l)
{
    if (!l) return SPDY_OK;
    retire(l, {l->d_tw, l->d_raw, l->d_qc_stats, l->d_rho, l->d_grid});
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

int spdy_relax_set(spdy_letkf *l, double rtpp, double rtps)
{
    NEED_LIVE(l, "analysis object");
    if (!(rtpp >= 0.0 && rtpp <= 1.0)) return fail(SPDY_ERR_ARG, "relax_set: rtpp must lie in [0, 1]");
    if (!(rtps >= 0.0 && rtps <= 1.0)) return fail(SPDY_ERR_ARG, "relax_set: rtps must lie in [0, 1]");
    spdy_plan *p = l->plan;
    if ((rtpp != 0.0 || rtps != 0.0) && p->device >= 0 && !l->d_raw) {
        // the first non-zero setting: the workspace of the raw increments
        NOT_CAPTURING(p, "spdy_relax_set (allocation)");
        HIP_TRY(hipSetDevice(p->device));
        if (const int rc = optional_block(p, l->d_raw, [&](auto &&v) { l->relax_arrays(v, grid_elems(p), (size_t)p->tab.kx); }, no_uploads)) {
            l->rtpp = l->rtps = 0.0;              // the object is left at (0, 0)
            return rc;
        }
    }
    l->rtpp = rtpp; l->rtps = rtps;
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
    spdy_letkf::InterpTables tab = interp_tables(ix, il, si, sj);
    if (p->device >= 0) {
        HIP_TRY(hipSetDevice(p->device));
        const size_t nc = tab.coarse.size(), ncol = grid_elems(p);
        RC(optional_block(p, l->d_tw, [&](auto &&v) { l->interp_arrays(v, nc, ncol, kx); }, [&]() -> int {
            RC(upload(p, l->d_iwgt, tab.iwgt.data(), 4 * ncol * sizeof(double)));
            RC(upload(p, l->d_iidx, tab.iidx.data(), 4 * ncol * sizeof(int)));
            return upload(p, l->d_coarse, tab.coarse.data(), nc * sizeof(int));
        }));                                  // a failure leaves the object at stride (1, 1), where drop_interp has put it
    }
    l->si = si; l->sj = sj;
    l->interp = std::move(tab);
    return SPDY_OK;
}

int spdy_letkf_table(const spdy_letkf *l, const char *name, double *buf, int cap)
{
    NEED_LIVE(l, "analysis object");
    if (!name) return fail(SPDY_ERR_ARG, "null table name");
    const struct { const char *name; const std::vector<int> *index; const std::vector<double> *v; } tables[] = {
        {"stencil_index", &l->obs.sidx, nullptr}, {"coarse_columns", &l->interp.coarse, nullptr}, {"interp_index", &l->interp.iidx, nullptr},
        {"stencil_weight", nullptr, &l->obs.swgt}, {"unit", nullptr, &l->obs.unit}, {"lnsigma", nullptr, &l->obs.lns},
        {"rinv", nullptr, &l->obs.rinv}, {"interp_weight", nullptr, &l->interp.iwgt}, {"lnp", nullptr, &l->obs.lnp}};
    auto give = [&](const auto &v) {          // the table as doubles, whichever it holds
        const int n = static_cast<int>(v.size());
        if (buf && cap < n) return fail(SPDY_ERR_ARG, "analysis table '%s' has %d values, the buffer %d", name, n, cap);
        if (buf) std::copy(v.begin(), v.end(), buf);
        return n;
    };
    for (const auto &t : tables)
        if (!std::strcmp(name, t.name)) return t.index ? give(*t.index) : give(*t.v);
    if (!std::strcmp(name, "slot_first"))
        return give(std::vector<int>(l->slot_first, l->slot_first + (l->nslots ? l->nslots + 1 : 0)));
    if (!std::strcmp(name, "adaptive_inflation"))
        return give(std::vector<double>{l->infl_on ? 1.0 : 0.0, l->infl_sigma_b, l->infl_min, l->infl_max});
    return fail(SPDY_ERR_ARG, "unknown analysis table '%s'", name);
}

int spdy_letkf_field(spdy_letkf *l, const char *name, double **d_ptr)
{
    NEED_LIVE(l, "analysis object");
    if (!name || !d_ptr) return fail(SPDY_ERR_ARG, "null name or result pointer");
    static const struct { const char *name; double *spdy_letkf::*ptr; } fields[] = {
        {"hx", &spdy_letkf::d_hx}, {"hxmean", &spdy_letkf::d_hxmean}, {"y", &spdy_letkf::d_y}, {"departure", &spdy_letkf::d_dep},
        {"weights", &spdy_letkf::d_tw}, {"value", &spdy_letkf::d_value}, {"grid", &spdy_letkf::d_grid},
        {"obs_lnsigma", &spdy_letkf::d_olns}, {"obs_used", &spdy_letkf::d_used}, {"members_used", &spdy_letkf::d_nused},
        {"inflation", &spdy_letkf::d_infl}, {"slot_ps", &spdy_letkf::d_slot_ps}, {"slot_out", &spdy_letkf::d_slot_out},
        {"obs_check", &spdy_letkf::d_qc_check}, {"obs_stats", &spdy_letkf::d_qc_stats}, {"obs_rinv", &spdy_letkf::d_reff},
        {"rho", &spdy_letkf::d_rho}, {"infl_parm", &spdy_letkf::d_infl_parm}, {"obs_s2", &spdy_letkf::d_obs_s2}};
    const auto *f = std::find_if(std::begin(fields), std::end(fields), [&](const auto &t) { return !std::strcmp(name, t.name); });
    if (f == std::end(fields)) return fail(SPDY_ERR_ARG, "unknown analysis field '%s'", name);
    if (f->ptr == &spdy_letkf::d_tw && l->si == 1 && l->sj == 1) return fail(SPDY_ERR_STATE, "letkf: no weight buffer at stride (1, 1)");
    NEED_DEVICE(l->plan);
    if ((f->ptr == &spdy_letkf::d_qc_check || f->ptr == &spdy_letkf::d_qc_stats) && !l->d_qc_stats) {
        // the names of the qc block are valid on every object: asking for one makes the block, and leaves the check off
        NOT_CAPTURING(l->plan, "spdy_letkf_field (allocation of the qc block)");
        RC(qc_block(l));
    }
    if ((f->ptr == &spdy_letkf::d_rho || f->ptr == &spdy_letkf::d_infl_parm || f->ptr == &spdy_letkf::d_obs_s2) && !l->d_rho) {
        // and so are the names of adaptive inflation's block: asking for one makes it, and leaves the feature off
        NOT_CAPTURING(l->plan, "spdy_letkf_field (allocation of the adaptive-inflation block)");
        RC(infl_block(l));
    }
    *d_ptr = l->*(f->ptr);
    if (f->ptr == &spdy_letkf::d_nused && l->masked_last) *d_ptr += 1;      // the count of the kind of call enqueued last
    return SPDY_OK;
}

int spdy_letkf_analyse_grid_dev(spdy_letkf *l, const double *ug, const double *vg, const double *tg, const double *qg, const double *psg,
                                double *du, double *dv, double *dt, double *dq, double *dps)
{
    return spdy_mask_letkf_analyse_grid_dev(l, ug, vg, tg, qg, psg, du, dv, dt, dq, dps, nullptr);
}

int spdy_mask_letkf_analyse_grid_dev(spdy_letkf *l, const double *ug, const double *vg, const double *tg, const double *qg, const double *psg,
                                     double *du, double *dv, double *dt, double *dq, double *dps, const int *d_use)
{
    RC(analysis_ready(l, ug && vg && tg && qg && psg && du && dv && dt && dq && dps, false));
    const double *x[spdy::LETKF_VARS] = {ug, vg, tg, qg, psg};
    double *dx[spdy::LETKF_VARS] = {du, dv, dt, dq, dps};
    return analyse_grid(l, x, dx, d_use);
}

int spdy_ens_letkf_dev(spdy_letkf *l, double *vor, double *div, double *t, double *q, double *ps)
{
    return spdy_mask_ens_letkf_dev(l, vor, div, t, q, ps, nullptr);
}

int spdy_mask_ens_letkf_dev(spdy_letkf *l, double *vor, double *div, double *t, double *q, double *ps, const int *d_use)
{
    RC(analysis_ready(l, vor && div && t && q && ps, false));
    return ens_analyse(l, vor, div, t, q, ps, d_use, false);
}

int spdy_slot_set(spdy_letkf *l, int nslots, const int *first)
{
    NEED_LIVE(l, "analysis object");
    if (nslots < 0 || nslots > SPDY_MAX_SLOTS) return fail(SPDY_ERR_ARG, "slot_set: nslots=%d outside [0, %d]", nslots, SPDY_MAX_SLOTS);
    if (nslots) {
        if (!first) return fail(SPDY_ERR_ARG, "slot_set: null ranges");
        if (first[0] != 0) return fail(SPDY_ERR_ARG, "slot_set: first[0]=%d must be 0", first[0]);
        for (int s = 0; s < nslots; ++s)
            if (first[s + 1] < first[s]) return fail(SPDY_ERR_ARG, "slot_set: first[%d]=%d < first[%d]=%d", s + 1, first[s + 1], s, first[s]);
        if (first[nslots] != l->nobs) return fail(SPDY_ERR_ARG, "slot_set: first[%d]=%d must be nobs=%d", nslots, first[nslots], l->nobs);
    }
    l->nslots = nslots;
    for (int s = 0; s <= nslots; ++s) l->slot_first[s] = nslots ? first[s] : 0;
    for (int s = 0; s < SPDY_MAX_SLOTS; ++s) l->slot_observed[s] = false;
    return SPDY_OK;
}

int spdy_slot_observe_grid_dev(spdy_letkf *l, int slot, const double *ug, const double *vg, const double *tg, const double *qg, const double *psg)
{
    RC(observe_ready(l, slot, ug && vg && tg && qg && psg));
    const double *x[spdy::LETKF_VARS] = {ug, vg, tg, qg, psg};
    return observe_grid(l, slot, x);
}

int spdy_slot_observe_dev(spdy_letkf *l, int slot, const double *vor, const double *div, const double *t, const double *q, const double *ps)
{
    RC(observe_ready(l, slot, vor && div && t && q && ps));
    if (l->slot_first[slot + 1] == l->slot_first[slot]) {      // an empty slot: nothing is enqueued, the transform neither
        l->slot_observed[slot] = true;
        return SPDY_OK;
    }
    RC(ens_to_grid(l->plan, l->nmem, vor, div, t, q, ps, l->d_grid));
    double *x[spdy::LETKF_VARS];
    grid_workspace(l, x);
    return observe_grid(l, slot, x);
}

int spdy_slot_analyse_grid_dev(spdy_letkf *l, const double *ug, const double *vg, const double *tg, const double *qg, const double *psg,
                               double *du, double *dv, double *dt, double *dq, double *dps, const int *d_use)
{
    RC(analysis_ready(l, ug && vg && tg && qg && psg && du && dv && dt && dq && dps, true));
    const double *x[spdy::LETKF_VARS] = {ug, vg, tg, qg, psg};
    double *dx[spdy::LETKF_VARS] = {du, dv, dt, dq, dps};
    return analyse_grid(l, x, dx, d_use, true);
}

int spdy_slot_ens_letkf_dev(spdy_letkf *l, double *vor, double *div, double *t, double *q, double *ps, const int *d_use)
{
    RC(analysis_ready(l, vor && div && t && q && ps, true));
    return ens_analyse(l, vor, div, t, q, ps, d_use, true);
}

int spdy_qc_set(spdy_letkf *l, double gross, int ngroups, const int *group)
{
    NEED_LIVE(l, "analysis object");
    if (!(gross >= 0.0) || !std::isfinite(gross)) return fail(SPDY_ERR_ARG, "qc_set: gross must be finite and >= 0");
    if (group) {
        if (ngroups < 1 || ngroups > SPDY_QC_MAX_GROUPS) return fail(SPDY_ERR_ARG, "qc_set: ngroups=%d outside [1, %d]", ngroups, SPDY_QC_MAX_GROUPS);
        for (int o = 0; o < l->nobs; ++o)
            if (group[o] < 0 || group[o] >= ngroups) return fail(SPDY_ERR_ARG, "qc_set: observation %d: group=%d outside [0, %d)", o, group[o], ngroups);
    }
    spdy_plan *p = l->plan;
    // a grouping of an empty network is still a grouping: one entry keeps it apart from the default
    std::vector<int> table;
    if (group) table.assign(group, group + l->nobs);
    if (group && table.empty()) table.push_back(0);
    const bool on = gross != 0.0 || group;
    if (p->device >= 0) {
        NOT_CAPTURING(p, "spdy_qc_set (upload)");
        HIP_TRY(hipSetDevice(p->device));
        auto all = [&]() -> int {
            if (on) RC(qc_block(l));              // the first setting that turns anything on makes the block
            if (group) RC(upload(p, l->d_qc_group, table.data(), (size_t)l->nobs * sizeof(int)));
            if (!on && l->qc_on() && !l->npobs) {
                // off again: a model-level network's obs_used is all ones, as the observation stage leaves it
                const std::vector<double> ones((size_t)l->nobs, 1.0);
                RC(upload(p, l->d_used, ones.data(), ones.size() * sizeof(double)));
                HIP_TRY(hipStreamSynchronize(p->stream));       // ones goes with this scope
            }
            HIP_TRY(hipStreamSynchronize(p->stream));
            return SPDY_OK;
        };
        if (const int rc = all()) {
            (void)hipStreamSynchronize(p->stream);        // no copy is still reading the host arrays when they go
            l->gross = 0.0; l->qc_group.clear(); l->qc_ngroups = spdy::LETKF_VARS;      // the object is left off
            return rc;
        }
    }
    l->gross = gross;
    l->qc_ngroups = group ? ngroups : (int)spdy::LETKF_VARS;
    l->qc_group = std::move(table);
    return SPDY_OK;
}

int spdy_infl_set(spdy_letkf *l, int on, double sigma_b, double rho_min, double rho_max)
{
    NEED_LIVE(l, "analysis object");
    if (!(sigma_b >= 0.0) || !std::isfinite(sigma_b)) return fail(SPDY_ERR_ARG, "infl_set: sigma_b must be finite and >= 0");
    if (!(rho_min > 0.0) || !std::isfinite(rho_min)) return fail(SPDY_ERR_ARG, "infl_set: rho_min must be finite and > 0");
    if (!(rho_max >= rho_min) || !std::isfinite(rho_max)) return fail(SPDY_ERR_ARG, "infl_set: rho_max must be finite and >= rho_min");
    spdy_plan *p = l->plan;
    if (on && p->device >= 0 && !l->d_rho) {
        // the first "on": the block, the field filled with the scalar rho
        NOT_CAPTURING(p, "spdy_infl_set (allocation)");
        HIP_TRY(hipSetDevice(p->device));
        if (const int rc = infl_block(l)) {
            l->infl_on = false;                       // the object is left off
            return rc;
        }
    }
    l->infl_on = on != 0; l->infl_sigma_b = sigma_b; l->infl_min = rho_min; l->infl_max = rho_max;
    return SPDY_OK;
}

int spdy_infl_fill(spdy_letkf *l, double rho0)
{
    NEED_LIVE(l, "analysis object");
    if (!(rho0 > 0.0) || !std::isfinite(rho0)) return fail(SPDY_ERR_ARG, "infl_fill: rho0 must be finite and > 0");
    spdy_plan *p = l->plan;
    NEED_DEVICE(p);
    NOT_CAPTURING(p, "spdy_infl_fill (upload)");
    RC(infl_block(l));
    const size_t n = (size_t)p->tab.kx * grid_elems(p);
    const std::vector<double> fill(n, rho0);
    const int rc = upload(p, l->d_rho, fill.data(), n * sizeof(double));
    const hipError_t done = hipStreamSynchronize(p->stream);      // fill goes with this scope
    if (rc) return rc;
    HIP_TRY(done);
    return SPDY_OK;
}

int spdy_qc_set_slot(spdy_letkf *l, int slot)
{
    NEED_LIVE(l, "analysis object");
    if (slot < 0 || slot >= SPDY_QC_SLOTS) return fail(SPDY_ERR_ARG, "qc_set_slot: slot=%d outside [0, %d)", slot, SPDY_QC_SLOTS);
    l->qc_slot = slot;
    return SPDY_OK;
}

int spdy_qc_stats_grid_dev(spdy_letkf *l, const double *ug, const double *vg, const double *tg, const double *qg, const double *psg,
                           const int *d_use, int slot)
{
    RC(stats_ready(l, ug && vg && tg && qg && psg, slot));
    const double *x[spdy::LETKF_VARS] = {ug, vg, tg, qg, psg};
    return stats_grid(l, x, d_use, slot);
}

int spdy_qc_stats_dev(spdy_letkf *l, const double *vor, const double *div, const double *t, const double *q, const double *ps,
                      const int *d_use, int slot)
{
    RC(stats_ready(l, vor && div && t && q && ps, slot));
    RC(ens_to_grid(l->plan, l->nmem, vor, div, t, q, ps, l->d_grid));
    double *x[spdy::LETKF_VARS];
    grid_workspace(l, x);
    return stats_grid(l, x, d_use, slot);
}

}  // extern "C"

// spdy_ens_letkf_dev behind its checks: the inverse batch, the analysis on the grid workspace (slots: with the finish kernel in the
// observation kernel's place), the direct batch and the kernel that adds the spectral increments
static int ens_analyse(spdy_letkf *l, double *vor, double *div, double *t, double *q, double *ps, const int *d_use, bool slots)
{
    spdy_plan *p = l->plan;
    const int kx = p->tab.kx, nmem = l->nmem, nk = nmem * kx;
    const size_t L = (size_t)nk * grid_elems(p), LS = (size_t)nk * spec_elems(p);
    double *g = l->d_grid, *s = l->d_spec;
    RC(ens_to_grid(p, nmem, vor, div, t, q, ps, g));
    // the increments take the place of the gridded ensemble
    double *x[spdy::LETKF_VARS];
    grid_workspace(l, x);
    RC(analyse_grid(l, x, x, d_use, slots));
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
