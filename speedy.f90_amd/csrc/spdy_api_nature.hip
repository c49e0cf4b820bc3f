// C ABI of the nature run (include/spdy.h, "nature run"): the gridded truth of a twin experiment, the observation
// values of an analysis object's network drawn from it, and the scores of an ensemble against it.  Kernels: csrc/spdy_nature.hip.
#include <cmath>
#include <cstring>
#include <vector>

#include "spdy_plan.hpp"

using namespace spdy_detail;

namespace {
int rows(const spdy_plan *p) { return 4 * p->tab.kx + 1; }

// the checks the two calls that take an analysis object share, in the documented order: both objects, then their plans
int need_pair(spdy_nature *n, spdy_letkf *l)
{
    NEED_LIVE(n, "nature run");
    NEED_LIVE(l, "analysis object");
    if (l->plan != n->plan) return fail(SPDY_ERR_ARG, "nature: the analysis object belongs to another plan");
    return SPDY_OK;
}

// the scores of a gridded ensemble x = u | v | t | q | ps into scores[slot]: two launches; d_use: NULL, or the member mask
int score(spdy_nature *n, int nmem, const double *const *x, int slot, const int *d_use)
{
    spdy_plan *p = n->plan;
    spdy::NatureScore a{};
    a.nmem = nmem; a.kx = p->tab.kx; a.ix = p->tab.ix; a.il = p->tab.il;
    for (int v = 0; v < spdy::LETKF_VARS; ++v) a.x[v] = x[v];
    a.use = d_use;
    a.truth = n->d_truth; a.gw = n->d_gw; a.part = n->d_part; a.scores = n->d_scores + (size_t)slot * 3 * rows(p);
    KERNEL(spdy::launch_nature_score(a, p->stream));
    return SPDY_OK;
}

int need_slot(const spdy_nature *n, const char *call, int slot)
{
    if (slot < 0 || slot >= n->capacity) return fail(SPDY_ERR_ARG, "%s: slot=%d outside [0, capacity=%d)", call, slot, n->capacity);
    return SPDY_OK;
}

// the values of the observations [first, last) of l's network, by the network's kind, then the counter: two launches; an empty
// range launches the count alone
int draw(spdy_nature *n, spdy_letkf *l, int first, int last, double noise)
{
    spdy_plan *p = n->plan;
    spdy::NatureObs o{};
    o.first = first; o.last = last; o.nobs = l->nobs; o.kx = p->tab.kx; o.ncol = (int)grid_elems(p);
    o.var = l->d_var; o.lev = l->d_lev; o.sidx = l->d_sidx; o.swgt = l->d_swgt; o.error = l->d_err;
    o.truth = n->d_truth; o.state = n->d_state; o.noise = noise; o.value = l->d_value;
    if (l->npobs) { o.atp = l->d_atp; o.lnp = l->d_lnp; o.lv = l->lv; }
    KERNEL(spdy::launch_nature_slot_draw(o, p->stream));
    KERNEL(spdy::launch_nature_count(n->d_state, p->stream));
    return SPDY_OK;
}

int restart(spdy_nature *n, unsigned long long seed)
{
    const unsigned long long h[2] = {seed, 0ull};
    return upload_sync(n->plan, n->d_state, h, sizeof(h));
}
}  // namespace

extern "C" {

int spdy_nature_create(spdy_plan *p, unsigned long long seed, int capacity, spdy_nature **out)
{
    NEED_PLAN(p);
    if (capacity < 1) return fail(SPDY_ERR_ARG, "nature_create: capacity=%d < 1", capacity);
    if (!out) return fail(SPDY_ERR_ARG, "null result pointer");
    const spdy::HostTables &t = p->tab;
    const int kx = t.kx, il = t.il, nf = rows(p);
    if (p->max_batch < 2 * kx + 1) return fail(SPDY_ERR_ARG, "nature_create: max_batch=%d must be >= 2*kx+1=%d", p->max_batch, 2 * kx + 1);
    if (!t.sigma_ready) return fail(SPDY_ERR_STATE, "nature_create needs sigma levels");
    NOT_CAPTURING(p, "spdy_nature_create (allocation + upload)");
    spdy_nature *n = new spdy_nature;
    adopt(p, n);
    n->capacity = capacity;
    *out = n;
    if (p->device < 0) return SPDY_OK;
    auto cleanup = [&](int rc) { spdy_nature_destroy(n); *out = nullptr; return rc; };
    if (hipSetDevice(p->device) != hipSuccess) return cleanup(fail(SPDY_ERR_HIP, "hipSetDevice failed"));
    // the Gaussian weights of the rows, south first, divided by their sum over the rows in ascending order
    std::vector<double> gw(il);
    double sum = 0.0;
    for (int j = 0; j < il; ++j) {
        gw[j] = t.wt[j < t.iy ? j : il - 1 - j];
        sum += gw[j];
    }
    for (int j = 0; j < il; ++j) gw[j] /= sum;
    const size_t ncol = grid_elems(p), ns = spec_elems(p);
    size_t bytes = 0;
    if (int rc = dev_carve(p, [&](auto &&v) { n->arrays(v, (size_t)nf, ncol, ns, (size_t)il); }, &bytes)) return cleanup(rc);
    if (hipMemsetAsync(n->d_truth, 0, bytes, p->stream) != hipSuccess ||
        hipMemcpyAsync(n->d_gw, gw.data(), il * sizeof(double), hipMemcpyHostToDevice, p->stream) != hipSuccess)
        return cleanup(fail(SPDY_ERR_HIP, "nature_create: upload failed"));
    int rc = restart(n, seed);
    // one inverse batch of zero spectra in set_state's shape: whatever the plan's inverse path allocates on its first call of this
    // size exists before a capture (verify's shape is the analysis object's, which its create has run)
    if (!rc) rc = ensure_four(p);
    const size_t LS = (size_t)kx * ns;
    const double *s = n->d_zero;
    if (!rc) rc = ens_to_grid(p, 1, s, s + LS, s + 2 * LS, s + 3 * LS, s + 4 * LS, n->d_truth);
    if (!rc && hipStreamSynchronize(p->stream) != hipSuccess) rc = fail(SPDY_ERR_HIP, "nature_create: the first transform failed");
    return rc ? cleanup(rc) : SPDY_OK;
}

int spdy_nature_destroy(spdy_nature *n)
{
    if (!n) return SPDY_OK;
    retire(n, {n->d_truth});
    delete n;
    return SPDY_OK;
}

int spdy_nature_reset(spdy_nature *n, unsigned long long seed)
{
    NEED_LIVE(n, "nature run");
    spdy_plan *p = n->plan;
    NOT_CAPTURING(p, "spdy_nature_reset (upload)");
    NEED_DEVICE(p);
    return restart(n, seed);
}

int spdy_nature_draws(spdy_nature *n, long long *count)
{
    NEED_LIVE(n, "nature run");
    if (!count) return fail(SPDY_ERR_ARG, "null result pointer");
    spdy_plan *p = n->plan;
    NOT_CAPTURING(p, "spdy_nature_draws (download)");
    NEED_DEVICE(p);
    unsigned long long h[2] = {0ull, 0ull};
    RC(download_sync(p, h, n->d_state, sizeof(h)));
    *count = (long long)h[1];
    return SPDY_OK;
}

int spdy_nature_field(spdy_nature *n, const char *name, double **d_ptr)
{
    NEED_LIVE(n, "nature run");
    if (!name || !d_ptr) return fail(SPDY_ERR_ARG, "null name or result pointer");
    const int which = !std::strcmp(name, "truth") ? 0 : !std::strcmp(name, "scores") ? 1 : !std::strcmp(name, "state") ? 2 : -1;
    if (which < 0) return fail(SPDY_ERR_ARG, "unknown nature field '%s'", name);
    NEED_DEVICE(n->plan);
    *d_ptr = which == 0 ? n->d_truth : which == 1 ? n->d_scores : reinterpret_cast<double *>(n->d_state);
    return SPDY_OK;
}

int spdy_nature_set_state_dev(spdy_nature *n, const double *vor, const double *div, const double *t, const double *q, const double *ps)
{
    NEED_LIVE(n, "nature run");
    if (!vor || !div || !t || !q || !ps) return fail(SPDY_ERR_ARG, "null device pointer");
    spdy_plan *p = n->plan;
    NEED_DEVICE(p);
    return ens_to_grid(p, 1, vor, div, t, q, ps, n->d_truth);
}

int spdy_nature_observe_dev(spdy_nature *n, spdy_letkf *l, double noise)
{
    RC(need_pair(n, l));
    if (!(noise >= 0.0) || !std::isfinite(noise)) return fail(SPDY_ERR_ARG, "nature_observe: noise must be finite and >= 0");
    spdy_plan *p = n->plan;
    NEED_DEVICE(p);
    return draw(n, l, 0, l->nobs, noise);
}

int spdy_slot_nature_observe_dev(spdy_nature *n, spdy_letkf *l, int slot, double noise)
{
    RC(need_pair(n, l));
    if (!(noise >= 0.0) || !std::isfinite(noise)) return fail(SPDY_ERR_ARG, "slot_nature_observe: noise must be finite and >= 0");
    if (!l->nslots) return fail(SPDY_ERR_STATE, "slot_nature_observe: spdy_slot_set first");
    if (slot < 0 || slot >= l->nslots) return fail(SPDY_ERR_ARG, "slot_nature_observe: slot=%d outside [0, nslots=%d)", slot, l->nslots);
    spdy_plan *p = n->plan;
    NEED_DEVICE(p);
    return draw(n, l, l->slot_first[slot], l->slot_first[slot + 1], noise);
}

int spdy_nature_verify_dev(spdy_nature *n, spdy_letkf *l, const double *vor, const double *div, const double *t, const double *q,
                           const double *ps, int slot)
{
    return spdy_mask_nature_verify_dev(n, l, vor, div, t, q, ps, nullptr, slot);
}

int spdy_mask_nature_verify_dev(spdy_nature *n, spdy_letkf *l, const double *vor, const double *div, const double *t, const double *q,
                                const double *ps, const int *d_use, int slot)
{
    RC(need_pair(n, l));
    RC(need_slot(n, "nature_verify", slot));
    if (!vor || !div || !t || !q || !ps) return fail(SPDY_ERR_ARG, "null device pointer");
    spdy_plan *p = n->plan;
    NEED_DEVICE(p);
    const int nmem = l->nmem;
    const size_t L = (size_t)nmem * p->tab.kx * grid_elems(p);
    double *g = l->d_grid;
    RC(ens_to_grid(p, nmem, vor, div, t, q, ps, g));
    const double *x[spdy::LETKF_VARS] = {g, g + L, g + 2 * L, g + 3 * L, g + 4 * L};
    return score(n, nmem, x, slot, d_use);
}

int spdy_nature_verify_grid_dev(spdy_nature *n, int nmem, const double *ug, const double *vg, const double *tg, const double *qg,
                                const double *psg, int slot)
{
    return spdy_mask_nature_verify_grid_dev(n, nmem, ug, vg, tg, qg, psg, nullptr, slot);
}

int spdy_mask_nature_verify_grid_dev(spdy_nature *n, int nmem, const double *ug, const double *vg, const double *tg, const double *qg,
                                     const double *psg, const int *d_use, int slot)
{
    NEED_LIVE(n, "nature run");
    if (nmem < 2 || nmem > spdy::LETKF_MAX_MEMBERS)
        return fail(SPDY_ERR_ARG, "nature_verify_grid: nmem=%d outside [2, %d]", nmem, spdy::LETKF_MAX_MEMBERS);
    RC(need_slot(n, "nature_verify_grid", slot));
    if (!ug || !vg || !tg || !qg || !psg) return fail(SPDY_ERR_ARG, "null device pointer");
    NEED_DEVICE(n->plan);
    const double *x[spdy::LETKF_VARS] = {ug, vg, tg, qg, psg};
    return score(n, nmem, x, slot, d_use);
}

}  // extern "C"
