// C ABI of the SPPT pattern (include/spdy.h, "SPPT"): gen_sppt of sppt.f90 device-resident.  Kernels: csrc/spdy_sppt.hip; host
// tables: csrc/spdy_tables.cpp (SpptTables).  The application to the tendencies is part of the column physics
// (csrc/spdy_api_physics.hip).
#include <cstring>
#include <vector>

#include "spdy_plan.hpp"

using namespace spdy_detail;

namespace {
size_t coefs(const spdy_plan *p) { return (size_t)p->tab.mx * p->tab.nx * p->tab.kx; }

// the counters and the seeds of members [first, first + n), stream-ordered as spdy_radiation_set_date's fields; a pattern is zero
// until its first advance
int restart(spdy_sppt *s, int first, int n, const unsigned long long *seeds)
{
    std::vector<spdy::SpptState> h((size_t)n);
    for (int e = 0; e < n; ++e) h[e] = spdy::SpptState{0ull, seeds[e]};
    return upload_sync(s->plan, s->d_state + first, h.data(), sizeof(spdy::SpptState) * (size_t)n);
}

int need_member(const spdy_sppt *s, int member)
{
    if (member < 0 || member >= s->nmem) return fail(SPDY_ERR_ARG, "SPPT member %d outside [0, %d)", member, s->nmem);
    return SPDY_OK;
}
}  // namespace

extern "C" {

int spdy_ens_sppt_create(spdy_plan *p, int nmem, int nsteps, const double *mu, const unsigned long long *seeds, spdy_sppt **out)
{
    NEED_PLAN(p);
    if (nmem < 1) return fail(SPDY_ERR_ARG, "ens_sppt_create: nmem=%d < 1", nmem);
    if (!seeds || !out) return fail(SPDY_ERR_ARG, "null seeds or result pointer");
    NOT_CAPTURING(p, "spdy_sppt_create (host table build + upload)");
    spdy_sppt *s = new spdy_sppt;
    adopt(p, s);
    s->nmem = nmem;
    auto cleanup = [&](int rc) { spdy_sppt_destroy(s); *out = nullptr; return rc; };
    const std::string err = s->tab.build(p->tab, nsteps, mu);
    if (!err.empty()) return cleanup(fail(SPDY_ERR_ARG, "sppt_create: %s", err.c_str()));
    *out = s;
    if (p->device < 0) return SPDY_OK;
    const long nk = (long)nmem * p->tab.kx;
    if (p->max_batch < nk)
        return cleanup(fail(SPDY_ERR_ARG, "max_batch=%d must be >= nmem*kx=%ld for the SPPT patterns' transform", p->max_batch, nk));
    if (hipSetDevice(p->device) != hipSuccess) return cleanup(fail(SPDY_ERR_HIP, "hipSetDevice failed"));
    const size_t nc = coefs(p) * nmem, ng = grid_elems(p) * nk, nsig = s->tab.sigma.size();
    const size_t bytes = (4 * nc + ng + nsig) * sizeof(double);
    if (int rc = dev_alloc(p, bytes, &s->d_eta)) return cleanup(rc);
    if (int rc = dev_alloc(p, sizeof(spdy::SpptState) * (size_t)nmem, &s->d_state)) return cleanup(rc);
    s->d_spec = s->d_eta + 2 * nc; s->d_pattern = s->d_spec + 2 * nc; s->d_sigma = s->d_pattern + ng;
    if (hipMemsetAsync(s->d_eta, 0, bytes, p->stream) != hipSuccess ||
        hipMemcpyAsync(s->d_sigma, s->tab.sigma.data(), nsig * sizeof(double), hipMemcpyHostToDevice, p->stream) != hipSuccess)
        return cleanup(fail(SPDY_ERR_HIP, "sppt_create: upload failed"));
    int rc = restart(s, 0, nmem, seeds);
    // one transform of the zero spectra of all members: whatever the plan's inverse path allocates on its first call of this size
    // exists before a capture
    if (!rc) rc = spdy_spec_to_grid_dev(p, (int)nk, s->d_spec, nullptr, 1, s->d_pattern);
    if (!rc && hipStreamSynchronize(p->stream) != hipSuccess) rc = fail(SPDY_ERR_HIP, "sppt_create: the first transform failed");
    return rc ? cleanup(rc) : SPDY_OK;
}

int spdy_sppt_create(spdy_plan *p, int nsteps, const double *mu, unsigned long long seed, spdy_sppt **out)
{
    return spdy_ens_sppt_create(p, 1, nsteps, mu, &seed, out);
}

int spdy_sppt_members(const spdy_sppt *s)
{
    NEED_LIVE(s, "SPPT pattern");
    return s->nmem;
}

int spdy_sppt_destroy(spdy_sppt *s)
{
    if (!s) return SPDY_OK;
    retire(s, {s->d_eta, s->d_state});
    delete s;
    return SPDY_OK;
}

int spdy_ens_sppt_reset(spdy_sppt *s, int member, unsigned long long seed)
{
    NEED_LIVE(s, "SPPT pattern");
    RC(need_member(s, member));
    spdy_plan *p = s->plan;
    NOT_CAPTURING(p, "spdy_sppt_reset (upload)");
    NEED_DEVICE(p);
    return restart(s, member, 1, &seed);
}

int spdy_sppt_reset(spdy_sppt *s, unsigned long long seed) { return spdy_ens_sppt_reset(s, 0, seed); }

int spdy_sppt_table(const spdy_sppt *s, const char *name, double *buf, int cap)
{
    NEED_LIVE(s, "SPPT pattern");
    if (!name) return fail(SPDY_ERR_ARG, "null table name");
    const std::vector<double> *v = s->tab.lookup(name);
    if (!v) return fail(SPDY_ERR_ARG, "unknown SPPT table '%s'", name);
    const int n = static_cast<int>(v->size());
    if (buf && cap < n) return fail(SPDY_ERR_ARG, "SPPT table '%s' has %d values, the buffer %d", name, n, cap);
    if (buf) std::memcpy(buf, v->data(), sizeof(double) * (size_t)n);
    return n;
}

int spdy_sppt_field(spdy_sppt *s, const char *name, double **d_ptr)
{
    NEED_LIVE(s, "SPPT pattern");
    if (!name || !d_ptr) return fail(SPDY_ERR_ARG, "null name or result pointer");
    double *const *f = !std::strcmp(name, "eta") ? &s->d_eta : !std::strcmp(name, "spec") ? &s->d_spec
                       : !std::strcmp(name, "pattern") ? &s->d_pattern : nullptr;
    if (!f) return fail(SPDY_ERR_ARG, "unknown SPPT field '%s'", name);
    NEED_DEVICE(s->plan);
    *d_ptr = *f;
    return SPDY_OK;
}

int spdy_ens_sppt_draws(spdy_sppt *s, int member, long long *draws)
{
    NEED_LIVE(s, "SPPT pattern");
    RC(need_member(s, member));
    if (!draws) return fail(SPDY_ERR_ARG, "null result pointer");
    spdy_plan *p = s->plan;
    NOT_CAPTURING(p, "spdy_sppt_draws (download)");
    NEED_DEVICE(p);
    spdy::SpptState h{};
    RC(download_sync(p, &h, s->d_state + member, sizeof(h)));
    *draws = (long long)h.draws;
    return SPDY_OK;
}

int spdy_sppt_draws(spdy_sppt *s, long long *draws) { return spdy_ens_sppt_draws(s, 0, draws); }

int spdy_sppt_advance_dev(spdy_sppt *s, const double *d_eta)
{
    NEED_LIVE(s, "SPPT pattern");
    spdy_plan *p = s->plan;
    NEED_DEVICE(p);
    const int nk = s->nmem * p->tab.kx;
    spdy::SpptNoise a{};
    a.n = (int)coefs(p); a.nspec = p->tab.mx * p->tab.nx; a.nmem = s->nmem;
    a.state = s->d_state; a.sigma = s->d_sigma; a.eta_in = d_eta; a.eta = s->d_eta; a.spec = s->d_spec;
    a.phi = s->tab.phi[0]; a.first = s->tab.first[0];
    KERNEL(spdy::launch_sppt_noise(a, p->stream));
    // sppt.f90:93-95: the reference never truncates sppt_spec and draws imaginary parts for m = 0; its spec_to_grid reads neither
    // (legendre.f90:93, fourier.f90:34-38), and neither does the plan's inverse.  The members are nmem * kx fields of ONE launch.
    RC(spdy_spec_to_grid_dev(p, nk, s->d_spec, nullptr, 1, s->d_pattern));
    KERNEL(spdy::launch_sppt_clip(s->d_pattern, (long)(grid_elems(p) * p->tab.kx), s->nmem, s->d_state, p->stream));
    return SPDY_OK;
}

}  // extern "C"
