// C ABI of the run's guard (include/spdy.h, "diagnostics"): check_diagnostics of diagnostics.f90 device-resident.  Kernel:
// csrc/spdy_diagnostics.hip.  The object owns the history ring, the limits and the per-level state; the host side here creates
// and resets them, downloads them (status, read) and writes the reference's three lines (format).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "spdy_plan.hpp"

using namespace spdy_detail;

namespace {
constexpr int MAX_CAPACITY = 1 << 20;

size_t row_doubles(const spdy_diagnostics *d) { return (size_t)3 * d->plan->tab.kx; }           // one member's (3, kx) block
size_t levels(const spdy_diagnostics *d) { return (size_t)d->nmem * d->plan->tab.kx; }            // DiagLevel records

// the state of a run that starts at next_step and an empty ring, stream-ordered
int restart(spdy_diagnostics *d, long long next_step)
{
    spdy_plan *p = d->plan;
    spdy::DiagLevel l{};
    l.next_step = next_step; l.bad_step = -1; l.row_step = -1;
    const std::vector<spdy::DiagLevel> h(levels(d), l);
    HIP_TRY(hipMemsetAsync(d->d_history, 0, (size_t)d->capacity * d->nmem * row_doubles(d) * sizeof(double), p->stream));
    RC(upload_sync(p, d->d_state, h.data(), h.size() * sizeof(l)));
    d->start_step = next_step;
    return SPDY_OK;
}

int upload_limits(spdy_diagnostics *d, const double *limits)
{
    static const double stock[4] = {500.0, 500.0, 180.0, 320.0};             // diagnostics.f90:61-62
    return upload_sync(d->plan, d->d_limits, limits ? limits : stock, sizeof(stock));
}

int download_state(spdy_diagnostics *d, std::vector<spdy::DiagLevel> &h)
{
    h.resize(levels(d));
    RC(download_sync(d->plan, h.data(), d->d_state, h.size() * sizeof(h[0])));
    for (const auto &l : h)
        if (l.next_step != h[0].next_step) return fail(SPDY_ERR_STATE, "the levels' step counters disagree (%lld, %lld)", h[0].next_step, l.next_step);
    return SPDY_OK;
}

// the first offending step of the member whose levels are h[0 .. kx) (-1: none)
long long first_offence(const spdy::DiagLevel *h, int kx)
{
    long long first = -1;
    for (int k = 0; k < kx; ++k)
        if (h[k].bad_step >= 0 && (first < 0 || h[k].bad_step < first)) first = h[k].bad_step;
    return first;
}

int need_member(const spdy_diagnostics *d, int member, const char *what)
{
    if (member < 0 || member >= d->nmem) return fail(SPDY_ERR_ARG, "%s: member %d is not in 0 .. %d", what, member, d->nmem - 1);
    return SPDY_OK;
}

int need_single(const spdy_diagnostics *d, const char *what, const char *form)
{
    if (d->nmem > 1) return fail(SPDY_ERR_ARG, "%s: the object checks %d members, use %s with a member", what, d->nmem, form);
    return SPDY_OK;
}

// Fortran's f8.2
void f8_2(double x, char *out)
{
    char tmp[400];
    if (std::isnan(x)) std::snprintf(tmp, sizeof(tmp), "%8s", "NaN");
    else if (std::isinf(x)) std::snprintf(tmp, sizeof(tmp), "%8s", x > 0 ? "Inf" : "-Inf");
    else std::snprintf(tmp, sizeof(tmp), "%8.2f", x);
    std::memcpy(out, std::strlen(tmp) == 8 ? tmp : "********", 8);
}
}  // namespace

extern "C" {

int spdy_diagnostics_create(spdy_plan *p, int capacity, long long first_step, spdy_diagnostics **out)
{
    return spdy_ens_diagnostics_create(p, 1, capacity, first_step, out);
}

int spdy_ens_diagnostics_create(spdy_plan *p, int nmem, int capacity, long long first_step, spdy_diagnostics **out)
{
    NEED_PLAN(p);
    if (nmem < 1 || nmem > 65535) return fail(SPDY_ERR_ARG, "diagnostics_create: nmem=%d is not in 1 .. 65535", nmem);
    if (!out) return fail(SPDY_ERR_ARG, "null result pointer");
    if (capacity < 1 || capacity > MAX_CAPACITY) return fail(SPDY_ERR_ARG, "diagnostics_create: capacity %d is not in 1 .. %d", capacity, MAX_CAPACITY);
    if (first_step < 0) return fail(SPDY_ERR_ARG, "diagnostics_create: first_step %lld is negative", first_step);
    NOT_CAPTURING(p, "spdy_diagnostics_create (allocation + upload)");
    spdy_diagnostics *d = new spdy_diagnostics;
    adopt(p, d);
    d->capacity = capacity; d->nmem = nmem; d->start_step = first_step;
    *out = d;
    if (p->device < 0) return SPDY_OK;
    auto cleanup = [&](int rc) { spdy_diagnostics_destroy(d); *out = nullptr; return rc; };
    if (hipSetDevice(p->device) != hipSuccess) return cleanup(fail(SPDY_ERR_HIP, "hipSetDevice failed"));
    if (int rc = dev_carve(p, [&](auto &&v) { d->arrays(v, (size_t)p->tab.kx); })) return cleanup(rc);
    int rc = upload_limits(d, nullptr);
    if (!rc) rc = restart(d, first_step);
    return rc ? cleanup(rc) : SPDY_OK;
}

int spdy_diagnostics_destroy(spdy_diagnostics *d)
{
    if (!d) return SPDY_OK;
    retire(d, {d->d_history});
    delete d;
    return SPDY_OK;
}

int spdy_diagnostics_set_limits(spdy_diagnostics *d, const double *limits)
{
    NEED_LIVE(d, "diagnostics object");
    spdy_plan *p = d->plan;
    NOT_CAPTURING(p, "spdy_diagnostics_set_limits (upload)");
    NEED_DEVICE(p);
    return upload_limits(d, limits);
}

int spdy_diagnostics_reset(spdy_diagnostics *d, long long next_step)
{
    NEED_LIVE(d, "diagnostics object");
    if (next_step < 0) return fail(SPDY_ERR_ARG, "diagnostics_reset: next_step %lld is negative", next_step);
    spdy_plan *p = d->plan;
    NOT_CAPTURING(p, "spdy_diagnostics_reset (upload)");
    NEED_DEVICE(p);
    return restart(d, next_step);
}

int spdy_diagnostics_check_dev(spdy_diagnostics *d, const double *vor, const double *div, const double *t)
{
    NEED_LIVE(d, "diagnostics object");
    if (!vor || !div || !t) return fail(SPDY_ERR_ARG, "diagnostics_check_dev: null spectra");
    spdy_plan *p = d->plan;
    NEED_DEVICE(p);
    spdy::DiagArgs a{};
    a.vor = vor; a.div = div; a.t = t;
    a.elm2 = p->dev.elm2; a.limits = d->d_limits; a.history = d->d_history; a.state = d->d_state;
    a.nspec = p->tab.mx * p->tab.nx; a.mx = p->tab.mx; a.kx = p->tab.kx; a.capacity = d->capacity; a.nmem = d->nmem;
    KERNEL(spdy::launch_diagnostics(a, p->stream));
    return SPDY_OK;
}

int spdy_mask_from_diagnostics_dev(spdy_diagnostics *d, int *d_use)
{
    NEED_LIVE(d, "diagnostics object");
    if (!d_use) return fail(SPDY_ERR_ARG, "mask_from_diagnostics_dev: null mask");
    spdy_plan *p = d->plan;
    NEED_DEVICE(p);
    KERNEL(spdy::launch_diagnostics_use(d->d_state, d->nmem, p->tab.kx, d_use, p->stream));
    return SPDY_OK;
}

int spdy_diagnostics_status(spdy_diagnostics *d, long long *next_step, long long *bad_step, int *bad_level, int *bad_mask, double *bad_row)
{
    NEED_LIVE(d, "diagnostics object");
    RC(need_single(d, "diagnostics_status", "spdy_ens_diagnostics_status"));
    return spdy_ens_diagnostics_status(d, 0, next_step, bad_step, bad_level, bad_mask, bad_row);
}

int spdy_ens_diagnostics_status(spdy_diagnostics *d, int member, long long *next_step, long long *bad_step, int *bad_level, int *bad_mask,
                                double *bad_row)
{
    NEED_LIVE(d, "diagnostics object");
    RC(need_member(d, member, "diagnostics_status"));
    spdy_plan *p = d->plan;
    NOT_CAPTURING(p, "spdy_diagnostics_status (download)");
    NEED_DEVICE(p);
    std::vector<spdy::DiagLevel> all;
    RC(download_state(d, all));
    const int kx = p->tab.kx;
    const spdy::DiagLevel *const h = all.data() + (size_t)member * kx;               // the member's levels
    const long long first = first_offence(h, kx);
    int level = -1, mask = 0;
    for (int k = 0; k < kx && first >= 0; ++k) {
        if (h[k].bad_step == first) { mask |= h[k].bad_mask; if (level < 0) level = k; }
        // every level of the member stopped refreshing its saved row at the first offence of any of them
        if (h[k].row_step != first)
            return fail(SPDY_ERR_STATE, "level %d saved the row of step %lld, the first offence is at step %lld", k, h[k].row_step, first);
    }
    if (next_step) *next_step = h[0].next_step;
    if (bad_step) *bad_step = first;
    if (bad_level) *bad_level = level;
    if (bad_mask) *bad_mask = mask;
    if (bad_row && first >= 0)
        for (int k = 0; k < kx; ++k)
            for (int i = 0; i < 3; ++i) bad_row[i * kx + k] = h[k].row[i];
    return SPDY_OK;
}

int spdy_diagnostics_read(spdy_diagnostics *d, long long step, int count, double *rows)
{
    NEED_LIVE(d, "diagnostics object");
    RC(need_single(d, "diagnostics_read", "spdy_ens_diagnostics_read"));
    return spdy_ens_diagnostics_read(d, 0, step, count, rows);
}

int spdy_ens_diagnostics_read(spdy_diagnostics *d, int member, long long step, int count, double *rows)
{
    NEED_LIVE(d, "diagnostics object");
    RC(need_member(d, member, "diagnostics_read"));
    if (!rows) return fail(SPDY_ERR_ARG, "null result pointer");
    if (count < 1) return fail(SPDY_ERR_ARG, "diagnostics_read: count %d", count);
    spdy_plan *p = d->plan;
    NOT_CAPTURING(p, "spdy_diagnostics_read (download)");
    NEED_DEVICE(p);
    std::vector<spdy::DiagLevel> h;
    RC(download_state(d, h));
    const long long next = h[0].next_step, oldest = std::max(d->start_step, next - d->capacity);
    if (step < oldest || count > next - step)
        return fail(SPDY_ERR_ARG, "diagnostics_read: steps %lld .. %lld asked, the ring holds %lld .. %lld", step, step + count - 1, oldest, next - 1);
    const size_t nrow = row_doubles(d);
    for (int i = 0; i < count; ++i)
        HIP_TRY(hipMemcpyAsync(rows + (size_t)i * nrow, d->d_history + ((size_t)((step + i) % d->capacity) * d->nmem + member) * nrow, nrow * sizeof(double),
                               hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return SPDY_OK;
}

int spdy_ens_diagnostics_stopped(spdy_diagnostics *d, long long *bad_step)
{
    NEED_LIVE(d, "diagnostics object");
    if (!bad_step) return fail(SPDY_ERR_ARG, "null result pointer");
    spdy_plan *p = d->plan;
    NOT_CAPTURING(p, "spdy_ens_diagnostics_stopped (download)");
    NEED_DEVICE(p);
    std::vector<spdy::DiagLevel> h;
    RC(download_state(d, h));                                                   // one synchronisation, one download
    int stopped = 0;
    for (int e = 0; e < d->nmem; ++e) {
        bad_step[e] = first_offence(h.data() + (size_t)e * p->tab.kx, p->tab.kx);
        stopped += bad_step[e] >= 0;
    }
    return stopped;
}

int spdy_diagnostics_field(spdy_diagnostics *d, const char *name, void **d_ptr)
{
    NEED_LIVE(d, "diagnostics object");
    if (!name || !d_ptr) return fail(SPDY_ERR_ARG, "null name or result pointer");
    const int which = !std::strcmp(name, "history") ? 0 : !std::strcmp(name, "state") ? 1 : !std::strcmp(name, "limits") ? 2 : -1;
    if (which < 0) return fail(SPDY_ERR_ARG, "unknown diagnostics field '%s'", name);
    NEED_DEVICE(d->plan);
    *d_ptr = which == 0 ? (void *)d->d_history : which == 1 ? (void *)d->d_state : (void *)d->d_limits;
    return SPDY_OK;
}

// diagnostics.f90:72-74: ' step =', i6, ' reke =', (10f8.2) / 13x, ' deke =', (10f8.2) / 13x, ' temp =', (10f8.2); past ten values
// format reversion goes back to the group (10f8.2): records of up to ten f8.2 fields and nothing else
int spdy_diagnostics_format(int kx, long long step, const double *row, char *buf, int cap)
{
    if (kx < 1) return fail(SPDY_ERR_ARG, "diagnostics_format: kx %d", kx);
    if (!row) return fail(SPDY_ERR_ARG, "null row");
    std::string s;
    char f[32];
    for (int i = 0; i < 3; ++i) {
        if (i == 0) {
            std::snprintf(f, sizeof(f), "%6lld", step);
            s += " step =";
            s += std::strlen(f) == 6 ? f : "******";
        } else {
            s += std::string(13, ' ');
        }
        s += i == 0 ? " reke =" : i == 1 ? " deke =" : " temp =";
        for (int k = 0; k < kx; ++k) {
            if (k && k % 10 == 0) s += '\n';
            f8_2(row[i * kx + k], f);
            s.append(f, 8);
        }
        s += '\n';
    }
    const int n = (int)s.size();
    if (!buf) return n;
    if (cap < n + 1) return fail(SPDY_ERR_ARG, "diagnostics_format: %d characters and the terminator, the buffer holds %d", n, cap);
    std::memcpy(buf, s.c_str(), (size_t)n + 1);
    return n;
}

}  // extern "C"
