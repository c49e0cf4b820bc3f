// Internal: the plan object behind include/spdy.h and the helpers shared by the C-ABI translation units
// (spdy_api.hip: plan, transforms, operators, graphs; spdy_api_step.hip: time-step tail, output; spdy_api_shard.hip:
// collectives; spdy_api_physics.hip: column physics; spdy_api_surfmodel.hip, spdy_api_sppt.hip,
// spdy_api_diagnostics.hip, spdy_api_letkf.hip, spdy_api_nature.hip: the objects made on a plan).
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/spdy.h"
#include "spdy_kernels.hpp"
#include "spdy_tables.hpp"

struct spdy_graph {
    struct spdy_plan *plan = nullptr;   // nullptr once the plan is gone: the graph is then dead (SPDY_ERR_STATE)
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

namespace spdy_detail {
// What every object made on a plan starts with (surface model, SPPT pattern, diagnostics, analysis, nature run).  The plan lists its live
// objects; their device memory is the plan's (dev_alloc / dev_release).  spdy_plan_destroy sets plan = nullptr in each: the handle
// stays valid but dead, every call but _destroy then returns SPDY_ERR_STATE (NEED_LIVE), as with graphs and communicators.
struct PlanObject {
    spdy_plan *plan = nullptr;
    virtual void forget_device() = 0;   // null every device pointer: the plan has freed what they pointed at
protected:
    ~PlanObject() = default;
};

// A device workspace allocated at its first use and grown when a larger one is asked for (ensure_workspace).
struct Workspace { double *g = nullptr; size_t doubles = 0; };

// An object that keeps several arrays in one device allocation (diagnostics, analysis, nature run) declares them once, in a
// member template `arrays(v, counts...)` that calls v(pointer member, element count) for each array in memory order.  Carve is
// the visitor: it hands out array after array from `base`, or null pointers without one (forget_device; the counts default to 0
// where only the pointers matter), adds up the bytes and notes an array that would start off its element's alignment
// (dev_carve).  The first array is the allocation's base, what retire and dev_release are given.  Adding an array to such an
// object: the member and its line in `arrays`; its upload if it has one; its public name if it has one.
struct Carve {
    char *base = nullptr;
    size_t bytes = 0;
    bool aligned = true;
    template <class T> void operator()(T *&ptr, size_t n)
    {
        aligned = aligned && bytes % alignof(T) == 0;
        ptr = base ? reinterpret_cast<T *>(base + bytes) : nullptr;
        bytes += n * sizeof(T);
    }
};
}  // namespace spdy_detail

struct spdy_plan {
    spdy::HostTables tab;
    int max_batch = 0;
    int device = -1;
    spdy::DevPlan dev{};
    hipStream_t own_stream = nullptr, stream = nullptr;
    std::vector<void *> allocs;       // everything hipMalloc'ed for this plan
    double *four = nullptr;           // [max_batch][il][fs] Fourier workspace (four-kernel path only; allocated on demand)
    // Host-pointer API staging, allocated at the first host-pointer call: two sets of four buffers.  These are the plan's
    // resources only; which set a call uses, and what it still has to copy out, is the call's own (spdy_detail::HostCall below).
    size_t stage_elems = 0;
    double *dstage[4] = {nullptr, nullptr, nullptr, nullptr};   // device memory, max_batch grids each
    double *hstage[4] = {nullptr, nullptr, nullptr, nullptr};   // hipHostMalloc (mapped, coherent), hstage_elems doubles each
    int *h_kcos = nullptr;                                      // hstage-route twin of d_kcos
    unsigned *h_stamp = nullptr;                                // host-mapped completion stamp of the hstage route (HostCall::finish)
    unsigned stamp_seq = 0;
    size_t hstage_elems = 0;
    const double *d_zero_spec = nullptr;         // one all-zero spectrum (gradient tiles of the mixed inverse kernel)
    double *tmp_c = nullptr, *tmp_d = nullptr;   // max_batch spectra each; allocated with `four` (multi-kernel operator sequences)
    // On-demand workspaces (ensure_workspace).  One that has to grow is allocated anew: the smaller earlier one stays with the plan
    // until it is destroyed, a captured graph may still point into it.
    using Workspace = spdy_detail::Workspace;
    Workspace out_grid, out_spec;     // output path: (5kx+1) grids, (3kx+1) spectra (spdy_output_workspace)
    Workspace ens_out_grid;           // ensemble output: (5kx+1) grids per member, u | v | t | q | phi (nmem*kx each) | ps (nmem) (spdy_ens_output_workspace)
    Workspace moist_grid;             // moist physics from spectra: (3kx+1) grids t | q | phi | ln ps (spdy_moist_workspace)
    double *d_radzonal = nullptr;     // [5][il] zonal radiation forcing fsol | ozone | ozupp | zenit | stratz (spdy_radiation_set_date)
    double *d_orog = nullptr;         // phis0 (ix,il) | forog (ix,il) | sqrt(coa(j)) [il] (spdy_surface_set_orography)
    Workspace physics_ws;             // column-physics chain: (3kx+12) grids per state, max_batch states (spdy_column_physics_workspace)
    // physics from spectra of nmem states: u | v | t | q | phi (nmem*kx grids each) | ln ps (nmem), then the chain workspace of
    // (3kx+12) fields of nmem grids.  The chain's part is not scratch: it holds ssrd from one shortwave step to the next, so the
    // single state and the ensemble each keep their own (spdy_physics_workspace, spdy_ens_physics_workspace)
    Workspace physics_grid, ens_physics_grid;
    Workspace sppt_ws;                // SPPT on gridded states: the dynamics tendencies, (2kx+2) grids per state, max_batch states
                                      // (spdy_column_physics_sppt_workspace)
    Workspace sppt_grid;              // SPPT from spectra: one state's (2kx+2) grids (spdy_physics_sppt_workspace)
    // SPPT from the spectra of nmem members: (2kx+2) fields of nmem grids; grows like ens_physics_grid (spdy_ens_physics_sppt_workspace)
    Workspace ens_sppt_grid;
    int physics_fused = -1;           // column physics in one launch: -1 unset (spdy_physics_dev only), 0 never, 1 always (spdy_plan_set_option)
    int *d_kcos = nullptr;
    // device copies of dt-dependent tables
    double *d_dmp[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double *d_xd = nullptr, *d_xc = nullptr, *d_xj = nullptr, *d_tref1 = nullptr, *d_dhsx = nullptr, *d_elz = nullptr;
    double *d_xt = nullptr;                      // xdt | xct | xjt (row-major, padded copies for the one-launch spectral step)
    double *d_levtab = nullptr;       // [LEVTAB_COUNT][kx] per-level tables (DevPlan::dhs ... qcorv)
    int num_cu = 256;
    int wg_per_cu = 1;                // fused kernels: one 448-thread wave-specialised workgroup per CU
    int fused_mode = -1;              // -1 auto, 0 four-kernel path, 1 fused kernels (T30 only)
    bool ens_member_qcorh = false;    // the ensemble spectral steps read d_qcorh as (mx, nx, nmem), a field per member (spdy_plan_set_option)
    bool t63_derive = true;           // T63 model-sized inverse batches evaluate uvspec / grad on load ($SPDY_T63_NODERIVE, spdy_plan_set_option)
    // optional per-kernel timing (HIP events on the launch stream)
    bool profiling = false;
    bool capturing = false;           // between spdy_graph_begin and spdy_graph_end
    struct Span { int kind; hipEvent_t t0, t1; };
    std::vector<Span> spans;
    std::vector<spdy_graph *> graphs; // graphs captured from this plan that are still alive
    std::vector<struct spdy_comm *> comms;   // communicators created on this plan that are still alive (spdy_api_shard.hip)
    std::vector<spdy_detail::PlanObject *> objects;   // objects made on this plan that are still alive (spdy_detail::PlanObject)
};

// The surface models behind include/spdy.h's spdy_surface_model (csrc/spdy_api_surfmodel.hip).
struct spdy_surface_model final : spdy_detail::PlanObject {
    int flags = 0;
    int nmem = 1;                     // members: every field a kernel writes, and fmask_l, is held (nmem, il, ix)
    size_t ncol = 0;
    spdy::SurfaceTables tab;
    double *d_f = nullptr;            // surf_total(nmem) fields of ncol doubles (csrc/spdy_kernels.hpp: SurfField, surf_slot)
    spdy::SurfDate *d_date = nullptr;
    bool date_ready = false;          // spdy_surface_model_set_date has run
    bool started = false;             // spdy_surface_model_couple_dev(day = 0) has been issued
    void forget_device() override { d_f = nullptr; d_date = nullptr; }
};

// The SPPT patterns behind include/spdy.h's spdy_sppt (csrc/spdy_api_sppt.hip), one per member, member-major like every ensemble
// array; spdy_physics_sppt_dev and spdy_ens_physics_sppt_dev read pattern and mu.  The tables are shared by the members.
struct spdy_sppt final : spdy_detail::PlanObject {
    int nmem = 1;
    spdy::SpptTables tab;
    spdy::SpptState *d_state = nullptr;   // [nmem] each member's counter and seed
    double *d_sigma = nullptr;            // (mx, nx)
    double *d_eta = nullptr, *d_spec = nullptr;   // (mx, nx, kx, nmem) complex
    double *d_pattern = nullptr;          // (ix, il, kx, nmem)
    void forget_device() override { d_state = nullptr; d_sigma = d_eta = d_spec = d_pattern = nullptr; }
};

// The run's guard behind include/spdy.h's spdy_diagnostics (csrc/spdy_api_diagnostics.hip): one device allocation.
struct spdy_diagnostics final : spdy_detail::PlanObject {
    int capacity = 0;
    int nmem = 1;                         // members checked by one launch (spdy_ens_diagnostics_create)
    long long start_step = 0;             // the first step since create / reset: nothing before it is in the ring
    double *d_history = nullptr;          // [capacity][nmem][3][kx]
    double *d_limits = nullptr;           // reke, deke, temp low, temp high: shared by the members
    spdy::DiagLevel *d_state = nullptr;   // [nmem][kx]
    template <class V> void arrays(V &&v, size_t kx = 0)
    {
        v(d_history, (size_t)capacity * nmem * 3 * kx); v(d_limits, 4); v(d_state, (size_t)nmem * kx);
    }
    void forget_device() override { arrays(spdy_detail::Carve{}); }
};

// The ensemble analysis behind include/spdy.h's spdy_letkf (csrc/spdy_api_letkf.hip): the observation tables on the host, and
// one device allocation that holds their copies, the observation-space fields and the analysis' two workspaces.
struct spdy_letkf final : spdy_detail::PlanObject {
    int nmem = 0, max_obs = 0, nobs = 0;
    int nlv = 1;                          // levels whose eigenproblems a workgroup keeps in flight
    size_t lds = 0;                       // dynamic LDS of the transform kernel
    double sigma_h = 0.0, sigma_v = 0.0, rho = 1.0;
    bool loc_set = false;
    std::vector<double> lat;              // [il] latitudes in degrees, south first
    spdy::VLevels lv{};                   // [kx] ln fsg, as the at-pressure kernels take it as an argument
    // the tables of spdy_letkf_table of the current network, replaced as one value (spdy_letkf_set_obs, spdy_pobs_set); lnp:
    // ln(p/p0) of each observation at a pressure (0 for the others), empty after spdy_letkf_set_obs
    struct ObsTables { std::vector<int> sidx; std::vector<double> swgt, unit, lns, rinv, lnp; } obs;
    int npobs = 0;                        // how many observations of the current network are at a pressure (spdy_pobs_set)
    double *d_grid = nullptr, *d_spec = nullptr;   // (4kx+1) nmem grids u | v | t | q | ps, and as many spectra
    double *d_colunit = nullptr, *d_lnfsg = nullptr;
    double *d_swgt = nullptr, *d_ounit = nullptr, *d_olns = nullptr, *d_rinv = nullptr, *d_value = nullptr;
    double *d_err = nullptr;              // [max_obs] the errors set_obs was given, next to rinv (spdy_nature_observe_dev reads them)
    double *d_hx = nullptr, *d_hxmean = nullptr, *d_y = nullptr, *d_dep = nullptr;
    // [max_obs] each: ln(p/p0) of the at-pressure observations; 1.0 / 0.0, the observation took part in the latest analysis call;
    // the 1/error^2 that call's transform kernel read (0 where it did not) -- written by letkf_pobs_kernel only
    double *d_lnp = nullptr, *d_used = nullptr, *d_reff = nullptr;
    int *d_sidx = nullptr, *d_var = nullptr, *d_lev = nullptr;
    int *d_atp = nullptr;                 // [max_obs] 1: the observation is at a pressure (its d_lev is 0); written by spdy_pobs_set only
    // the member mask (include/spdy.h, "member mask"): d_nused = {nmem, n of the latest masked call} as doubles -- an unmasked call
    // launches what it always did and writes neither, so "members_used" is the word of the kind of call enqueued last (masked_last);
    // d_umap [LETKF_UMAP] is the table a masked call's first launch builds from the caller's d_use (csrc/spdy_kernels.hpp)
    double *d_nused = nullptr;
    int *d_umap = nullptr;
    bool masked_last = false;
    // the main allocation: the doubles, then the ints; ncol, ns: elements of a grid and of a spectrum
    template <class V> void arrays(V &&v, size_t ncol = 0, size_t ns = 0, size_t kx = 0)
    {
        const size_t nf = (4 * kx + 1) * nmem, M = max_obs > 0 ? max_obs : 1, E = nmem;
        v(d_grid, nf * ncol); v(d_spec, nf * ns); v(d_colunit, 3 * ncol); v(d_lnfsg, kx);
        v(d_swgt, 4 * M); v(d_ounit, 3 * M); v(d_olns, M); v(d_rinv, M); v(d_err, M); v(d_value, M);
        v(d_hx, M * E); v(d_hxmean, M); v(d_y, M * E); v(d_dep, M);
        v(d_lnp, M); v(d_used, M); v(d_reff, M); v(d_nused, 2); v(d_infl, (4 * kx + 1) * ncol);
        v(d_slot_ps, M * E); v(d_slot_out, M * E);
        v(d_sidx, 4 * M); v(d_var, M); v(d_lev, M); v(d_atp, M); v(d_umap, spdy::LETKF_UMAP);
    }
    // observations in time slots (include/spdy.h, "observations in time slots"; spdy_slot_set): the ranges first[0 .. nslots] of the
    // current network, nslots == 0: none, and whether a slot has been observed since they were set -- host side, read when a call is
    // enqueued.  d_slot_ps, d_slot_out [max_obs][nmem], part of the main allocation: the stencil's ps_e and the out-of-column flag
    // (1.0 / 0.0) of every member at the slot's time, written next to d_hx by an observe of an at-pressure network
    int nslots = 0;
    int slot_first[SPDY_MAX_SLOTS + 1] = {0};
    bool slot_observed[SPDY_MAX_SLOTS] = {false};
    double *d_slot_ps = nullptr, *d_slot_out = nullptr;
    // weight interpolation (spdy_letkf_set_weight_stride); at stride (1, 1) the tables are empty and nothing is allocated
    int si = 1, sj = 1;
    // coarse [ncoarse] grid columns, ascending; iidx [ncol][4] entries of that list; iwgt [ncol][4]
    struct InterpTables { std::vector<int> coarse, iidx; std::vector<double> iwgt; } interp;
    double *d_tw = nullptr, *d_iwgt = nullptr;     // [ncoarse][kx][nmem][nmem]; [ncol][4]
    int *d_iidx = nullptr, *d_coarse = nullptr;
    template <class V> void interp_arrays(V &&v, size_t ncoarse = 0, size_t ncol = 0, size_t kx = 0)
    {
        v(d_tw, ncoarse * kx * nmem * nmem); v(d_iwgt, 4 * ncol); v(d_iidx, 4 * ncol); v(d_coarse, ncoarse);
    }
    // relaxation (spdy_relax_set): read when an analysis is enqueued; both 0: the analysis launches what it always did.
    // d_infl [(4 kx + 1)][ncol], the factor f of the latest relaxed call, is part of the main allocation.  d_raw, (4 kx + 1) nmem
    // grids in d_grid's layout, takes the raw increments of a relaxed call: an allocation of its own, made when relaxation is first
    // switched on and kept from then on (a captured graph may point into it)
    double rtpp = 0.0, rtps = 0.0;
    double *d_infl = nullptr, *d_raw = nullptr;
    template <class V> void relax_arrays(V &&v, size_t ncol = 0, size_t kx = 0) { v(d_raw, (4 * kx + 1) * nmem * ncol); }
    // the background check and the observation statistics (spdy_qc_set, spdy_qc_set_slot): read when a call is enqueued.  gross 0
    // and no grouping: off, the analysis launches what it always did.  qc_group: the caller's group of every observation of the
    // current network, empty: the default, the observation's variable (qc_ngroups is then LETKF_VARS); set_obs and pobs_set
    // return it to the default.  qc_analysed: an analysis call with the check on has been enqueued for the current network, so
    // the kept record and departure are its.  The qc block is an allocation of its own, made by the first setting that turns
    // anything on and kept from then on (a captured graph may point into it): d_qc_stats [SPDY_QC_SLOTS][SPDY_QC_MAX_GROUPS][10],
    // d_qc_check, d_qc_depb [max_obs] the record (0.0 passed, 1.0 rejected, 2.0 out of column) and the departure of the latest
    // checked analysis, d_qc_group [max_obs] the uploaded grouping
    double gross = 0.0;
    int qc_ngroups = spdy::LETKF_VARS, qc_slot = 0;
    std::vector<int> qc_group;
    bool qc_analysed = false;
    double *d_qc_stats = nullptr, *d_qc_check = nullptr, *d_qc_depb = nullptr;
    int *d_qc_group = nullptr;
    bool qc_on() const { return gross != 0.0 || !qc_group.empty(); }
    template <class V> void qc_arrays(V &&v, size_t M = 0)
    {
        v(d_qc_stats, M ? (size_t)SPDY_QC_SLOTS * SPDY_QC_MAX_GROUPS * spdy::QC_STATS : 0); v(d_qc_check, M); v(d_qc_depb, M);
        v(d_qc_group, M);
    }
    // adaptive inflation (spdy_infl_set, spdy_infl_fill): read when an analysis is enqueued; off: the analysis launches what it
    // always did and the scalar rho above is the transform's.  The block is an allocation of its own, made by the first "on" (or
    // by asking spdy_letkf_field for one of its names) and kept from then on (a captured graph may point into it): d_rho [kx][ncol]
    // the field, filled with the scalar rho of that moment; d_infl_parm [3][kx][ncol] p1, p2, p3 of the latest call; d_obs_s2 [max_obs]
    bool infl_on = false;
    double infl_sigma_b = 0.0, infl_min = 0.0, infl_max = 0.0;
    double *d_rho = nullptr, *d_infl_parm = nullptr, *d_obs_s2 = nullptr;
    template <class V> void infl_arrays(V &&v, size_t ncol = 0, size_t kx = 0, size_t M = 0)
    {
        v(d_rho, kx * ncol); v(d_infl_parm, 3 * kx * ncol); v(d_obs_s2, M);
    }
    void forget_device() override
    {
        arrays(spdy_detail::Carve{}); interp_arrays(spdy_detail::Carve{}); relax_arrays(spdy_detail::Carve{});
        qc_arrays(spdy_detail::Carve{}); infl_arrays(spdy_detail::Carve{});
    }
};

// The nature run behind include/spdy.h's spdy_nature (csrc/spdy_api_nature.hip): one device allocation.
struct spdy_nature final : spdy_detail::PlanObject {
    int capacity = 0;
    double *d_truth = nullptr;            // (4 kx + 1) grids u | v | t | q (kx each) | ps
    double *d_zero = nullptr;             // (4 kx + 1) zero spectra: what create's first transform reads
    double *d_part = nullptr;             // [4 kx + 1][il][3] zonal sums of a verify call
    double *d_gw = nullptr;               // [il] Gaussian weights / their sum, south first
    double *d_scores = nullptr;           // [capacity][3][4 kx + 1]
    unsigned long long *d_state = nullptr;   // {seed, draws}
    template <class V> void arrays(V &&v, size_t nf = 0, size_t ncol = 0, size_t ns = 0, size_t il = 0)
    {
        v(d_truth, nf * ncol); v(d_zero, nf * ns); v(d_part, nf * il * 3); v(d_gw, il); v(d_scores, (size_t)capacity * 3 * nf);
        v(d_state, 2);
    }
    void forget_device() override { arrays(spdy_detail::Carve{}); }
};

namespace spdy_detail {

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int dev_alloc(spdy_plan *p, size_t bytes, void **out);
// gives a dev_alloc'ed buffer back before the plan goes: the plan's stream is synchronised first (queued work may still use it).
// Null is fine; a buffer that cannot be released now (an open capture) stays with the plan.
int dev_release(spdy_plan *p, void *ptr);
template <class T> int dev_alloc(spdy_plan *p, size_t bytes, T **out)
{
    void *ptr = nullptr;
    const int rc = dev_alloc(p, bytes, &ptr);
    *out = static_cast<T *>(ptr);
    return rc;
}
// One dev_alloc for the arrays that walk(visitor) visits, handed out in the walk's order; refused (SPDY_ERR_ARG) if an array
// would start off its element's alignment.  *bytes: the allocation's size (for the caller's memset).
template <class Walk> int dev_carve(spdy_plan *p, Walk &&walk, size_t *bytes = nullptr)
{
    Carve sum;
    walk(sum);
    if (!sum.aligned) return fail(SPDY_ERR_ARG, "dev_carve: an array of the allocation would be misaligned");
    char *base = nullptr;
    const int rc = dev_alloc(p, sum.bytes, &base);
    if (!rc) walk(Carve{base});
    if (bytes) *bytes = sum.bytes;
    return rc;
}
// w holds at least `doubles` doubles afterwards: NEED_DEVICE, nothing to do if it is large enough, NOT_CAPTURING(p, what),
// [ensure_four], dev_alloc (see spdy_plan::Workspace for what becomes of a smaller earlier one)
int ensure_workspace(spdy_plan *p, Workspace *w, size_t doubles, const char *what, bool with_four = false);
// one copy on the plan's stream and its synchronisation: the caller's host array is free (upload) or filled (download) on return.
// Stream-ordered: work enqueued, or a graph replayed, before the call sees the old contents, work after it the new ones.
int upload_sync(spdy_plan *p, void *dst, const void *src, size_t bytes);
int download_sync(spdy_plan *p, void *dst, const void *src, size_t bytes);
// An object joins its plan where it is `new`ed, on a host-only plan too and before anything can fail.  Its _destroy calls retire
// with the device buffers it owns and then deletes the handle: a live object leaves the plan's list and gives the buffers back
// (dev_release), a dead one has nothing left to give.
inline void adopt(spdy_plan *p, PlanObject *o) { o->plan = p; p->objects.push_back(o); }
void retire(PlanObject *o, std::initializer_list<void *> buffers);
int check_batch(const spdy_plan *p, int nb);
int stream_sync(spdy_plan *p);        // hipStreamSynchronize of the plan's stream; refused while a capture is open
// One host-pointer call, from its argument checks to its return: open, in..., the _dev form on the call's four staging buffers
// c[0..3], out..., finish.  The call's route is chosen once, by open, and is the call's own; so is the list of what finish has
// to copy out.  A call that returns early (a failed step) copies nothing anywhere and leaves nothing behind for the next one.
//
// The two routes.  Device: the buffers are device memory (spdy_plan::dstage), in and out are hipMemcpyAsync on the plan's stream
// and finish is its synchronisation.  Host-mapped, for small calls (the reference's one-field-per-call pattern, level stacks):
// the buffers are PINNED HOST memory mapped into the device's address space (spdy_plan::hstage) and both PCIe copy engines are
// skipped -- in is a memcpy by the calling thread, the kernels read and write the buffers across the link themselves, out is
// remembered, and finish waits (a spin on a host-mapped completion stamp, see there) and then memcpy's the results out.
// $SPDY_HOST_STAGE_KB (default 512; 0 = off), read when the plan allocates its staging, is the largest per-buffer size that
// takes the host-mapped route.
//
// open(elems): elems is the largest array, in doubles, that the call puts into ONE buffer; the call is host-mapped when that
// fits, on the device set otherwise -- and always without a stated size.  Who states what:
//   nb grids      spdy_spec_to_grid[_batch], spdy_grid_to_spec[_batch], spdy_uvspec_to_grid, spdy_grad_to_grid, spdy_vdspec
//   nb spectra    spdy_laplacian, spdy_inverse_laplacian, spdy_trunct, spdy_grad, spdy_vds, spdy_uvspec
//   no size       spdy_legendre_inv, spdy_legendre_dir, spdy_fourier_inv, spdy_fourier_dir (their other operand is the Fourier
//                 workspace, device memory), spdy_hdiff, spdy_implicit_terms, spdy_geopotential, spdy_step_field
struct HostCall {
    explicit HostCall(spdy_plan *plan) : p(plan) {}
    HostCall(const HostCall &) = delete;
    HostCall &operator=(const HostCall &) = delete;
    // SPDY_ERR_STATE inside a capture; allocates the plan's staging at its first use; chooses the route
    int open(size_t elems = (size_t)-1);
    double *operator[](int slot) const { return buf[slot]; }
    bool on_host_stage() const { return host; }
    int in(int slot, const double *src, size_t n, size_t offset = 0);   // n doubles of the caller's into buf[slot] + offset
    int out(double *dst, int slot, size_t n);                           // n doubles of buf[slot] into the caller's, by finish at the latest
    int finish();                                                       // on return the caller's output arrays are filled
private:
    spdy_plan *p;
    double *buf[4] = {nullptr, nullptr, nullptr, nullptr};
    bool host = false;
    struct Out { double *dst; const double *src; size_t bytes; } outs[3];   // host-mapped route: at most three (spdy_implicit_terms)
    int nouts = 0;
};
int ensure_four(spdy_plan *p);        // four-kernel path workspace
// T63 fused path: the direct batch WITHOUT vds -- the scaled (u, v) grids' spectra go to raw_u / raw_v (null: p->tmp_c /
// p->tmp_d), the plain grids' to spec (spdy_direct_batch_spectral_step_dev, the level-sharded step)
int direct_batch_raw63(spdy_plan *p, int npairs, const double *ug, const double *vg, int kcos, int nplain, const double *grid, double *spec,
                       double *raw_u = nullptr, double *raw_v = nullptr);
bool use_raw63(const spdy_plan *p, int npairs);   // whether a step's direct batch of npairs (u, v) pairs takes that route
// the plain spectra of nseg segments (kcos 1) -> ONE grid stack, as one launch of the fused inverse kernels (spdy_moist_physics_dev)
int inverse_plain_one(spdy_plan *p, int nseg, const spdy_spec_seg *segs, double *grid);
// time level 1 of nmem members (vor, div, t, q [nmem][kx] spectra, ps [nmem], read in place) to the grid stack g = u | v | t | q |
// ps: one inverse batch, nmem * kx pairs as true wind next to the segments t | q | ps (spdy_api_letkf.hip; the nature run's too)
int ens_to_grid(spdy_plan *p, int nmem, const double *vor, const double *div, const double *t, const double *q, const double *ps, double *g);
int upload_level_tables(spdy_plan *p);
void release_comms(spdy_plan *p);     // plan teardown: RCCL communicators of this plan are shut down, their handles stay valid but dead

inline size_t spec_elems(const spdy_plan *p) { return (size_t)2 * p->tab.mx * p->tab.nx; }
inline size_t grid_elems(const spdy_plan *p) { return (size_t)p->tab.ix * p->tab.il; }
inline size_t four_elems(const spdy_plan *p) { return (size_t)2 * p->tab.mx * p->tab.il; }

}  // namespace spdy_detail

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return spdy_detail::fail(SPDY_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

#define NEED_PLAN(p)                                                                   \
    do {                                                                               \
        if (!(p)) return spdy_detail::fail(SPDY_ERR_ARG, "null plan");                 \
    } while (0)
#define NEED_DEVICE(p)                                                                                       \
    do {                                                                                                     \
        NEED_PLAN(p);                                                                                        \
        if ((p)->device < 0) return spdy_detail::fail(SPDY_ERR_NO_DEVICE, "host-only plan: no HIP device, no CPU fallback"); \
        HIP_TRY(hipSetDevice((p)->device));                                                                  \
    } while (0)
// the first check of every call on an object made on a plan but _destroy (spdy_detail::PlanObject)
#define NEED_LIVE(x, what)                                                                                   \
    do {                                                                                                     \
        if (!(x)) return spdy_detail::fail(SPDY_ERR_ARG, "null %s", what);                                   \
        if (!(x)->plan) return spdy_detail::fail(SPDY_ERR_STATE, "the plan this %s was made on has been destroyed", what); \
    } while (0)
#define NOT_CAPTURING(p, what)                                                                               \
    do {                                                                                                     \
        if ((p)->capturing) return spdy_detail::fail(SPDY_ERR_STATE, "%s is not possible while a graph capture is open", what); \
    } while (0)
#define RC(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)
#define KERNEL(expr) HIP_TRY(expr)
