// Launch interface between the C-ABI layer (spdy_api.hip) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "spdy_vinterp.hpp"

namespace spdy {

// Launch-policy switches of a plan (host-side use: which kernel form a launcher picks; none changes results beyond the
// rounding-level path choices documented in include/spdy.h).  Read from the environment ONCE, at plan creation
// (spdy_plan_create), and changed per plan with spdy_plan_set_option -- no launcher calls getenv.
struct LaunchOpts {
    int t30_nopart = 0;     // small T30 inverse launches walk whole tiles              ($SPDY_T30_NOPART,  "t30_part" = 0)
    int t30_nosplit = 0;    // small T30 direct launches as whole tiles                 ($SPDY_T30_NOSPLIT, "t30_split" = 0)
    int t63_nosplit = 0;    // one workgroup per pair in small fused T63 direct launches ($SPDY_T63_NOSPLIT, "t63_split" = 0)
    int t63_nostage = 0;    // small T63 direct batches fused instead of staged         ($SPDY_T63_NOSTAGE, "t63_stage" = 0)
    int t63_np2_from = 40;  // pairs from which the staged contraction takes two pairs per workgroup ($SPDY_T63_NP2_FROM)
    int wt_min_mb = 6;      // output MB from which a model-sized launch writes through ($SPDY_WT_MIN_MB; 0 = never)
};

// Device-side view of a plan: dimensions + table pointers (all device memory).
struct DevPlan {
    int trunc, ix, iy, il, kx, nx, mx;
    int num_cu;    // compute units of the plan's device (sizes the persistent launches; host-side use)
    int fs;        // row stride (doubles) of the Fourier workspace: 2*mx rounded up to 16
    int ks_inv;    // k-steps (of 4 n's) per parity in the inverse-Legendre A table
    int jt;        // 16-latitude tiles per hemisphere (ceil(iy/16))
    int nt_dir;    // 16-row n tiles per parity in the direct-Legendre A table
    int js_dir;    // k-steps (of 4 latitudes) in the direct transform (iy/4)
    const double *pa_inv;   // [mx][2][ks_inv][jt][64]      P(m,n,j)            MFMA A fragments
    const double *pa_dir;   // [mx][2][nt_dir][js_dir][64]  P(m,n,j)*wt(j)      MFMA A fragments
    // 4x4x4-block fragments with both parities packed (fused T30 kernels; nullptr otherwise):
    const double *pa_inv2;  // [mx][ks_inv][64]  blocks 0,1: latitudes 16..23 of even n; blocks 2,3: of odd n
    const double *pa_dir2;  // [mx][js_dir][64]  blocks 0,1: n rows 0..7 of even n; blocks 2,3: of odd n
    // the same fragments in the order the fused T30 kernels keep them in registers, two per 16-byte load:
    const double *img_s2g;  // [4 Legendre waves][30][64 lanes][2]
    const double *img_g2s;  // [4 Legendre waves][36][64 lanes][2]
    // the inverse kernel's small-batch form (work items = (tile, third of the latitudes)): per part the packed fragments of
    // latitudes 8 part .. 8 part + 7 (blocks 0, 1: even n, blocks 2, 3: odd n), in slot order
    const double *img_s2g3; // [3 parts][4 Legendre waves][10][64 lanes][2]
    // A-operand images of the fused T63 kernels: [4 Legendre waves][38 slots][6 chunks][64 lanes][2] (spdy_t63_sched.hpp)
    const double *img_g2s63, *img_s2g63;
    // row workspace of the staged form of small T63 direct batches: [pair][chunk][field][16 rows][128] Fourier rows
    double *rows_ws;
    int rows_ws_fields;     // capacity in fields (0: none -- the fused split form runs instead)
    const double *cosgr;    // [il]
    const double *cosgr2;   // [il]
    // spectral operator tables, each [nx][mx] (gradx: [mx])
    const double *el2, *elm2, *trfilt, *gradx, *gradym, *gradyp, *uvdx, *uvdym, *uvdyp, *vddym, *vddyp;
    const double *gradx_e;  // gradx expanded to [nx][mx] (gradient tiles of the mixed inverse kernel index it like uvdx)
    // implicit tables
    const double *xd, *xc, *xj, *tref1, *dhsx, *elz;
    // the same matrices row-major with rows padded to kxp = kx rounded up to even (16-byte rows): xdt, xct [kx][kxp],
    // xjt [mx+nx+1][kx][kxp] -- a thread's mat-vec row is one contiguous run instead of kx strided elements
    const double *xdt, *xct, *xjt;
    int kxp;
    // per-level tables [kx]: sigma-level functions (geometry.f90:51-60, geopotential.f90:22-30,53,
    // horizontal_diffusion.f90:70-82) and the reference temperature profile (implicit.f90:62-67);
    // rgtref = rgas*tref.  tref* are filled by spdy_implicit_init, the others whenever sigma levels exist.
    const double *dhs, *dhsr, *fsgr, *tref, *tref2, *tref3, *rgtref, *xgeop1, *xgeop2, *corf, *tcorv, *qcorv;
    const double *dmp_t[6]; // dmp, dmpd, dmps, dmp1, dmp1d, dmp1s [nx][mx] (dmp1* valid after spdy_implicit_init)
    const double *coriol;   // [il] 2*omega*sin(lat) (geometry.f90:89), southernmost row first
    double rgas, akap;      // physical_constants.f90:22-24 (float32 literals widened)
    LaunchOpts lo;          // (host-side use, like num_cu)
};
constexpr int LEVTAB_COUNT = 12;   // number of per-level tables above (one device allocation of LEVTAB_COUNT*kx doubles)

// FFTPACK twiddles / constants for one resolution; copied to __constant__ memory once.
struct FftConstants {
    double first[144];  // stage with ido=48: 1 block (N=96, radix 2) or 3 blocks (N=192, radix 4)
    double a[36];       // radix-4 stage, ido=12: 3 blocks of 12
    double b[9];        // radix-4 stage, ido=3 : 3 blocks of 3
    double taui, sqrt2, hsqt2, scale;
};
hipError_t upload_fft_constants(int ix, const FftConstants &c);

// four: [nb][il][fs] workspace layout.  All launches are asynchronous on `s`.
hipError_t launch_legendre_inv(const DevPlan &p, int nb, const double *spec, double *four, hipStream_t s);
hipError_t launch_legendre_dir(const DevPlan &p, int nb, const double *four, double *spec, hipStream_t s);
hipError_t launch_fourier_inv(const DevPlan &p, int nb, const double *four, const int *d_kcos, int kcos_all,
                              double *grid, hipStream_t s);
// gscale: nullptr, or a per-latitude factor applied to the grid on load (vdspec's cosgr/cosgr2)
hipError_t launch_fourier_dir(const DevPlan &p, int nb, const double *grid, const double *gscale, double *four,
                              hipStream_t s);

// Fused persistent T30 kernels (whole transform in one pass through LDS; at most max_wg workgroups)
// One inverse launch.  mode 0: plain -- nb fields spec -> grid, kcos per field (d_kcos) or kcos_all.  mode 1: uvspec fused -- tile
// i = (vor[i], div[i]) = (spec, spec2) -> (ug, vg) = (grid, grid2).  mode 2: grad fused -- tile i = psi[i] = spec -> (d/dx, d/dy) =
// (grid, grid2).  In modes 1/2 nb counts tiles and kcos_all applies to both outputs.
// mode 3: a model step's whole inverse batch -- nb (vor, div) pairs as in mode 1, plain fields from up to four source arrays
// (plain[i] holds nplain[i] of them; their grids are ONE stack grid_p) with their own kcos (kcos_p per field, or kcos_all_p), and
// ngrad gradient tiles psi[i] -> gx[i], gy[i] that ride along as uvspec tiles with vor = `zero` and the grad tables
struct S2gFused {
    int mode = 0, nb = 0;
    const double *spec = nullptr, *spec2 = nullptr;
    const int *d_kcos = nullptr;
    int kcos_all = 1;
    double *grid = nullptr, *grid2 = nullptr;
    const double *plain[4] = {nullptr, nullptr, nullptr, nullptr};
    int nplain[4] = {0, 0, 0, 0};
    const int *kcos_p = nullptr;
    int kcos_all_p = 1;
    double *grid_p = nullptr;
    int ngrad = 0, kcos_grad = 2;
    const double *psi = nullptr;
    double *gx = nullptr, *gy = nullptr;
    const double *zero = nullptr;
};
hipError_t launch_s2g_fused(const DevPlan &p, const S2gFused &r, int max_wg, hipStream_t s);
// One direct launch: nb fields grid -> spec, gscale (nullptr or a per-latitude factor) applied on load.
// grid2 / spec2 non-null: vdspec in one pass -- tile i is the pair (grid[i], grid2[i]) scaled by gscale, the outputs are vds of the
// pair's spectra: vorticity -> spec, divergence -> spec2 (nb pairs).
// nplain > 0: a model step's whole direct batch in one launch -- nb (u,v) pairs as above plus nplain ordinary fields grid_p -> spec_p
// (unscaled).
// allow_split = false: never the three-workgroups-per-tile form -- its workgroups read every tile three times, which is the wrong
// trade when the rows are host-mapped staging memory read across the link
struct G2sFused {
    int nb = 0;
    const double *grid = nullptr, *gscale = nullptr;
    double *spec = nullptr;
    const double *grid2 = nullptr;
    double *spec2 = nullptr;
    int nplain = 0;
    const double *grid_p = nullptr;
    double *spec_p = nullptr;
    bool allow_split = true;
};
hipError_t launch_g2s_fused(const DevPlan &p, const G2sFused &r, int max_wg, hipStream_t s);

// SIMD of each of the eight waves of nwg workgroups shaped like the fused T63 kernels' (d_out: 8 ints per workgroup)
hipError_t launch_wave_placement(int *d_out, int nwg, hipStream_t s);
// Fused T63 kernels: a pair of fields per tile, six latitude chunks, accumulators / B operands resident in VGPRs
hipError_t launch_s2g_fused_t63(const DevPlan &p, int nb, const double *spec, const int *d_kcos, int kcos_all, double *grid, int max_wg,
                                hipStream_t s);
// One fused T63 launch over up to six independent sub-batches (own arrays, own scale / kcos policy); pair0 and npairs are
// filled in by the launcher
constexpr int T63_MAX_SEG = 8;
struct T63Seg {
    const double *src;
    double *dst;
    const double *scale;   // direct: per-latitude factor applied on load, or nullptr
    const int *kcos;       // inverse: per-field kcos (device), or nullptr for kcos_all
    int nb, kcos_all, pair0;
    int op;                // inverse: 0 = src holds the spectra; T63_OP_* = they are derived from src / (const double *)scale on load
                           // direct: T63_OP_VDS = vdspec pairs -- pair i of the segment is (src[i], T63Batch::vds_src2[i]) = (u, v) grids,
                           // nb pairs; the contraction applies vds (spectral.f90:146-171) to the pair's spectra in registers:
                           // vorticity -> dst[i], divergence -> T63Batch::vds_dst2[i]
};
// spectral operators folded into the inverse kernel's operand load (spectral.f90:124-196): the segment's spectra are
//   U / V of uvspec(vor = src, div = scale)  or  d/dlambda / d/dmu of grad(psi = src)
enum { T63_OP_NONE = 0, T63_OP_U = 1, T63_OP_V = 2, T63_OP_GX = 3, T63_OP_GY = 4, T63_OP_VDS = 5 };
struct T63Batch {
    int nseg, npairs;
    int by_chunk, wt;      // inverse, small batches: work items are (pair, chunk) instead of whole pairs; model-sized launches with
                           // several MB of output: stores written through (both set by the launcher)
    int nop_items, ipw;    // by-chunk walk (set by the launcher): items of the derived segments (one per workgroup), items per
                           // workgroup behind them
    const double *vds_src2; // direct launches: the second arrays of the (one) T63_OP_VDS segment -- in the header, not in the
    double *vds_dst2;       // segment, whose size decides whether the compiler indexes the by-value argument or copies it to scratch
    T63Seg seg[T63_MAX_SEG];
};
hipError_t launch_s2g_fused_t63_batch(const DevPlan &p, T63Batch b, int max_wg, hipStream_t s);
// whether an inverse launch of `pairs` field pairs may carry its derived ones (model-sized launches: the by-chunk form) --
// lead_op_pairs of U / V (or of the gradient, when it is the only operator), op_pairs of all operators together
bool s2g_t63_derives(int max_wg, int pairs, int lead_op_pairs, int op_pairs);
hipError_t launch_g2s_fused_t63_batch(const DevPlan &p, T63Batch b, int max_wg, hipStream_t s);
// whether a direct launch of `pairs` field pairs takes the STAGED form (rows launch + contraction launch: model-sized batches) --
// the form that can apply vds to T63_OP_VDS segments (callers otherwise run vds as a kernel behind the launch)
bool g2s_t63_staged(const DevPlan &p, int max_wg, int pairs);
hipError_t launch_g2s_fused_t63(const DevPlan &p, int nb, const double *grid, const double *gscale, double *spec, int max_wg, hipStream_t s);

enum SpecOp { OP_LAPLACIAN = 0, OP_INV_LAPLACIAN = 1, OP_TRUNCT = 2 };
hipError_t launch_scale_op(const DevPlan &p, int op, int nb, const double *in, double *out, hipStream_t s);
hipError_t launch_grad(const DevPlan &p, int nb, const double *psi, double *psdx, double *psdy, hipStream_t s);
hipError_t launch_vds(const DevPlan &p, int nb, const double *u, const double *v, double *vor, double *div, hipStream_t s);
hipError_t launch_uvspec(const DevPlan &p, int nb, const double *vor, const double *div, double *u, double *v, hipStream_t s);
hipError_t launch_uvspec_grad(const DevPlan &p, int nuv, const double *vor, const double *div, double *u, double *v, int ngr,
                              const double *psi, double *psdx, double *psdy, hipStream_t s);
hipError_t launch_hdiff(const DevPlan &p, int nlev, const double *field, const double *fdt, const double *dmp,
                        const double *dmp1, double *out, hipStream_t s);
struct HdiffOps {   // up to 8 independent diffusion operations, passed by value as one kernel argument
    int nops, nlev[8];
    const double *field[8], *fdt[8], *dmp[8], *dmp1[8];
    double *out[8];
};
hipError_t launch_hdiff_multi(const DevPlan &p, const HdiffOps &ops, hipStream_t s);
hipError_t launch_implicit(const DevPlan &p, double *divdt, double *tdt, double *psdt, hipStream_t s);

// ---- spectral side of a time step (spdy_step.hip) ----
// step_field_2d/3d (time_stepping.f90:121-167): up to 8 prognostic arrays [2][nlev][nx][mx] + their tendencies in one launch
struct StepOps {
    int nops, nlev[8];
    double *field[8], *fdt[8];
};
hipError_t launch_step_fields(const DevPlan &p, const StepOps &ops, int j1, double dt, double eps, double wil, int do_trunct,
                              hipStream_t s);
// the diffusion block of `step` (time_stepping.f90:62-96) incl. the orographic corrections and the stratospheric drag
struct HdiffStep {
    const double *vor, *div, *t, *tr;            // time level 1 of the prognostics, [kx][nx][mx] complex
    double *vordt, *divdt, *tdt, *trdt;          // tendencies, in place
    const double *tcorh, *qcorh;                 // [nx][mx] complex (horizontal_diffusion.f90:31-32)
    const double *dmp, *dmpd, *dmps, *dmp1, *dmp1d, *dmp1s;
    double sdrag;
};
hipError_t launch_hdiff_step(const DevPlan &p, const HdiffStep &h, hipStream_t s);
// get_geopotential (geopotential.f90:33-57) of nmem members: t, phi [nmem][kx], phis shared
hipError_t launch_geopotential(const DevPlan &p, int nmem, const double *t, const double *phis, double *phi, hipStream_t s);
// get_spectral_tendencies (tendencies.f90:242-293); phi is written as the reference's module variable is
hipError_t launch_spectral_tendencies(const DevPlan &p, const double *div, const double *t, const double *ps, const double *phis,
                                      double *divdt, double *tdt, double *psdt, double *phi, hipStream_t s);
// Level-block layout of a level-sharded step (spdy_api_shard.hip).  Rank r of R owns the levels [kx r / R, kx (r + 1) / R)
// = [lo_r, hi_r), nl_r of them.  A stack of F fields x kx levels that the ranks fill and exchange is stored block by block,
// block r = the rank's own contiguous launch operands [F][nl_r] (+ X level-free fields behind them): its slab offset is
// F lo_r + X r, and field f of level k lives at slab  F lo_r + X r + f nl_r + (k - lo_r)  of the owner r of k.  So ONE
// contiguous block per rank travels in the exchange and every transform launch reads/writes plain contiguous stacks; only
// the column kernels (grid tendencies, spectral step) index through the blocks.  nranks = 0: not sharded (the plain [F][kx]
// stacks of separate pointers); with one rank the block layout coincides with the plain one.
struct LevelShard { int nranks, rank; };
// grid-space dynamical tendencies (tendencies.f90:105-197) and their spectral-space combination (:125-126, 218-233)
struct GridTend {
    const double *ug, *vg, *tg, *vorg, *divg, *trg;   // [kx] grids each (vorg WITHOUT the Coriolis term)
    const double *px, *py;                            // grad(ps) on the grid
    double *u, *v, *plain;                            // [3 kx], [3 kx], [3 kx + 1] grids: operands of the direct batch
    // sh.nranks >= 1: the six inputs are ONE level-block stack `ug` (F = 6, X = 0, field order ug, vg, vorg, divg, tg, trg:
    // the other five pointers are ignored) holding all levels; the outputs are this rank's own launch operands only --
    // u, v [3 nl], plain [3 nl + 1] with nl = the rank's level count (every rank gets the level-free last field)
    LevelShard sh;
    // TRANSPOSED form of the level-sharded step (sh.nranks >= 1 and tr_out non-null): this rank holds ALL levels of the points
    // [pt0, pt0 + npts) only.  `ug` is the F = 6 level-block stack with slabs of npts doubles (local point index); px, py stay
    // whole grids (every rank computes them itself) and are read at pt0 + i; the outputs of ALL levels go to tr_out, an F = 9,
    // X = 1 level-block stack with slabs of npts doubles -- block q = rank q's direct-batch operands u [3 nl_q] | v [3 nl_q] |
    // plain [3 nl_q] | the level-free field, restricted to these points (u, v, plain are ignored).
    int npts, pt0;
    double *tr_out;
    // Ensemble form (nmem >= 1 members, blockIdx.y; not with sh): every level dimension above is nmem*kx, member-major -- the
    // inputs (nmem, kx) grids each, px, py (nmem), the outputs group-major [3][nmem][kx] (+ the nmem level-free fields behind
    // plain's groups).  Member e works on level slot e*kx + k with group stride nmem*kx; nmem = 1 is the layout above.
    int nmem;
};
hipError_t launch_grid_tendencies(const DevPlan &p, const GridTend &g, hipStream_t s);
// Whether a fused launch with this many grid-side bytes streams them (non-temporal loads / stores; >= 16 MB): the size from which
// a launch is throughput-bound rather than latency-bound
bool streams(long grid_bytes);
// Write-through policy of a model-sized launch (the step's kernels): outputs of at least p.lo.wt_min_mb MB (default 6; 0 = never)
// leave the L2s as they are produced instead of waiting, dirty, for the end-of-kernel release.
bool write_through_policy(const DevPlan &p, long output_bytes);
hipError_t launch_tendency_combine(const DevPlan &p, double *pdiv, double *pspec, hipStream_t s);
// the whole spectral-space tail of a step in one launch (kx <= 16)
struct SpecStep {
    double *pvor, *pdiv, *pspec;                 // direct-batch outputs [3kx], [3kx], [3kx+1]; tendencies are left in them
    double *vor, *div, *t, *tr, *ps;             // prognostics, both time levels ([2][kx] / [2])
    const double *phis, *tcorh, *qcorh;
    double *phi;
    double sdrag, dt, eps, wil;
    int j1, do_trunct;
    // non-null: the vdspec pairs' spectra have NOT been through vds yet -- raw_u, raw_v [3kx] are grid_to_spec of the scaled
    // (u, v) grids and the kernel applies vds (spectral.f90:146-171) where it reads them (pvor / pdiv are outputs only)
    const double *raw_u, *raw_v;
    // sh.nranks >= 1: the direct batches' outputs of all ranks are ONE level-block stack `pvor` (F = 9: the rank's pvor | pdiv
    // | pspec stacks of 3 nl each, X = 1: its copy of the level-free psdt; pdiv / pspec / raw_u / raw_v are then only flags:
    // raw_u non-null = the first six groups are the raw pairs' spectra) and the final tendencies go to tend_out
    // [vordt | divdt | tdt | trdt] (kx each) | psdt in the plain layout instead of back into the operands
    LevelShard sh;
    double *tend_out;
    // TRANSPOSED form (sh.nranks >= 1 and ne > 0): this rank holds ALL levels of the coefficients [e0, e0 + ne) only (e0 a
    // multiple of the kernel's 16-coefficient blocks).  The level-block stack `pvor` has slabs of ne complex values (local
    // coefficient index); the prognostics, phi and tend_out are the whole arrays as ever and are read / written at these
    // coefficients only.  No raw pairs (vds needs the neighbouring rows): raw_u must be null.
    int e0, ne;
    // Ensemble form (nmem >= 1 members, blockIdx.y; not with sh): prognostics [2][nmem][kx] / ps [2][nmem], phi [nmem][kx],
    // pvor / pdiv / pspec / raw_u / raw_v group-major [3][nmem][kx] (+ the nmem level-free fields behind pspec's groups); phis,
    // tcorh, qcorh are shared.  nmem = 1 is the layout above.
    int nmem;
    // non-zero: qcorh is (mx, nx, nmem), member e's own field (the plan option "ens_member_qcorh"); tcorh stays shared
    int member_qcorh;
};
hipError_t launch_spectral_step(const DevPlan &p, const SpecStep &a, hipStream_t s);
// output path (input_output.f90:184-206)
struct GatherOps { int nops, nfld[8]; const double *src[8]; double *dst[8]; };
hipError_t launch_gather_spectra(const DevPlan &p, const GatherOps &g, hipStream_t s);
struct OutputCast { int nops, nfld[8], kind[8]; double factor[8]; const double *src[8]; float *dst[8]; };
hipError_t launch_output_cast(const DevPlan &p, const OutputCast &c, hipStream_t s);
// Ensemble output: OutputCast's epilogue for nmem members in one launch, and the mean and the spread over the members (two-pass, FP64,
// sequential in ascending member order).  src: the gridded stacks u | v | t | q | phi (nmem*kx grids each, member-major) | ps
// (nmem grids); kind / factor per quantity as OutputCast's.  use: null (all members) or nmem device ints, non-zero = the member
// enters the statistics (the member outputs are written for every member).  members[i]: (ix,il,kx,nmem) float, ps (ix,il,nmem);
// mean[i], spread[i]: (ix,il,kx), ps (ix,il).  A group is wanted if its entry 0 is non-null, and then all six are; 8-byte aligned.
struct EnsOutput {
    int nmem, kx, kind[6];
    double factor[6];
    const double *src;
    const int *use;
    float *members[6], *mean[6], *spread[6];
};
hipError_t launch_ens_output(const DevPlan &p, const EnsOutput &c, hipStream_t s);
// Pressure-level output: EnsOutput's values interpolated in the vertical to nlev targets per member, and the mean and the spread of
// the interpolated values.  src, use: as EnsOutput's.  lv: fsg (log_p 0) or ln fsg (log_p 1); x[l]: the target, plev[l] in Pa or
// ln(plev[l] / p0).  qfac, grav, p0: the factors of q, phi and ps.  members[i]: (ix,il,nlev,nmem) float, ps (ix,il,nmem); mean[i],
// spread[i]: (ix,il,nlev), ps (ix,il); below: null or (ix,il,nlev), the members in use whose lowest level lies above the target.
constexpr int PLEV_MAX_LEVELS = 32;       // SPDY_MAX_PLEV (include/spdy.h)
struct PlevOutput {
    int nmem, nlev, log_p;
    double qfac, grav, p0;
    VLevels lv;
    double x[PLEV_MAX_LEVELS];
    const double *src;
    const int *use;
    float *members[6], *mean[6], *spread[6], *below;
};
hipError_t launch_plev_output(const DevPlan &p, const PlevOutput &c, hipStream_t s);
// once per device, before the first launch: raises the dynamic-LDS limit of every kernel that needs > 64 KB
hipError_t prepare_device_kernels();
hipError_t prepare_device_step_kernels(int kx);

// Column physics of nb states of (ix, il, kx) grids, one thread per column, 5 <= kx <= COLUMN_KMAX: the launch and addressing
// layer the schemes share is csrc/spdy_columns.hpp, their C ABI csrc/spdy_api_physics.hip.
constexpr int COLUMN_KMAX = 16;

// Moist physics (csrc/spdy_physics.hip): physics.f90:110-138.  Per-level tables are bottom up: entry r belongs to the
// reference's level k = kx - r.  Output pointers may be null.
struct MoistCols {
    int nb, ncol, kx;
    const double *tg, *qg, *phig, *pslg;
    double *ttend, *qtend;                        // (ix, il, kx) per state, updated in place
    double *precnv, *precls, *cbmf;               // (ix, il) per state
    int *iptop, *icnv;                            // (ix, il) per state
    double *qsat, *rh, *se;                       // (ix, il, kx) per state
    double fsg[COLUMN_KMAX], wvi2[COLUMN_KMAX], entr[COLUMN_KMAX], grdsig[COLUMN_KMAX], grdscp[COLUMN_KMAX];
    double rhref[COLUMN_KMAX], dqmax[COLUMN_KMAX], pfact[COLUMN_KMAX];
    double fm0;
};
hipError_t launch_moist_columns(const MoistCols &a, hipStream_t s);

// Radiation (csrc/spdy_radiation.hip): physics.f90:146-163 (phase 0), :166 (phase 1) and :180-186 (phase 2).  Per-level
// tables are top down: entry k belongs to the reference's level k + 1.  Output pointers may be null.  The radiation state of a
// model state is rad_state_fields(kx) fields of ncol doubles: tau2 (4 kx, band-major), stratc (2), tt_rsw (kx), flux (4), the
// longwave dfabs of the downward half (kx), slrd (1).
__host__ __device__ constexpr int rad_state_fields(int kx) { return 6 * kx + 7; }
struct RadCols {
    int nb, ncol, ix, il, kx, compute_sw;
    const double *tg, *qg, *phig, *pslg;          // (ix, il, kx) / (ix, il) per state
    const double *rh, *precnv, *precls;           // down, compute_sw only: (ix, il, kx), (ix, il), (ix, il)
    const int *iptop;
    const double *fmask, *albsfc;                 // (ix, il) per state
    const double *ts, *fsfcu;                     // up: (ix, il) per state
    const double *zonal;                          // [5][il]: fsol ozone ozupp zenit stratz (device, plan-owned)
    double *state, *ttend;
    double *cloudc, *clstr, *ssrd, *ssr, *tsr, *slrd, *slr, *olr, *tt_rsw, *tt_rlw;
    int *icltop;
    double dhs[COLUMN_KMAX], abs1[COLUMN_KMAX], wvi2[COLUMN_KMAX], grdscp[COLUMN_KMAX];
    double eps1;                                  // epslw/(dhs(1) + dhs(2))
};
hipError_t launch_radiation(const RadCols &a, int phase, hipStream_t s);   // 0 shortwave, 1 longwave down, 2 up

// Surface fluxes (csrc/spdy_surface.hip, surface_fluxes_kernel): get_surface_fluxes with lfluxland = .true.
// (surface_fluxes.f90:97-295).  Required outputs ts, fsfcu and flux3 (4 fields per state: ustr3 vstr3 shf3 evap3); the others
// may be null.  Three-plane outputs are (ix, il, 3) per state (land, sea, weighted), hfluxn (ix, il, 2).
struct SfcCols {
    int nb, ncol, ix, kx;
    const double *ug, *vg, *tg, *qg, *phig, *pslg;   // (ix, il, kx) / (ix, il) per state
    const double *ssrd, *slrd;                       // (ix, il) per state: the down half of the radiation
    const double *fmask, *sst, *stl, *soilw, *snowc, *alb_l, *alb_s;   // (ix, il) per state
    const double *phis0, *forog, *sqcoa;             // plan-owned: (ix, il), (ix, il), [il] sqrt(coa(j))
    double *ts, *fsfcu, *flux3;
    double *ustr, *vstr, *shf, *evap, *slru, *hfluxn, *tskin, *u0, *v0, *t0;
    double wvi2_kx, sigl_kx, rgas;                   // wvi(kx,2), sigl(kx), rgas = akap*cp
};
hipError_t launch_surface_fluxes(const SfcCols &a, hipStream_t s);

// Vertical diffusion and the boundary-layer sums (csrc/spdy_surface.hip, pbl_kernel): vertical_diffusion.f90:57-142 and
// physics.f90:197-205.  Per-level tables are top down: entry k belongs to the reference's level k + 1.  utend / vtend are read
// and written at level kx only; ut_pbl / vt_pbl (level kx, (ix, il) per state), tt_pbl / qt_pbl may be null.
struct PblCols {
    int nb, ncol, kx, diffmask;                      // diffmask bit k: sigh(k + 1) > 0.5 (the moisture diffusion of level k + 1)
    const double *qg, *phig, *pslg, *se, *rh, *qsat, *flux3;
    const int *icnv;
    double *utend, *vtend, *ttend, *qtend;
    double *ut_pbl, *vt_pbl, *tt_pbl, *qt_pbl;
    double rsig[COLUMN_KMAX], rsig1[COLUMN_KMAX], drh0[COLUMN_KMAX], fvdiq2[COLUMN_KMAX];
    double fshcq, fshcse, fvdise, grdsig_kx, grdscp_kx;
};
hipError_t launch_pbl(const PblCols &a, hipStream_t s);

// The whole chain in one launch (csrc/spdy_column_chain.hip): moist, shortwave (rad.compute_sw), longwave down, surface fluxes,
// longwave up, boundary layer for each column, in the reference's order.  The four argument sets are those of the five calls
// with one difference: precnv, precls, iptop, icnv, slrd, ts, fsfcu and flux3 pass from block to block in registers, so their
// OUTPUT pointers (moist.*, rad.slrd, sfc.ts / fsfcu / flux3) may be null = not stored, and the matching input pointers are not
// read.  se, rh, qsat and ssrd are read back from where moist.* / rad.ssrd put them, so those must be set.
struct ChainCols {
    int nb, ncol, kx;                                // as in each of the four
    MoistCols moist;
    RadCols rad;
    SfcCols sfc;
    PblCols pbl;
};
hipError_t launch_column_chain(const ChainCols &a, hipStream_t s);

// SPPT (csrc/spdy_sppt.hip; sppt.f90, physics.f90:207-222).  The pattern object's counters and seeds live in device memory, so
// one captured advance serves the first step and every later one and each replay draws new noise.  A pattern object holds nmem
// patterns, member-major (member e starts e * kx fields in), and one {draws, seed} per member.
struct SpptState { unsigned long long draws, seed; };
// gen_sppt up to the AR(1) update: one thread per complex coefficient of a member's (mx, nx, kx) rectangle in storage order, the
// member in blockIdx.y.  eta_in null: the coefficient's two Philox4x32-10 draws (include/spdy.h) with the member's seed and
// counter and the index INSIDE the member; otherwise eta_in is copied.  Both parts are clipped to +-10, eta is stored, and spec =
// first * sigma * eta where the member's draws == 0, phi * spec + sigma * eta otherwise: the branch is the member's own.
struct SpptNoise {
    int n, nspec, nmem;                              // mx * nx * kx coefficients per member, mx * nx per level
    const SpptState *state;                          // [nmem]
    const double *sigma, *eta_in;                    // (mx, nx), shared; (mx, nx, kx, nmem) complex or null
    double *eta, *spec;                              // (mx, nx, kx, nmem) complex
    double phi, first;
};
hipError_t launch_sppt_noise(const SpptNoise &a, hipStream_t s);
// the clip of the transformed patterns to +-1 in place, n = ix * il * kx values per member, the member in blockIdx.y; the member's
// thread 0 then counts its advance (draws += 1)
hipError_t launch_sppt_clip(double *pattern, long n, int nmem, SpptState *state, hipStream_t s);
// physics.f90:85-88 and :207-222 around the five calls: save copies the dynamics tendencies (ttend, qtend on every level, utend,
// vtend on level kx) into `save`, (2 kx + 2) fields each g doubles long; apply makes each tendency
// (1 + pattern * mu(k)) * (tend - tend_dyn) + tend_dyn.  pattern is (ix, il, kx) per state; mu is top down.
struct SpptCols {
    int nb, ncol, kx;
    const double *pattern;
    double *utend, *vtend, *ttend, *qtend, *save;
    size_t g;
    double mu[COLUMN_KMAX];
};
hipError_t launch_sppt_save(const SpptCols &a, hipStream_t s);
hipError_t launch_sppt_apply(const SpptCols &a, hipStream_t s);
// The one-launch chain with SPPT (csrc/spdy_column_chain.hip): the thread keeps its column's entry values of utend and vtend
// (level kx) in registers, those of ttend and qtend go through save_t / save_q ((ix, il, kx) per state, as se, rh and qsat
// travel), and the factor is applied after the boundary layer.  Same instructions on the same values as save + chain + apply.
struct ChainSpptCols {
    ChainCols c;
    const double *pattern;
    double *save_t, *save_q;
    double mu[COLUMN_KMAX];
};
hipError_t launch_column_chain_sppt(const ChainSpptCols &a, hipStream_t s);

// The slab land, sea and ice models and the daily forcing (csrc/spdy_surfmodel.hip): couple_sea_land (coupler.f90:30-38) and
// set_forcing parts 2 and 4 (forcing.f90:55-62, :84-99), one thread per column of ONE state.  A surface model keeps its fields in
// one device array of SM_TOTAL fields of ncol doubles: field n at f + n * ncol, month mo (0-based) of a climatology c at
// f + (c + mo) * ncol.  A model of nmem > 1 members (blockIdx.y of both kernels) holds what no kernel writes once and every field
// a kernel writes, SM_STLCL_OB .. SM_CORH, as (nmem, il, ix): member e of field n is ncol doubles after member e - 1 of field n.
// fmask_l is (nmem, il, ix) too, replicated (the physics takes every boundary field per state).  surf_slot gives the place of
// (field, member) in units of ncol doubles; with nmem = 1 it is n, the layout above.
enum SurfField {
    // constants of land_model_init / sea_model_init
    SM_FMASK_L, SM_FMASK_S, SM_ALB0, SM_RHCAPL, SM_CDLAND, SM_RHCAPS, SM_RHCAPI, SM_CDSEA, SM_CDICE,
    // land model, sea and ice model, by the reference's names
    SM_STLCL_OB, SM_SNOWDCL_OB, SM_SOILWCL_OB, SM_STL_LM, SM_STL_AM, SM_SNOWD_AM, SM_SOILW_AM,
    SM_SSTCL_OB, SM_SICECL_OB, SM_TICECL_OB, SM_SSTAN_OB, SM_SST_OM, SM_TICE_OM, SM_SICE_OM,
    SM_SST_AM, SM_SSTAN_AM, SM_SICE_AM, SM_TICE_AM, SM_SSTI_OM,
    // set_forcing: mod_radcon's fields and the gridded humidity correction
    SM_SNOWC, SM_ALB_L, SM_ALB_S, SM_ALBSFC, SM_CORH,
    SM_NFIELDS,
    SM_STL12 = SM_NFIELDS, SM_SNOWD12 = SM_STL12 + 12, SM_SOILW12 = SM_SNOWD12 + 12, SM_SST12 = SM_SOILW12 + 12,
    SM_SICE12 = SM_SST12 + 12, SM_SSTAN3 = SM_SICE12 + 12, SM_TOTAL = SM_SSTAN3 + 3
};
constexpr int SM_NMEMBER = 1 + SM_NFIELDS - SM_STLCL_OB;   // fields held per member: fmask_l and SM_STLCL_OB .. SM_CORH
__host__ __device__ inline bool surf_per_member(int n) { return n == SM_FMASK_L || (n >= SM_STLCL_OB && n < SM_NFIELDS); }
// [fmask_l (nmem)] [fmask_s .. cdice] [SM_STLCL_OB .. SM_CORH (nmem each)] [the climatologies and sstan3]
__host__ __device__ inline long surf_slot(int n, int nmem, int e)
{
    if (n == SM_FMASK_L) return e;
    if (n < SM_STLCL_OB) return (long)nmem - 1 + n;
    if (n < SM_NFIELDS) return (long)nmem - 1 + SM_STLCL_OB + (long)(n - SM_STLCL_OB) * nmem + e;
    return (long)(nmem - 1) * SM_NMEMBER + n;
}
inline long surf_total(int nmem) { return (long)(nmem - 1) * SM_NMEMBER + SM_TOTAL; }
// The date as the interpolations need it (interpolation.f90:16-69), in model memory: forin5's five months (0-based: imon-2 ..
// imon+2) and weights wm2 wm1 w0 wp1 wp2; forint's two months (imon, imon2) and weight wmon; forint(2, sstan3)'s second slot
struct SurfDate {
    double w5[5], wmon;
    int m5[5], m2[2], s2, pad;
};
enum { SURF_LAND = 1, SURF_ICE = 2, SURF_SSTAN = 4 };   // the SPDY_SURFACE_* flags of include/spdy.h
struct SurfCols {
    int ncol, day, flags;
    double *f;                                       // the model's fields
    const SurfDate *date;
    const double *hfluxn, *shf, *evap, *ssrd;        // (ix,il,2), (ix,il,3), (ix,il,3), (ix,il) per member: read with day > 0 only
    int nmem;                                        // members: ONE launch, the member in blockIdx.y, its arrays at uniform offsets
};
hipError_t launch_surface_couple(const SurfCols &a, hipStream_t s);
struct SurfForcingCols {
    int ncol;
    double *f;
    const double *phis0;                             // plan-owned (ix, il)
    double gamlat, pexp;                             // gamma/(1000 grav), 1/(rgas gamlat) (forcing.f90:86, :112)
    int nmem;                                        // as SurfCols::nmem; phis0 is shared
};
hipError_t launch_surface_forcing(const SurfForcingCols &a, hipStream_t s);

// check_diagnostics (csrc/spdy_diagnostics.hip; diagnostics.f90:16-75).  One DiagLevel per level in device memory, written by
// that level's workgroup only: the number of the next step, the level's first offending step (-1: none) with its mask, and the
// level's three numbers of step row_step -- the latest step, until some level has tripped: then that step's, for good.
enum { DIAG_REKE = 1, DIAG_DEKE = 2, DIAG_TEMP_LOW = 4, DIAG_TEMP_HIGH = 8, DIAG_NONFINITE = 16 };   // SPDY_DIAG_* of include/spdy.h
struct DiagLevel {
    long long next_step, bad_step, row_step;
    int bad_mask, pad;
    double row[3];                                   // reke, deke, temp
};
// ONE launch, one workgroup per level: the level's sums over the (mx, nx) rectangle without m = 1, temp, the range test against
// limits (reke, deke, temp low, temp high), row (next_step mod capacity) of history ([capacity][3][kx]) and the state's update.
// nmem members: a (kx, nmem) grid, the member in blockIdx.y.  Member e reads slice e of the (mx, nx, kx, nmem) spectra, owns
// state[e][.] -- its own counter, its own sticky first offence: it reads no other member's -- and block e of each history row.
struct DiagArgs {
    const double *vor, *div, *t;                     // (mx, nx, kx, nmem) complex
    const double *elm2, *limits;                     // (mx, nx); 4: shared
    double *history;                                 // [capacity][nmem][3][kx]
    DiagLevel *state;                                // [nmem][kx]
    int nspec, mx, kx, capacity;                     // nspec = mx * nx
    int nmem;
};
hipError_t launch_diagnostics(const DiagArgs &a, hipStream_t s);
// use[e] = 1 if none of member e's kx levels holds a first offence, else 0: one launch, one thread per member (include/spdy.h,
// "member mask")
hipError_t launch_diagnostics_use(const DiagLevel *state, int nmem, int kx, int *use, hipStream_t s);

// The ensemble analysis (csrc/spdy_letkf.hip; include/spdy.h, "ensemble analysis").  Gridded ensemble arrays are
// member-major: field (e, k) of a level variable starts (e * kx + k) * ncol doubles in, the surface field of member e e * ncol.
enum { LETKF_VARS = 5 };                             // u, v, t, q, ps: the SPDY_OBS_* order
constexpr int LETKF_MAX_MEMBERS = 32;
// The observation stage (csrc/spdy_obsop.hpp): one argument for every launch that observes or couples.  The
// observations [first, last) of the network: the four-point stencil the host made, the members in ascending order.  atp NULL: a
// model-level network, and nothing of the pressure part is read or written.  Otherwise (include/spdy.h, "observations at a
// pressure") atp[o] != 0 marks an observation given at a pressure (its lev[o] is 0: a kernel that does not know of it
// stays in bounds) and lnp[o] = ln(p_o / p0) is its target.
struct LetkfObserve {
    int first, last, nmem, kx, ncol;
    const int *var, *lev, *sidx;                     // [nobs], [nobs] (0 for ps), [nobs][4] grid points j * ix + i
    const double *swgt, *value;                      // [nobs][4], [nobs]
    const double *x[LETKF_VARS];                     // the gridded ensemble
    double *hx, *hxmean, *y, *dep;                   // [nobs][nmem], [nobs], [nobs][nmem], [nobs]
    const int *atp;                                  // [nobs], or NULL
    const double *lnp, *rinv;                        // [nobs], [nobs] 1 / error^2
    double *olns, *used, *reff;                      // [nobs] each
    double *slot_ps, *slot_out;                      // [nobs][nmem] each: what a slot keeps per member besides hx
    VLevels lv;                                      // ln fsg
    const int *umap;                                 // NULL, or the member mask's table (below)
};
// hx, hxmean, y and departure of every observation of the range in one launch.  A model-level network: one thread per observation.
// With atp: a workgroup owns whole observations, one thread per (observation, member) interpolates the four stencil columns of its
// member, one thread per observation then couples the members; written besides: olns[o] = lnp[o] - psbar_o of the at-pressure
// observations only (the others keep what set_obs uploaded), used[o] (1.0 / 0.0) and reff[o] = used ? rinv[o] : 0.0 of all.
// umap: the sums and the out-of-column test over its members, y = 0.0 for the others; hx is every member's own.
hipError_t launch_letkf_observe(const LetkfObserve &a, hipStream_t s);
// Observations in time slots (include/spdy.h, "observations in time slots").  Observing a slot: what is per member
// only, one thread per (observation of the range, member) -- hx[o][e] with the bits launch_letkf_observe gives it and, with atp,
// slot_ps[o][e], the stencil's ps_e, and slot_out[o][e], 1.0 / 0.0, the member's out-of-column flag.  Nothing else is written, and
// umap is not read.
hipError_t launch_letkf_slot_obs(const LetkfObserve &a, hipStream_t s);
// The finish, in the observation launch's place of an analysis call: everything that couples members, from the rows the slots kept
// -- what launch_letkf_observe writes besides hx, with its bits.  x is not read.  One thread per observation.
hipError_t launch_letkf_slot_finish(const LetkfObserve &a, hipStream_t s);
// The member mask (include/spdy.h, "member mask").  One small launch turns the caller's use[nmem] into the table the
// masked kernels read, umap [LETKF_UMAP]: umap[0] = n, the members in use; umap[1 + c] = u_c, the member of compact index c < n,
// ascending; umap[LETKF_URANK + e] = member e's compact index, -1 for a member not in use; *nused = n as a double.
enum { LETKF_URANK = 33, LETKF_UMAP = 66 };
hipError_t launch_letkf_mask(const int *use, int nmem, int *umap, double *nused, hipStream_t s);
// The local analyses: one workgroup per grid column.  nlv levels' eigenproblems are in flight at a time (1, 2 or 4: what the LDS
// holds; the results do not depend on it); lds = letkf_lds_bytes(nmem, kx, nlv).
struct LetkfCols {
    int nobs, nmem, kx, ncol, nlv;
    double ch, cv, diag;                             // c_h in metres, c_v (<= 0: no vertical factor), (nmem - 1) / rho
    const double *colunit, *lnfsg;                   // [3][ncol] unit vectors of the columns, [kx] ln fsg
    const double *ounit, *olns, *rinv;               // [nobs][3], [nobs] ln sigma_o, [nobs] 1 / error^2
    const double *y, *dep;                           // as LetkfObserve
    const double *x[LETKF_VARS];
    double *dx[LETKF_VARS];                          // the increments; may be x
    // weight interpolation (both NULL / 0: every grid column is solved and gets its increments).  With a column list the
    // workgroups solve the nlist listed columns only and write T of every level, [list][kx][nmem][nmem], instead of increments
    int nlist;
    const int *cols;                                 // [nlist] grid columns j * ix + i, ascending
    double *tw;
};
// LetkfCols under the member mask: the kernel solves the problem of umap's n members in compact indices, with (n - 1) / rho formed
// on the device (c.diag is not read), in the LDS layout of n; y, x, dx and tw keep the strides of c.nmem.  A type of its own, so
// that the unmasked kernels' argument is the one it was.
struct LetkfMaskedCols {
    LetkfCols c;
    double rho;
    const int *umap;
};
size_t letkf_lds_bytes(int nmem, int kx, int nlv);
hipError_t letkf_prepare(size_t lds);                // before the first launch on a device: admits a compute unit's whole LDS
// The increments of every grid column from the transforms of a coarse set: per column a stencil of four list entries and their
// weights (a zero weight: the entry is not read), T = ((w0 T0 + w1 T1) + w2 T2) + w3 T3 from the first term present, then
// dx_e = sum_f (x_f - mean) T[f][e] as the transform kernel forms it.
struct LetkfApply {
    int nmem, kx, ncol, nlist;
    const int *iidx;                                 // [ncol][4] entries of the coarse list
    const double *iwgt;                              // [ncol][4]
    const double *tw;                                // [nlist][kx][nmem][nmem]
    const double *x[LETKF_VARS];
    double *dx[LETKF_VARS];                          // may be x
};
// umap: NULL, or the member mask's table -- the members in use from the leading n x n block of each T, 0.0 for the others
hipError_t launch_letkf_apply(const LetkfApply &a, hipStream_t s, const int *umap = nullptr);
// dst[i] += src[i] for nops arrays in one launch; an increment equal to zero leaves the destination's bits (a -0.0 included)
struct LetkfAdd {
    int nops;
    long n[LETKF_VARS];
    double *dst[LETKF_VARS];
    const double *src[LETKF_VARS];
};
hipError_t launch_spec_add(const LetkfAdd &a, hipStream_t s);
// Relaxation to the prior perturbations and spread (include/spdy.h, "relaxation"): one launch over the (4 kx + 1)
// ncol grid items after the increments have been formed.  raw: the increments as the transform or apply kernel wrote them; dx: the
// relaxed increments, which may be x (never raw); inflation [(4 kx + 1)][ncol]: the factor f of every item.
struct LetkfRelax {
    int nmem, kx, ncol;
    double omr, rtps;                                // 1 - rtpp, formed on the host; rtps
    const double *x[LETKF_VARS];
    const double *raw[LETKF_VARS];
    double *dx[LETKF_VARS];
    double *inflation;
    const int *umap;                                 // NULL, or the member mask's table
};
hipError_t launch_letkf_relax(const LetkfRelax &a, hipStream_t s);
// The background check and the observation statistics (include/spdy.h, "background check and observation statistics"; DESIGN.md
// s27): ONE launch between the observation stage and the transform, one workgroup per group.  Per observation of the network, from
// the y and dep the observation stage has just written: s2 = (sum_U y_e^2) / (n - 1), v = s2 + err^2, rejected if dep^2 > g2 v
// (g2 == 0 or n < 2: the test is not made); check[o] = 0.0 passed, 1.0 rejected, 2.0 out of column (incol[o] == 0, which wins;
// incol NULL: every observation is in its column); used[o] = check == 0 ? 1.0 : 0.0, reff[o] = used ? rinv[o] : 0.0, depb[o] =
// dep[o].  decide false (the stats-only call): check and depb are read, not written, and used and reff follow them.  stats
// [ngroups][QC_STATS]: n_all, n_out, n_rej, n_used, then over the used ones sum dep, dep^2, s2, err^2, dep depb, depb -- thread t of
// 1024 takes the group's observations o = t (mod 1024) ascending, then a halving tree in LDS; no atomics.  group NULL: var.
enum { QC_STATS = 10, QC_MAX_GROUPS = 64 };
struct LetkfQc {
    int nobs, nmem, ngroups;
    double g2;                                       // gross * gross, formed on the host
    const int *group, *var;                          // [nobs] each; group may be NULL
    const double *y, *dep, *err, *rinv;              // [nobs][nmem], [nobs], [nobs], [nobs]
    const double *incol;                             // [nobs] what the observation stage wrote to used, or NULL; may be used
    double *used, *reff;                             // [nobs] each
    double *check, *depb;                            // [nobs] each: the record and the departure of the latest checked analysis
    double *stats;                                   // [ngroups][QC_STATS]: the row of the call's slot
    const int *umap;                                 // NULL, or the member mask's table
};
hipError_t launch_letkf_qc(const LetkfQc &a, bool decide, hipStream_t s);
// Adaptive inflation (include/spdy.h, "adaptive inflation").  The transform under a field rho [kx][ncol]: LetkfCols
// with the diagonal of level k of column col formed on the device as (n - 1) / rho[k * ncol + col] (c.diag is not read), without
// and with the member mask.  Types of their own, as LetkfMaskedCols is: the kernels on the other two arguments stay what they were.
struct LetkfAdaptiveCols {
    LetkfCols c;
    const double *rho;
};
struct LetkfAdaptiveMaskedCols {
    LetkfCols c;
    const double *rho;
    const int *umap;
};
// The transform's one launcher: LetkfCols with the scalar rho (read by the masked form; c.diag has it for the plain one), under the
// field `field` if not NULL, under the member mask's table umap if not NULL -- the kernel on the argument struct of that route.
hipError_t launch_letkf_transform(const LetkfCols &c, double rho, const double *field, const int *umap, size_t lds, hipStream_t s);
// The estimate, TWO launches after everything else of an analysis call: s2[o] of every observation, one thread each; then one
// workgroup per grid column scans the network as the transform kernel does and lane k < kx sums p1, p2, p3 of level k over the
// observations in range, ascending, updates rho[k][col] in place and stores parm [3][kx][ncol].  reff: the 1 / error^2 the call's
// transform read.  n < 2 under the mask: neither launch writes anything.
struct LetkfInfl {
    int nobs, nmem, kx, ncol;
    double ch, cv;                                   // as LetkfCols
    double vb, rho_min, rho_max;                     // sigma_b^2, formed on the host; the bounds
    const double *colunit, *lnfsg, *ounit, *olns, *reff, *y, *dep;
    double *s2, *rho, *parm;                         // [nobs], [kx][ncol], [3][kx][ncol]
    const int *umap;                                 // NULL, or the member mask's table
};
hipError_t launch_letkf_infl(const LetkfInfl &a, hipStream_t s);

// The nature run (csrc/spdy_nature.hip; include/spdy.h, "nature run").  The truth is one member of the analysis'
// gridded layout: row f = v * kx + k of u, v, t, q, then ps, (4 kx + 1) grids.  state = {seed, draws}.
// The observation values of the observations [first, last) of an analysis object's network from the truth, one thread each
// (include/spdy.h, "observations in time slots": a slot's draw is the whole network's draw on its range): h as the analysis forms
// hx, the truth being the one member (csrc/spdy_obsop.hpp), then value = h + (noise * error) * z with z = sppt_randn(o, 0, draws,
// seed); noise == 0 stores h.  Reads state, does not advance it.  atp NULL: a model-level network.  Otherwise atp[o] != 0 marks an
// observation given at a pressure with the target lnp[o]: h is the bilinear sum of the four columns' values interpolated to the
// target with the truth's ps, clamped to the end level outside the column.
struct NatureObs {
    int first, last, nobs, kx, ncol;
    const int *var, *lev, *sidx;                     // the analysis object's tables, as LetkfObserve
    const double *swgt, *error;                      // [nobs][4], [nobs]
    const double *truth;                             // (4 kx + 1) grids
    const unsigned long long *state;
    double noise;
    double *value;                                   // [nobs]
    const int *atp;                                  // [nobs], or NULL
    const double *lnp;                               // [nobs]
    VLevels lv;                                      // ln fsg
};
hipError_t launch_nature_slot_draw(const NatureObs &a, hipStream_t s);
// draws += 1 by one thread: every launch before it on the stream has read the counter, every launch after it sees the new one
hipError_t launch_nature_count(unsigned long long *state, hipStream_t s);
// The scores of an ensemble on the grid (x: LetkfObserve::x) against the truth, two launches.  One workgroup per (row, latitude) forms
// the zonal sums of mbar, mbar^2 and sum_e (d_e - mbar)^2 / (E - 1), d_e = x_e - truth, mbar = (sum_e d_e, e ascending) / E, in a
// fixed tree into part [nrows][il][3]; one thread per row then adds them over the latitudes in ascending order with gw [il] and
// writes rmse | bias | spread of its row into scores [3][nrows].  No atomics.
struct NatureScore {
    int nmem, kx, ix, il;
    const double *x[LETKF_VARS];
    const double *truth, *gw;
    double *part, *scores;
    const int *use;                                  // NULL, or [nmem]: non-zero = the member is scored (the caller's array, read as it is)
};
hipError_t launch_nature_score(const NatureScore &a, hipStream_t s);

}  // namespace spdy
