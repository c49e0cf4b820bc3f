/*
 * spdy.h -- C ABI of the MI355X-native spectral transform path for speedy.f90.
 *
 * This is the drop-in boundary: every entry point below replaces one public procedure of the
 * reference's Fortran modules `spectral`, `fourier`, `legendre`, `horizontal_diffusion` and
 * `implicit` (file:line cited per function, relative to /root/reference/source).  The
 * reference-side binding (an ISO_C_BINDING module that keeps the reference's names and
 * signatures) is speedy.f90_amd/fortran/spectral.f90; see INTEGRATION.md.
 *
 * Conventions
 *  - All data is FP64.  Arrays are Fortran column-major exactly as the reference declares them:
 *        grid  g(ix,il)            ix*il doubles, longitude fastest, j=1 southernmost
 *        spec  s(mx,nx) complex    mx*nx (re,im) pairs, zonal wavenumber index fastest
 *        four  f(2*mx,il)          re/im interleaved Fourier coefficients per latitude
 *    A batch of nb fields is nb such arrays back to back (e.g. a (mx,nx,kx) level stack).  An output field depends on the
 *    inputs the reference reads for that field and on nothing else the batch holds, non-finite values included: a NaN, an
 *    infinity or an overflow in one field -- or in an entry the reference never reads -- changes no bit of another field.
 *  - Functions without suffix take HOST pointers: they copy in, run the HIP kernels, copy out
 *    and synchronise (signature-compatible with the reference, PCIe-bound).
 *    Functions ending in _dev take DEVICE pointers, are asynchronous on the plan's stream and
 *    never touch the host -- this is the throughput path (state stays resident in HBM).
 *  - Every function returns 0 on success or a negative SPDY_ERR_* code; spdy_last_error()
 *    gives the message for the calling thread.  There is no CPU fallback: without a usable
 *    HIP device every compute entry point fails with SPDY_ERR_NO_DEVICE.
 *  - A plan is immutable after creation (except spdy_implicit_init / spdy_plan_set_stream);
 *    calls on one plan are serialised by its stream; distinct plans are independent.
 */
#ifndef SPDY_H
#define SPDY_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spdy_plan spdy_plan;

enum {
    SPDY_OK = 0,
    SPDY_ERR_ARG = -1,          /* bad argument (null pointer, nb > max_batch, bad kcos ...)   */
    SPDY_ERR_UNSUPPORTED = -2,  /* resolution the kernels are not built for                   */
    SPDY_ERR_NO_DEVICE = -3,    /* no HIP device / host-only plan used for compute             */
    SPDY_ERR_HIP = -4,          /* a HIP runtime call failed                                  */
    SPDY_ERR_STATE = -5,        /* e.g. implicit_terms before implicit_init                    */
    SPDY_ERR_TABLE = -6,        /* generated table failed its pinned-value self check          */
    SPDY_ERR_COMM = -7          /* RCCL could not be loaded / a collective failed              */
};

/* ---- plan ------------------------------------------------------------------------------
 * Replaces the private module state filled by initialize_geometry (geometry.f90:35),
 * initialize_fourier (fourier.f90:18), initialize_legendre (legendre.f90:23),
 * initialize_spectral (spectral.f90:20) and initialize_horizontal_diffusion
 * (horizontal_diffusion.f90:36).  Supported: (trunc,ix,iy) = (30,96,24) and (63,192,48); 1 <= kx <= SPDY_MAX_KX.
 * Transforms, operators and do_horizontal_diffusion are level-agnostic.  Everything that needs sigma levels
 * (implicit solve, geopotential, spectral tendencies, the diffusion block's orographic correction) works out of the
 * box for kx in {5,7,8} -- the only sets the reference defines (geometry.f90:42-48) -- and for any other kx after
 * spdy_plan_set_sigma.
 * device >= 0 selects a HIP device; device = SPDY_DEVICE_AUTO takes $SPDY_DEVICE, else the process's local rank
 * ($LOCAL_RANK, $OMPI_COMM_WORLD_LOCAL_RANK, $SLURM_LOCALID) modulo the visible devices, else device 0;
 * device = SPDY_DEVICE_NONE builds a host-only plan (tables only: lets CPU-side tests inspect tables; every compute
 * call on it returns SPDY_ERR_NO_DEVICE).
 * max_batch bounds nb of every batched call.  Device memory beyond the tables (< 10 MB) is allocated on demand:
 * the host-pointer entry points stage through 4 x max_batch grids (+ 4 x 512 KB of pinned host memory for small calls,
 * $SPDY_HOST_STAGE_KB below) from their first call on; the four-kernel path
 * (spdy_plan_set_fused(0)) and the T63 operator+transform sequences
 * keep a workspace of max_batch x (il x 2mx + 2 mx nx complex) doubles, allocated at plan creation when it is <= 64 MB
 * (model-shaped plans: a graph capture then needs no warm-up) and at the first call that needs it otherwise (allocation
 * inside an open capture is refused with SPDY_ERR_STATE).  Destroying a plan also invalidates the graphs captured
 * from it (spdy_graph_launch then returns SPDY_ERR_STATE) and shuts down its communicators (spdy_comm_*: the handles
 * stay valid for spdy_comm_destroy, every other call on them returns SPDY_ERR_STATE).
 * The same rule holds for every object made on a plan (spdy_surface_model, spdy_sppt, spdy_diagnostics, spdy_letkf, spdy_nature):
 * its device memory is the plan's and goes with it, the handle stays valid for its _destroy, and every other call on it returns
 * SPDY_ERR_STATE.  A plan and what was made on it may so be destroyed in any order.                                  */
/* Environment read by the library (measurement and debugging aids; none changes results beyond rounding-level path choices).
 * The launch-policy switches (SPDY_T30_*, SPDY_T63_*, SPDY_WT_MIN_MB) are read ONCE per plan, in spdy_plan_create; a plan's
 * values are changed afterwards with spdy_plan_set_option.
 *   SPDY_DEVICE        device index for SPDY_DEVICE_AUTO              SPDY_FUSED = 0 | 1   initial spdy_plan_set_fused mode
 *   SPDY_WG_PER_CU     persistent workgroups per CU of the T30 kernels (default 1)
 *   SPDY_COMM_FORCE=1  issue the collectives even at world size 1
 *   SPDY_SHARD_TRANSPOSE=1  communicators created under it run the level-sharded step in its transposed form (spdy_comm_set_option)
 *   SPDY_T63_NOSPLIT   one workgroup per pair in small T63 direct launches instead of two (same bits)
 *   SPDY_T63_NODERIVE  T63 model-sized inverse batches run uvspec / grad as an operator kernel in front of the transform launch instead
 *                      of evaluating them where the transform loads its operands (agree to rounding)
 *   SPDY_T63_NOSTAGE   small T63 direct batches run fused (row FFTs inside the contraction launch) instead of staged (same bits)
 *   SPDY_T63_NP2_FROM  pairs from which the staged contraction takes two pairs per workgroup (default 40; same bits)
 *   SPDY_T30_NOSPLIT   small T30 direct batches as whole tiles instead of three workgroups per tile (same bits)
 *   SPDY_WT_MIN_MB     output size (MB, default 6) from which a model-sized launch writes its output through the L2s instead of
 *                      leaving it dirty for the end-of-kernel release (0 = never; same bits either way)
 *   SPDY_COMM_TIMEOUT_S  seconds (> 0; default 120; read when a group is created) an in-process collective waits for its missing ranks before it breaks the group
 *   SPDY_T30_NOPART    small T30 inverse launches walk whole tiles instead of (tile, third of the latitudes) items (same bits)
 *   SPDY_COMM_DRY=1    RCCL communicators created under it skip their collectives (timing a sharded step without its
 *                      exchanges; results are then wrong)
 *   SPDY_HOST_SPIN=0   host-staged calls (below) end in hipStreamSynchronize instead of spinning on a host-mapped completion stamp that
 *                      a one-thread kernel behind the call's kernels writes (the spin saves the runtime's wake-up: 1.3x the rate of
 *                      one-field calls at T30; it gives up after 2 s and falls back to the runtime)
 *   SPDY_HOST_STAGE_KB host-pointer calls whose largest array is at most this many KB (default 512; 0 = never) stage through
 *                      pinned host memory mapped into the device: the caller's thread copies in and out, the kernels read and
 *                      write the staging buffers across the link themselves (no copy-engine round trips: 1.4-1.6x the rate
 *                      of one-field calls); larger calls use device staging and hipMemcpyAsync.  Same bits either way.      */
enum { SPDY_MAX_KX = 32, SPDY_DEVICE_NONE = -1, SPDY_DEVICE_AUTO = -2 };
int spdy_plan_create(int trunc, int ix, int iy, int kx, int max_batch, int device, spdy_plan **plan);
int spdy_plan_destroy(spdy_plan *plan);
/* Half levels hsg[kx+1] (strictly increasing within [0,1]) for a level count the reference has no set for -- or
 * to override its set.  Rebuilds dhs, fsg, dhsr, fsgr (geometry.f90:51-60) and the tables derived from them
 * (geopotential.f90:22-30, horizontal_diffusion.f90:70-82); spdy_implicit_init must be called (again) afterwards. */
int spdy_plan_set_sigma(spdy_plan *plan, const double *hsg);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream); NULL restores the plan's own. */
int spdy_plan_set_stream(spdy_plan *plan, void *hip_stream);
int spdy_plan_synchronize(spdy_plan *plan);
/* Device memory for a host that has no HIP binding of its own (the Fortran model: fortran/time_stepping.f90 keeps the
 * reference's prognostics -- prognostics.f90:16-24 -- in HBM with these).  spdy_dev_alloc returns zero-filled memory on
 * the plan's device; upload/download are ordered on the plan's stream and return when the copy is complete; none of the
 * four may be called while a graph capture is open (SPDY_ERR_STATE).  A host with HIP (hipfort, torch) does not need them:
 * every *_dev entry point takes any device pointer.                                                                   */
int spdy_dev_alloc(spdy_plan *plan, size_t bytes, void **d_ptr);
int spdy_dev_free(spdy_plan *plan, void *d_ptr);
int spdy_dev_upload(spdy_plan *plan, void *d_dst, const void *src, size_t bytes);
int spdy_dev_download(spdy_plan *plan, void *dst, const void *d_src, size_t bytes);

/* Per-kernel timing for the roofline report: while on, every transform kernel launched by the
 * *_dev entry points is bracketed by HIP events on its own stream.  spdy_plan_get_profile
 * synchronises, adds up milliseconds and launch counts per kernel kind (arrays of
 * SPDY_K_COUNT) and clears the record.                                                       */
enum { SPDY_K_LEGENDRE_INV = 0, SPDY_K_FOURIER_INV = 1, SPDY_K_FOURIER_DIR = 2, SPDY_K_LEGENDRE_DIR = 3,
       SPDY_K_S2G_FUSED = 4, SPDY_K_G2S_FUSED = 5, SPDY_K_COUNT = 6 };
int spdy_plan_set_profiling(spdy_plan *plan, int on);
/* Kernel selection for the transforms: 1 and -1 (default) = fused single-pass kernels (T30, T63) at every batch size,
 * 0 = the four-kernel path (any resolution; the only path for other resolutions).  The two paths agree to rounding, not
 * bitwise; within one setting a field's bits never depend on the size or composition of the batch it travels in
 * (tests/test_gpu_determinism.py).  Fused launches whose grid-side array is >= 16 MB stream it with
 * non-temporal loads/stores (the data passes through the caches once); smaller ones leave it cached for their
 * consumer.                                                                                        */
int spdy_plan_set_fused(spdy_plan *plan, int mode);
/* Launch-policy switches of one plan (measurement and test aids; same results, see the environment list above -- the
 * environment gives a plan its initial values when it is created and is not read again).  name / value:
 *   "t30_part", "t30_split", "t63_split", "t63_stage", "t63_derive"   0 = the form named by $SPDY_T30_NOPART, $SPDY_T30_NOSPLIT,
 *                       $SPDY_T63_NOSPLIT, $SPDY_T63_NOSTAGE, $SPDY_T63_NODERIVE; 1 = the default form
 *   "t63_np2_from" >= 1, "wt_min_mb" >= 0                              as $SPDY_T63_NP2_FROM, $SPDY_WT_MIN_MB
 *   "physics_fused"     the column-physics chain as ONE launch (1) or as its five calls (0), same bits either way; any other
 *                       value is SPDY_ERR_ARG.  Never set: spdy_column_physics_dev makes the five calls, spdy_physics_dev the one launch
 *   "ens_member_qcorh"  1: spdy_ens_spectral_step_dev and spdy_ens_direct_batch_spectral_step_dev read d_qcorh as (mx,nx,nmem), a
 *                       field per member ("ensemble time step" below); 0 (the default): one shared (mx,nx) field.  Read when the
 *                       call is enqueued; the single-state calls ignore it.  Any other value is SPDY_ERR_ARG.  It describes
 *                       an argument, not a launch form, so it alone may be set while a capture is open.
 * Not while a graph capture is open (SPDY_ERR_STATE); captured graphs keep the forms they were captured with.       */
int spdy_plan_set_option(spdy_plan *plan, const char *name, int value);
int spdy_plan_get_profile(spdy_plan *plan, double *ms, int *launches);
/* Diagnostic: where the dispatcher places the eight waves of a workgroup shaped like the fused T63 kernels' (512 threads,
 * their LDS footprint, one workgroup per CU).  simd_of_wave[0..7] = SIMD of waves 0..7 of workgroup 0; violations = how many of
 * the launch's workgroups (one per CU) do NOT have waves w and w + 4 on one SIMD and waves 0..3 on four different ones.  The
 * T63 kernels assign their two wave roles to SIMDs on that assumption (csrc/spdy_fused_t63.inc: a tuning choice per kernel,
 * results do not depend on it); tests/test_gpu_determinism.py checks violations == 0.                                      */
int spdy_wave_placement(spdy_plan *plan, int *simd_of_wave, int *violations);
/* dims[0..7] = trunc, ix, iy, il, kx, nx, mx, max_batch */
int spdy_plan_dims(const spdy_plan *plan, int *dims);
const char *spdy_last_error(void);
/* Copy a named host table into buf (up to cap doubles); returns the element count or <0.
 * Names: sia_half coa_half cosgr cosgr2 hsg dhs fsg dhsr fsgr work ifac epsi wt poly nsh2
 *        el2 elm2 el4 trfilt gradx gradym gradyp uvdx uvdym uvdyp vddym vddyp
 *        dmp dmpd dmps dmp1 dmp1d dmp1s tref tref1 tref2 tref3 xc xd xj dhsx elz
 *        xgeop1 xgeop2 corf tcorv qcorv coriol sigl sigh grdsig grdscp wvi entr fband
 *        fsol ozone ozupp zenit stratz (the last five after spdy_radiation_set_date)            */
int spdy_get_table(const spdy_plan *plan, const char *name, double *buf, int cap);

/* ---- grid <-> spectral transforms --------------------------------------------------------
 * spec_to_grid(vorm,kcos)  spectral.f90:98-110  = fourier_inv(legendre_inv(.),kcos)
 * grid_to_spec(vorg)       spectral.f90:112-122 = legendre_dir(fourier_dir(.))
 * kcos semantics as fourier.f90:47-51: 1 = plain, anything else = multiply row j by cosgr(j). */
int spdy_spec_to_grid(spdy_plan *plan, const double *spec, int kcos, double *grid);
int spdy_grid_to_spec(spdy_plan *plan, const double *grid, double *spec);
/* nb independent fields; kcos[nb] per field (NULL = all 1). */
int spdy_spec_to_grid_batch(spdy_plan *plan, int nb, const double *spec, const int *kcos, double *grid);
int spdy_grid_to_spec_batch(spdy_plan *plan, int nb, const double *grid, double *spec);
/* Device-resident batch.  d_kcos: device int[nb] or NULL (then kcos_all applies to every field). */
int spdy_spec_to_grid_dev(spdy_plan *plan, int nb, const double *d_spec, const int *d_kcos, int kcos_all,
                          double *d_grid);
int spdy_grid_to_spec_dev(spdy_plan *plan, int nb, const double *d_grid, double *d_spec);

/* ---- transform stages (host pointers, batched) -------------------------------------------
 * legendre_inv legendre.f90:74-111 ; legendre_dir legendre.f90:114-155
 * fourier_inv  fourier.f90:23-53   ; fourier_dir  fourier.f90:56-82                          */
int spdy_legendre_inv(spdy_plan *plan, int nb, const double *spec, double *four);
int spdy_legendre_dir(spdy_plan *plan, int nb, const double *four, double *spec);
int spdy_fourier_inv(spdy_plan *plan, int nb, const double *four, int kcos, double *grid);
int spdy_fourier_dir(spdy_plan *plan, int nb, const double *grid, double *four);

/* ---- spectral-space operators (nb fields each) -------------------------------------------
 * laplacian spectral.f90:84 ; inverse_laplacian :91 ; trunct :229 (in place)
 * grad :124 ; vds :146 ; uvspec :173 ; vdspec :198 (kcos==2: *cosgr, else *cosgr2)            */
int spdy_laplacian(spdy_plan *plan, int nb, const double *in, double *out);
int spdy_inverse_laplacian(spdy_plan *plan, int nb, const double *in, double *out);
int spdy_trunct(spdy_plan *plan, int nb, double *inout);
int spdy_grad(spdy_plan *plan, int nb, const double *psi, double *psdx, double *psdy);
int spdy_vds(spdy_plan *plan, int nb, const double *ucosm, const double *vcosm, double *vorm, double *divm);
int spdy_uvspec(spdy_plan *plan, int nb, const double *vorm, const double *divm, double *ucosm, double *vcosm);
int spdy_vdspec(spdy_plan *plan, int nb, const double *ug, const double *vg, double *vorm, double *divm, int kcos);
int spdy_laplacian_dev(spdy_plan *plan, int nb, const double *in, double *out);
int spdy_inverse_laplacian_dev(spdy_plan *plan, int nb, const double *in, double *out);
int spdy_trunct_dev(spdy_plan *plan, int nb, double *inout);
int spdy_grad_dev(spdy_plan *plan, int nb, const double *psi, double *psdx, double *psdy);
int spdy_vds_dev(spdy_plan *plan, int nb, const double *ucosm, const double *vcosm, double *vorm, double *divm);
int spdy_uvspec_dev(spdy_plan *plan, int nb, const double *vorm, const double *divm, double *ucosm, double *vcosm);
/* device-pointer operators: outputs must not overlap inputs (except spdy_trunct_dev, which is in place);
 * vdspec at T30 is one kernel and writes its outputs while other inputs are still being read */
int spdy_vdspec_dev(spdy_plan *plan, int nb, const double *ug, const double *vg, double *vorm, double *divm, int kcos);

/* ---- spectral-space tail ------------------------------------------------------------------
 * do_horizontal_diffusion(field,fdt_in,dmp,dmp1) horizontal_diffusion.f90:86-105:
 *     fdt_out = (fdt_in - dmp*field)*dmp1, nlev levels sharing the two (mx,nx) real tables.
 * initialize_implicit(dt) implicit.f90:36-165 ; implicit_terms(divdt,tdt,psdt) :168-217
 * (in place; divdt,tdt are (mx,nx,kx), psdt is (mx,nx)).                                      */
int spdy_hdiff(spdy_plan *plan, int nlev, const double *field, const double *fdt_in, const double *dmp,
               const double *dmp1, double *fdt_out);
int spdy_hdiff_dev(spdy_plan *plan, int nlev, const double *field, const double *fdt_in, const double *d_dmp,
                   const double *d_dmp1, double *fdt_out);
/* The seven diffusion calls of one time step (time_stepping.f90:63-96) in one launch: nops <= SPDY_HDIFF_MAX_OPS
 * independent operations, each as spdy_hdiff_dev would do it (device pointers; ops is a host array).          */
enum { SPDY_HDIFF_MAX_OPS = 8 };
typedef struct {
    int nlev;
    const double *field, *fdt_in, *d_dmp, *d_dmp1;
    double *fdt_out;
} spdy_hdiff_op;
int spdy_hdiff_multi_dev(spdy_plan *plan, int nops, const spdy_hdiff_op *ops);
int spdy_implicit_init(spdy_plan *plan, double dt);
int spdy_implicit_terms(spdy_plan *plan, double *divdt, double *tdt, double *psdt);
int spdy_implicit_terms_dev(spdy_plan *plan, double *divdt, double *tdt, double *psdt);
/* Device copies of the plan's damping tables for spdy_hdiff_dev: name in
 * {dmp,dmpd,dmps,dmp1,dmp1d,dmp1s}; *d_ptr stays valid until the next spdy_implicit_init.     */
int spdy_device_table(spdy_plan *plan, const char *name, const double **d_ptr);

/* ---- spectral side of a time step (device-resident prognostics) ---------------------------------------------
 * With these a host keeps vor, div, t, ps, tr in HBM across steps: everything between the direct transforms of one
 * step and the inverse transforms of the next runs on the device (and can be captured into one graph).
 *   get_geopotential(t, phis) -> phi                         geopotential.f90:33-57
 *   get_spectral_tendencies(divdt, tdt, psdt, j2)            tendencies.f90:242-293: div, t, ps are the time-level-j2
 *       slabs of the prognostics, phis the surface geopotential; phi is written like the reference's module variable
 *   the diffusion block of step()                            time_stepping.f90:62-96: seven do_horizontal_diffusion
 *       calls with the orographic corrections ctmp = t + tcorh*tcorv(k), tr + qcorh*qcorv(k) and the stratospheric
 *       zonal-wind drag sdrag folded in; vor..tr are time level 1; tcorh/qcorh are device (mx,nx) complex arrays the
 *       host owns (forcing.f90 computes them); tr/trdt/qcorh may all be NULL (no tracer; the reference has ntr = 1)
 *   step_field_2d/3d(j1, dt, eps, input, fdt)                time_stepping.f90:121-167: leapfrog + Robert-Asselin-
 *       Williams filter; field is (mx,nx,nlev,2) with both time levels, fdt (mx,nx,nlev) is truncated in place as the
 *       reference does when ix == 4*iy; wil is the caller's params%wil.  Up to SPDY_STEP_MAX_OPS arrays per launch.   */
int spdy_geopotential(spdy_plan *plan, const double *t, const double *phis, double *phi);
int spdy_geopotential_dev(spdy_plan *plan, const double *t, const double *phis, double *phi);
int spdy_spectral_tendencies_dev(spdy_plan *plan, const double *div, const double *t, const double *ps, const double *phis,
                                 double *divdt, double *tdt, double *psdt, double *phi);
int spdy_hdiff_step_dev(spdy_plan *plan, const double *vor, const double *div, const double *t, const double *tr,
                        const double *d_tcorh, const double *d_qcorh, double sdrag,
                        double *vordt, double *divdt, double *tdt, double *trdt);
enum { SPDY_STEP_MAX_OPS = 8 };
typedef struct {
    int nlev;
    double *field, *fdt;
} spdy_step_op;
int spdy_step_fields_dev(spdy_plan *plan, int nops, const spdy_step_op *ops, int j1, double dt, double eps, double wil);
int spdy_step_field(spdy_plan *plan, int nlev, int j1, double dt, double eps, double wil, double *field, double *fdt);

/* ---- grid-space dynamical tendencies (tendencies.f90:105-197) --------------------------------------
 * Closes the loop inverse batch -> nonlinear terms -> direct batch on the device: from the gridded prognostics of time
 * level j2 (ug, vg, tg, vorg, divg, trg: (ix,il,kx) each, exactly what spdy_inverse_batch_dev produced -- vorg without
 * the Coriolis term, it is added here) and px, py = spec_to_grid(grad(ps), 2) it computes the vertical means, the
 * sigma-dot velocities and every grid tendency, laid out as the operands of ONE spdy_direct_batch_dev launch:
 *     u_out, v_out [3 kx] : (utend, vtend) | (-ug*tgg, -vg*tgg) | (-ug*trg, -vg*trg)
 *     plain_out [3 kx+1]  : 0.5*(ug^2+vg^2) | ttend | trtend | -umean*px - vmean*py
 * A host with physics adds its tendencies to utend, vtend, ttend, trtend in place before the direct batch
 * (tendencies.f90:203-206).  After the direct batch (pvor, pdiv [3 kx] from the pairs, pspec [3 kx + 1] from the plain
 * fields) spdy_tendency_combine_dev finishes tendencies.f90:125-126, 218-233 in place: pdiv[0:kx] -= laplacian(pspec[0:kx]),
 * pdiv[kx:3kx] += pspec[kx:3kx], pspec[3kx](1,1) = 0 -- so vordt = pvor[0:kx], divdt = pdiv[0:kx], tdt = pdiv[kx:2kx],
 * trdt = pdiv[2kx:3kx], psdt = pspec[3kx] are views, no copies.                                                     */
int spdy_grid_tendencies_dev(spdy_plan *plan, const double *ug, const double *vg, const double *tg, const double *vorg,
                             const double *divg, const double *trg, const double *px, const double *py, double *u_out,
                             double *v_out, double *plain_out);
int spdy_tendency_combine_dev(spdy_plan *plan, double *pdiv, double *pspec);
/* Everything after the direct batch in ONE launch (kx <= 16; the separate kernels otherwise): spdy_tendency_combine_dev,
 * spdy_spectral_tendencies_dev, spdy_implicit_terms_dev, spdy_hdiff_step_dev and spdy_step_fields_dev of ps, vor, div, t, tr.
 * Same expressions in the same order as the separate kernels; the results agree with them to rounding (the compiler is free
 * to contract a*b+c differently in the two translation contexts), not necessarily bit for bit.  pvor/pdiv/pspec: the direct batch's outputs (the final, truncated tendencies are left in
 * them); vor, div, t, tr: (mx,nx,kx,2), ps: (mx,nx,2) -- time level 1 feeds the spectral tendencies and the diffusion, as
 * in the reference's leapfrog step (tendencies.f90:34-38 with alph >= 0.5, time_stepping.f90:63-96).                    */
int spdy_spectral_step_dev(spdy_plan *plan, double *pvor, double *pdiv, double *pspec, double *vor, double *div, double *t,
                           double *tr, double *ps, const double *phis, const double *d_tcorh, const double *d_qcorh, double sdrag,
                           int j1, double dt, double eps, double wil, double *phi);
/* spdy_direct_batch_dev(3 kx pairs ug, vg -> pvor, pdiv; 3 kx + 1 plain fields d_grid -> pspec) followed by
 * spdy_spectral_step_dev, as ONE call: the second half of a time step (tendencies.f90:212-234, :242-293,
 * implicit.f90:168-217, time_stepping.f90:62-167).  At T30 exactly those two calls; at T63, where vds is not part of the
 * transform kernel, the pairs' spectra stay in the plan's temporaries and vds (spectral.f90:146-171) is applied where the
 * spectral step reads them: 2 launches instead of 3.  pvor, pdiv, pspec receive the truncated tendencies as with the
 * separate calls; results agree with them to rounding.  Checks, in this order: the plan and its device; what the spectral
 * step needs (spdy_implicit_init, sigma levels) SPDY_ERR_STATE; a NULL pointer, then j1 outside {1, 2} SPDY_ERR_ARG; only
 * then the direct batch's own (max_batch) -- a call that fails enqueues nothing.                                      */
int spdy_direct_batch_spectral_step_dev(spdy_plan *plan, const double *d_ug, const double *d_vg, const double *d_grid, int kcos,
                                        double *pvor, double *pdiv, double *pspec, double *vor, double *div, double *t, double *tr,
                                        double *ps, const double *phis, const double *d_tcorh, const double *d_qcorh, double sdrag,
                                        int j1, double dt, double eps, double wil, double *phi);

/* ---- ensemble time step: nmem model states through ONE step's launches ---------------------------------
 * A T30 L8 step is four or five launches, each bound by its fixed costs, not by bytes: an ensemble amortises them.  An ensemble
 * array is the single-state array with every level dimension kx widened to nmem*kx, member-major inside it:
 *     vor, div, t, tr  (mx,nx,kx,nmem,2)   ps (mx,nx,nmem,2)     time level lv of all members = one stack of nmem*kx fields
 *     phis, d_tcorh, d_qcorh (mx,nx)       shared by all members; with the plan option "ens_member_qcorh" d_qcorh is (mx,nx,nmem)
 *     phi              (mx,nx,kx,nmem)
 *     ug, vg, tg, vorg, divg, trg (ix,il,kx,nmem)                px, py (ix,il,nmem)
 *     u_out, v_out, pvor, pdiv  [3][nmem][kx]                    group-major: the group stride is nmem*kx fields
 *     plain_out, pspec          [3][nmem][kx] + [nmem]           the level-free fields of the members behind the three groups
 * so the transforms are the existing calls with larger counts (inverse: nmem*kx pairs, plain segments of nmem*kx, nmem gradient
 * fields; direct: 3*nmem*kx pairs, 3*nmem*kx + nmem plain fields), and utend, vtend, ttend, qtend of all members -- the first
 * nmem*kx fields of u_out, v_out and the second and third group of plain_out -- are nmem states back to back as the column physics
 * takes them.  Member e of the column kernels works on level slot e*kx + k, its level-free slot is 3*nmem*kx + e.  The kernels are
 * those of the single-state calls with the member in blockIdx.y: same expressions, same order, and with nmem = 1 the same
 * addresses, so a member's results do not depend on the ensemble it travels in wherever the transforms' do not (T30: bit for
 * bit; T63: the pairs' spectra to rounding where the launch form differs, see spdy_direct_batch_spectral_step_dev).  Members are
 * fields of those batches and states of the column physics, so the contract of a batch (Conventions) holds between them: what one
 * member holds, non-finite values included, changes no bit of another member, of its radiation state, surface-model fields or
 * guard rows; a member that goes non-finite is flagged by the guard (SPDY_DIAG_NONFINITE) and the others run on.
 *   spdy_ens_grid_tendencies_dev / _spectral_step_dev / _geopotential_dev   the single-state calls for nmem members, one launch
 *   spdy_ens_direct_batch_spectral_step_dev   ONE direct batch of all members, then the spectral step; the routes of the
 *       single-state call (T63: the raw pairs' spectra in the plan's temporaries) where the batch fits them, silently the plain
 *       direct batch followed by the spectral step otherwise
 *   spdy_ens_physics_dev   spdy_physics_dev for nmem members: ONE inverse launch of time level 1 of all members (vor .. phi
 *       (mx,nx,kx,nmem), ps (mx,nx,nmem)), then the column physics with nb = nmem; the fields of bnd, albsfc, rad_state and the
 *       optional outputs are per member, back to back, as spdy_column_physics_dev takes them.  spdy_ens_physics_workspace(nmem)
 *       allocates its workspace (not possible during a capture; a larger nmem later allocates anew).
 * Checks, in this order: a NULL plan, nmem < 1, kx > 16 with nmem > 1 (physics: kx outside [5, 16]) and
 * max_batch < nmem*(3*kx+1) SPDY_ERR_ARG; what the single-state call needs first (spdy_implicit_init, sigma levels; physics: sigma
 * levels, date, orography) SPDY_ERR_STATE; a NULL required pointer, then j1 outside {1, 2} SPDY_ERR_ARG; a host-only plan
 * SPDY_ERR_NO_DEVICE last.  Every call can be captured.  SPPT: a pattern object of nmem members and spdy_ens_physics_sppt_dev ("SPPT" below).  Not covered: the
 * sharded step.
 * A coupled ensemble needs the option "ens_member_qcorh": qcorh = grid_to_spec(corh) and corh is made from the member's own stl_am
 * and sst_am ("surface models" below), so once the members' land and sea temperatures differ no two members have the same qcorh.
 * d_tcorh depends neither on time nor on the member and stays shared.  In the kernel it is one more uniform member offset (a
 * stride of 0 or mx*nx complex); no expression changes.  The surface models and the guard of all members are one object each
 * (spdy_ens_surface_model_create, spdy_ens_diagnostics_create), one launch per call.  Order of calls of a coupled ensemble step: on
 * a day's first step forcing_dev(qcorh (mx,nx,nmem)); the step, its physics reading the model's boundary arrays and writing
 * hfluxn, shf, evap, ssrd of all members; check_dev on time level 2; the host's newdate, and set_date when the day changed;
 * couple_dev(day).                                                                                                              */
int spdy_ens_grid_tendencies_dev(spdy_plan *plan, int nmem, const double *ug, const double *vg, const double *tg, const double *vorg,
                                 const double *divg, const double *trg, const double *px, const double *py, double *u_out,
                                 double *v_out, double *plain_out);
int spdy_ens_spectral_step_dev(spdy_plan *plan, int nmem, double *pvor, double *pdiv, double *pspec, double *vor, double *div, double *t,
                               double *tr, double *ps, const double *phis, const double *d_tcorh, const double *d_qcorh, double sdrag,
                               int j1, double dt, double eps, double wil, double *phi);
int spdy_ens_direct_batch_spectral_step_dev(spdy_plan *plan, int nmem, const double *d_ug, const double *d_vg, const double *d_grid,
                                            int kcos, double *pvor, double *pdiv, double *pspec, double *vor, double *div, double *t,
                                            double *tr, double *ps, const double *phis, const double *d_tcorh, const double *d_qcorh,
                                            double sdrag, int j1, double dt, double eps, double wil, double *phi);
int spdy_ens_geopotential_dev(spdy_plan *plan, int nmem, const double *t, const double *phis, double *phi);

/* ---- multi-GPU: level-sharded time steps (one process per GPU with RCCL over xGMI, or ranks inside one process) -------
 * The transform batch shards over (field x level) with no communication.  What couples levels in a step is exchanged:
 * implicit_terms' operands (implicit.f90:174-216) with spdy_implicit_terms_sharded_dev, or -- the complete adiabatic step --
 * everything the two column kernels read, with spdy_sharded_step_dev below.
 * Rank r of n owns levels [nlev*r/n, nlev*(r+1)/n) (spdy_comm_level_range).  RCCL ranks: rank 0 obtains an id with
 * spdy_comm_unique_id and hands the SPDY_COMM_ID_BYTES bytes to the other ranks by whatever means the host has
 * (MPI_Bcast, a file, torch.distributed); then every rank calls spdy_comm_create.  Collectives run on the plan's
 * stream and can be captured into a graph.  RCCL is loaded on first use.                                        */
typedef struct spdy_comm spdy_comm;
enum { SPDY_COMM_ID_BYTES = 128, SPDY_COMM_MAX_ARRAYS = 16 };
int spdy_comm_unique_id(char *id);
int spdy_comm_create(spdy_plan *plan, int nranks, int rank, const char *id, spdy_comm **comm);
int spdy_comm_destroy(spdy_comm *comm);
int spdy_comm_level_range(const spdy_comm *comm, int nlev, int *lo, int *hi);
/* Ranks INSIDE one process -- a single-process host (the reference is one: speedy.f90:24-54) that drives several GPUs, one
 * host thread and one plan per GPU; also how the multi-rank paths are tested on a 1-GPU box (several plans on one device).
 * No RCCL: a collective blocks its calling thread until every rank of the group has entered it and moves the blocks with
 * device-to-device / peer copies on the ranks' own streams.  The calls of different ranks must come from different threads;
 * a rank missing for $SPDY_COMM_TIMEOUT_S (default 120) seconds breaks the group (SPDY_ERR_COMM) instead of hanging it.
 * Not graph-capturable (SPDY_ERR_STATE inside a capture).  Everything else -- level ranges, spdy_allgather_levels_dev, the
 * sharded step -- is the same code as with RCCL ranks.                                                                 */
typedef struct spdy_comm_group spdy_comm_group;
int spdy_comm_group_create(int nranks, spdy_comm_group **group);
int spdy_comm_group_destroy(spdy_comm_group *group);      /* after the group's communicators (SPDY_ERR_STATE otherwise) */
int spdy_comm_create_local(spdy_plan *plan, spdy_comm_group *group, int rank, spdy_comm **comm);
/* in place: d_full[i] are narr <= SPDY_COMM_MAX_ARRAYS full (mx,nx,nlev) stacks in which this rank has filled its own level block */
int spdy_allgather_levels_dev(spdy_comm *comm, int nlev, int narr, double *const *d_full);
/* all-gather of the level blocks of divdt and tdt, then implicit_terms on the full columns (every rank).  psdt must already be
 * the complete surface-pressure tendency on every rank -- true for implicit_terms called on its own, NOT inside a level-sharded
 * step, where get_spectral_tendencies (tendencies.f90:256-263) first sums the divergence of all levels into it.        */
int spdy_implicit_terms_sharded_dev(spdy_comm *comm, double *divdt, double *tdt, double *psdt);

/* The COMPLETE adiabatic time step with the transforms sharded by level (BASELINE config 3).  Lines of the reference that couple
 * levels: get_grid_point_tendencies' vertical means, sigma-dot sums and half-level fluxes (tendencies.f90:109-197),
 * get_spectral_tendencies' dmean / sigma-dot sums and psdt -= dmean (:256-285), the hydrostatic integration
 * (geopotential.f90:33-57), implicit_terms (implicit.f90:174-216).  Rank r runs the inverse and the direct transforms of ITS
 * levels only; the two column kernels run on full columns on every rank, each behind ONE in-place all-gather:
 *     inverse batch (own levels of time level j2; + grad(ps), level-free and replicated)  ->  all-gather of the gridded
 *     prognostics (6 kx grids)  ->  grid tendencies (full columns in, own levels' direct-batch operands out)  ->  direct batch
 *     (own levels; + the level-free ps tendency)  ->  all-gather of the spectral tendencies (9 kx + nranks spectra)  ->
 *     spectral step on full columns: tendency combination, get_spectral_tendencies, implicit_terms, diffusion, leapfrog.
 * Every rank holds the full prognostic state (vor, div, t, tr: (mx,nx,kx,2); ps: (mx,nx,2)) before and after; no rank reads a
 * level of an intermediate field that it neither computed nor received.  The exchanged stacks are stored block by block, one
 * contiguous block per rank (csrc/spdy_kernels.hpp: LevelShard), in workspace the communicator owns
 * (spdy_sharded_step_workspace: allocate before a graph capture).  kx <= 16, nranks <= kx, max_batch >= 4 kx + 2.
 * Results: the transforms are position-independent and the column kernels evaluate the unsharded kernels' expressions, so the
 * step agrees with spdy_inverse_batch_segs_dev + spdy_grid_tendencies_dev + spdy_direct_batch_spectral_step_dev to rounding
 * (in practice bit for bit, tests/test_gpu_sharded_step.py) for every rank count.
 *   spdy_sharded_step_dev          the whole step; tend_out (4 kx + 1 spectra: vordt | divdt | tdt | trdt | psdt, truncated, as
 *                                  step_field_* leaves them) may be NULL
 *   spdy_sharded_step_grid_dev     first half, up to the grid tendencies ...
 *   spdy_sharded_step_operands     ... whose results -- this rank's levels [lo, hi): u, v [3 nl], plain [3 nl + 1] grids laid
 *                                  out as spdy_grid_tendencies_dev documents, with nl for kx -- a host with physics updates in
 *                                  place (tendencies.f90:203-206) before ...
 *   spdy_sharded_step_spectral_dev ... the second half
 *   spdy_sharded_step_stacks       the two exchanged stacks (tests poison them between steps)                              */
int spdy_sharded_step_workspace(spdy_comm *comm);
int spdy_sharded_step_dev(spdy_comm *comm, double *vor, double *div, double *t, double *tr, double *ps, const double *phis,
                          const double *d_tcorh, const double *d_qcorh, double sdrag, int j1, int j2, double dt, double eps, double wil,
                          double *phi, double *tend_out);
int spdy_sharded_step_grid_dev(spdy_comm *comm, double *vor, double *div, double *t, double *tr, double *ps, int j2);
int spdy_sharded_step_operands(spdy_comm *comm, double **u, double **v, double **plain, int *lo, int *hi);
int spdy_sharded_step_spectral_dev(spdy_comm *comm, double *vor, double *div, double *t, double *tr, double *ps, const double *phis,
                                   const double *d_tcorh, const double *d_qcorh, double sdrag, int j1, double dt, double eps, double wil,
                                   double *phi, double *tend_out);
int spdy_sharded_step_stacks(spdy_comm *comm, double **grid_stack, size_t *grid_doubles, double **spec_stack, size_t *spec_doubles);
/* The TRANSPOSED form of the same step (spdy_comm_set_option(comm, "transpose", 1), or $SPDY_SHARD_TRANSPOSE=1 when the
 * communicator is created; the all-gather form above stays the default).  Instead of gathering whole stacks and running the
 * two column kernels redundantly on every rank, the ranks TRANSPOSE: the grid-space column kernel is coupled in the vertical
 * but independent in the horizontal (tendencies.f90:109-197), the spectral step independent per coefficient
 * (tendencies.f90:242-293, implicit.f90:168-217) -- so rank r runs them for ALL levels of ITS share of the grid points /
 * coefficients (contiguous ranges in units of 16):
 *     inverse batch (own levels)  ->  exchange 1: levels -> point ranges (6 kx slabs)  ->  grid tendencies, all levels of the own
 *     points  ->  exchange 2 back: every rank's direct-batch operands come home (9 nl + 1 grids)  ->  direct batch incl. vds (own
 *     levels)  ->  exchange 3: levels -> coefficient ranges (9 kx + nranks slabs)  ->  spectral step, all levels of the own
 *     coefficients  ->  exchange 4 back (time level j2 of the own levels; ps whole), issued at the START of the next grid half.
 * Each exchange is one grouped ncclSend / ncclRecv per peer on the plan's stream (in-process groups: 2-D peer copies).  Per rank
 * and step it receives (R - 1) / R of 6 nl + 9 nl + 1 grids and 9 nl + 1 + 4 nl + 1 spectra -- a third of the all-gather form's
 * bytes at 8 ranks (spdy_comm_describe prints both) -- and does 1 / R of the column kernels' work.  Same kernels' expressions
 * on the same values: bit-identical to the all-gather form and to the unsharded step at T30, equal to rounding (1e-13) at T63,
 * where vds is applied before exchange 3 and the bits of the staged T63 direct batch's vdspec depend on the batch size
 * (tests/test_gpu_sharded_step.py).
 * STATE: nothing is replicated any more.  After a transposed step the caller's prognostic arrays are current on (all levels x
 * own coefficients) only (with one rank: whole, unless $SPDY_COMM_FORCE).  Every transposed spdy_sharded_step_grid_dev, eager or
 * captured, first completes what it reads IN PLACE in the caller's arrays (exchange 4: on a whole state it moves values that are
 * already there), and spdy_sharded_state_gather_dev makes them whole on every rank (output, restart, switching the form; eager
 * only, SPDY_ERR_STATE inside a capture).  Switching back to the all-gather form (spdy_comm_set_option "transpose" 0) needs an
 * eager spdy_sharded_state_gather_dev after the last eager transposed step, and is refused for good (SPDY_ERR_STATE: create a
 * new communicator) once a transposed step of the communicator has been recorded into a graph, whose replays leave the state
 * range-sharded whatever the host has called since.  phi and tend_out are written on the own coefficients;
 * spdy_sharded_gather_ranges_dev completes any such array (rows of mx nx complex values; <= 4 kx + 2 rows).  The physics hook
 * (spdy_sharded_step_operands between the two halves) is unchanged.                                                         */
int spdy_comm_set_option(spdy_comm *comm, const char *name, int value);      /* "transpose" 0 | 1; "force", "dry" as $SPDY_COMM_FORCE / _DRY */
int spdy_sharded_state_gather_dev(spdy_comm *comm, double *vor, double *div, double *t, double *tr, double *ps);
int spdy_sharded_gather_ranges_dev(spdy_comm *comm, int narr, double *const *arrays, const int *nrows);
/* One line of JSON about the communicator: route ("rccl" with the path of the librccl the symbols were bound from -- a host
 * process that carries two RCCL builds is a known source of hangs -- or the in-process group), rank / ranks, form, this rank's
 * levels / points / coefficients, bytes received per step in either form.                                                   */
int spdy_comm_describe(spdy_comm *comm, char *buf, int len);

/* ---- fused operator + transform sequences (device-resident; extensions of the reference interface) ------
 * The reference's callers always follow uvspec by two spec_to_grid(.,2) (tendencies.f90:98-100, physics.f90:96-98)
 * and grad by two spec_to_grid(.,2) (tendencies.f90:121-123).  These entry points do each sequence in one pass:
 * the operator is applied while the spectra are staged for the inverse transform, so the intermediate spectra
 * never exist in memory.  Results equal spdy_uvspec_dev / spdy_grad_dev followed by spdy_spec_to_grid_dev.
 *   spdy_uvspec_to_grid_dev : (vor, div)[nb] -> ug, vg [nb] grids     (spectral.f90:173-196 + :98-110)
 *   spdy_grad_to_grid_dev   : psi[nb]        -> gx, gy [nb] grids     (spectral.f90:124-144 + :98-110)          */
int spdy_uvspec_to_grid_dev(spdy_plan *plan, int nb, const double *d_vor, const double *d_div, double *d_ug, double *d_vg,
                            int kcos);
int spdy_grad_to_grid_dev(spdy_plan *plan, int nb, const double *d_psi, double *d_gx, double *d_gy, int kcos);
/* One model step's whole direct batch in one launch (tendencies.f90:212-234: vdspec of 3*kx (u,v) pairs next to
 * grid_to_spec of the remaining fields): at these sizes every launch costs its ~10 us pipeline latency, whatever it
 * carries.  Equals spdy_vdspec_dev(npairs, ...) followed by spdy_grid_to_spec_dev(nplain, ...); the two groups must
 * not overlap in memory.                                                                                       */
/* ... and its whole inverse batch (tendencies.f90:89-107: uvspec + two spec_to_grid(.,2) per level next to the
 * spec_to_grid of the other fields).  Equals spdy_uvspec_to_grid_dev(npairs, ..., kcos_pairs) followed by
 * spdy_spec_to_grid_dev(nplain, d_spec, d_kcos, kcos_all, d_grid).                                          */
int spdy_inverse_batch_dev(spdy_plan *plan, int npairs, const double *d_vor, const double *d_div, double *d_ug, double *d_vg,
                           int kcos_pairs, int nplain, const double *d_spec, const int *d_kcos, int kcos_all, double *d_grid);
int spdy_direct_batch_dev(spdy_plan *plan, int npairs, const double *d_ug, const double *d_vg, double *d_vorm,
                          double *d_divm, int kcos, int nplain, const double *d_grid, double *d_spec);
/* spdy_inverse_batch_dev followed by spdy_grad_to_grid_dev(ngrad, d_psi, d_gx, d_gy, kcos_grad) -- everything
 * get_grid_point_tendencies transforms to the grid before its level loops (tendencies.f90:89-107 and the grad(ps) /
 * spec_to_grid(.,2) pair of :121-123).  One launch at T30 (gradient tiles ride along in the mixed kernel); at T63 the
 * five groups of spectra are one fused launch behind the two operator kernels (a lone gradient is a one-workgroup
 * launch of a full pipeline latency).  npairs + ngrad <= max_batch for the one-launch T63 form.                                                                                                */
int spdy_inverse_batch_grad_dev(spdy_plan *plan, int npairs, const double *d_vor, const double *d_div, double *d_ug, double *d_vg,
                                int kcos_pairs, int nplain, const double *d_spec, const int *d_kcos, int kcos_all, double *d_grid,
                                int ngrad, const double *d_psi, double *d_gx, double *d_gy, int kcos_grad);
/* The same with the plain spectra taken from up to SPDY_MAX_SPEC_SEGS separate device arrays -- the reference reads vor, div,
 * t, tr of time level j2 straight from its four prognostic arrays (tendencies.f90:89-101), so a captured time step needs no
 * gather copy in front of this call.  Segment i contributes segs[i].nb fields; the grids of all segments are ONE stack
 * d_grid (sum of nb fields, in segment order); d_kcos (optional) is indexed along that stack.  Still one launch at T30 (the
 * mixed kernel looks the source array up per field) and one fused launch at T63 (one segment of the launch each).
 * ngrad may be 0.                                                                                                  */
enum { SPDY_MAX_SPEC_SEGS = 4 };
typedef struct {
    int nb;
    const double *d_spec;
} spdy_spec_seg;
int spdy_inverse_batch_segs_dev(spdy_plan *plan, int npairs, const double *d_vor, const double *d_div, double *d_ug, double *d_vg,
                                int kcos_pairs, int nseg, const spdy_spec_seg *segs, const int *d_kcos, int kcos_all, double *d_grid,
                                int ngrad, const double *d_psi, double *d_gx, double *d_gy, int kcos_grad);
/* the same with host pointers (one H2D + one D2H round trip for a whole level stack) */
int spdy_uvspec_to_grid(spdy_plan *plan, int nb, const double *vor, const double *div, double *ug, double *vg, int kcos);
int spdy_grad_to_grid(spdy_plan *plan, int nb, const double *psi, double *gx, double *gy, int kcos);

/* ---- output path: one snapshot's fields to the grid, scaled and rounded to float32 ------------------------------
 * input_output.f90:184-206: per level uvspec + spec_to_grid(.,2) of (vor, div), spec_to_grid(.,1) of t, q (= tr(:,:,:,1,1)),
 * phi, and of ps; then u, v, t unchanged, q*1.0e-3, phi/grav, p0*exp(ps), each converted with real(., sp).  The inputs are
 * time level 1 of the device-resident prognostics ((mx,nx,kx) complex; ps (mx,nx)); the outputs are float arrays
 * (ix,il,kx) / (ix,il) ready for the host's NetCDF writer (which stays on the host).  Three launches: gather of the plain
 * spectra, ONE transform launch for all 5 kx + 1 fields, float32 epilogue.  spdy_output_workspace allocates the plan's
 * scratch (5 kx + 1 grids) ahead of time, e.g. before a graph capture; max_batch must be >= 3 kx + 1.                    */
int spdy_output_workspace(spdy_plan *plan);
int spdy_output_batch_dev(spdy_plan *plan, const double *vor, const double *div, const double *t, const double *q, const double *phi,
                          const double *ps, float *u_out, float *v_out, float *t_out, float *q_out, float *phi_out, float *ps_out);

/* ---- ensemble output: every member's snapshot, the ensemble mean and the spread, in one call ----------------
 * spdy_output_batch_dev for the nmem members of an ensemble ("ensemble time step" above: layout) and, from the same grid values,
 * the statistics an ensemble is run for.  Inputs: time level 1 of the ensemble, vor .. phi (mx,nx,kx,nmem) complex, ps
 * (mx,nx,nmem); phi is the caller's, as in the single-state call.  Outputs, float: the fields of `members` (ix,il,kx,nmem), its ps
 * (ix,il,nmem); the fields of `mean` and `spread` (ix,il,kx), their ps (ix,il).  Each of the three structs may be NULL = that
 * group is not wanted; at least one must be given, and inside a given struct all six pointers are required (8-byte aligned).
 * Per grid point, level and quantity, with x_e the FP64 value of member e -- u, v, t as they are, q * (double)1.0e-3f, phi / grav,
 * (double)1.e+5f * exp(ps), the expressions of spdy_output_batch_dev --
 *     members   (float)x_e: the bits of spdy_output_batch_dev on the same grid value; written for every member
 *     mean      (sum x_e) / n                              over the n members in use, in FP64, rounded to float at the store
 *     spread    sqrt(sum (x_e - mean)^2 / (n - 1))         the sample standard deviation; n = 1: +0; n = 0: NaN, as the mean
 * d_use: NULL = all members, or nmem ints on the device, non-zero = the member is in use.  A member not in use is skipped by a
 * select, never multiplied by zero: it may hold NaN or inf and the statistics are, bit for bit, those of the ensemble without it.
 * The spread is formed in two passes (the sum, then the squared deviations from the finished mean), sequentially in ascending
 * member order, without atomics: results are bit-reproducible, and x_e near 288 with a spread of 1e-6 loses nothing.
 * Two launches' worth of work: ONE inverse batch of all members (nmem*kx pairs, the segments t | q | phi of nmem*kx fields and ps
 * of nmem, read in place: no gather copy) into the workspace of (5 kx + 1) nmem grids, then one epilogue kernel.
 * spdy_ens_output_workspace(nmem) allocates the workspace (not possible during a capture; a larger nmem later allocates anew);
 * the call itself can be captured.  Checks, in this order: a NULL plan, nmem < 1, max_batch < nmem*(3*kx+1) SPDY_ERR_ARG; a NULL
 * required pointer or no output group SPDY_ERR_ARG; a host-only plan SPDY_ERR_NO_DEVICE last.  A failing call enqueues nothing. */
typedef struct {                      /* one group of output fields: device pointers, all six required                          */
    float *u, *v, *t, *q, *phi;       /* (ix,il,kx), as `members` (ix,il,kx,nmem)                                               */
    float *ps;                        /* (ix,il), as `members` (ix,il,nmem)                                                     */
} spdy_output_fields;
int spdy_ens_output_workspace(spdy_plan *plan, int nmem);
int spdy_ens_output_batch_dev(spdy_plan *plan, int nmem, const double *vor, const double *div, const double *t,
                              const double *q, const double *phi, const double *ps, const int *d_use,
                              const spdy_output_fields *members, const spdy_output_fields *mean,
                              const spdy_output_fields *spread);

/* ---- pressure-level output: every member's fields on pressure surfaces, their ensemble mean and spread ------
 * The fields people read and verify are on pressure surfaces; the reference's post-processing (scripts/sigma_to_pressure.py) runs,
 * per column of a snapshot, np.interp(p_levels, ps/100 * sigma, field).  This is that product from the device-resident ensemble in
 * one capturable call, and the mean and spread ON the pressure levels -- which are not the interpolation of the sigma-level mean
 * and spread: each member has its own surface pressure and so its own bracket.
 * Inputs: those of spdy_ens_output_batch_dev (time level 1 of nmem members, phi, ps, d_use), and
 *     nlev   the number of pressure levels, 1 <= nlev <= SPDY_MAX_PLEV
 *     plev   nlev pressures in Pa on the HOST, each finite and > 0, in any order; read when the call is enqueued (a captured call
 *            keeps its values)
 *     coord  SPDY_PLEV_LINEAR_P: linear in p, the reference script's choice; SPDY_PLEV_LOG_P: linear in ln p
 * Per member e, grid point and quantity x -- u, v, t, q * (double)1.0e-3f, phi / grav: the FP64 values x_e[k] the ensemble output
 * forms before its float rounding, on the full levels k = 0 .. kx-1 (fsg ascending) -- the coordinate of the model levels and of
 * the target is
 *     linear   X_k = ((double)1.e+5f * exp(ps_e)) * fsg[k]      x = plev[l]
 *     log      X_k = ps_e + ln fsg[k]                           x = ln(plev[l] / (double)1.e+5f)      (logarithms formed on the host)
 * and the value on the level follows np.interp:
 *     x <= X_0        x_e[0]      (that level's bits, not an arithmetic result)
 *     x >= X_{kx-1}   x_e[kx-1]   (likewise)
 *     otherwise       the k with X_k <= x < X_{k+1}:  w = (x - X_k) / (X_{k+1} - X_k),  y_e = x_e[k] + w * (x_e[k+1] - x_e[k])
 * each operation rounded once, without contraction; kx = 1: every level gets x_e[0].  A member whose ps_e is not finite gets NaN on
 * every level (no loop bound and no address depends on ps_e).
 * Outputs, float, the three optional groups of the ensemble output: the fields of `members` u .. phi (ix,il,nlev,nmem), its ps
 * (ix,il,nmem); of `mean` and `spread` u .. phi (ix,il,nlev), ps (ix,il).  Mean and spread are formed over the members in use from
 * the y_e in FP64 exactly as the ensemble output forms them from x_e: two passes, ascending member order, a select and never a
 * multiplication for a member not in use, n = 1 gives +0, n = 0 NaN.  The three ps fields are the surface pressure, with the bits
 * of spdy_ens_output_batch_dev's.  `below` (ix,il,nlev), float, or NULL = not wanted: the number of members in use for which
 * x > X_{kx-1} -- the level lies below that member's lowest model level and its value there is the clamped one: what a user masks
 * with.  All output pointers 8-byte aligned.
 * spdy_ens_output_pressure_dev: the ensemble output's inverse batch into its workspace, then ONE kernel; capturable after
 * spdy_ens_output_workspace(plan, nmem).  spdy_ens_output_pressure_grid_dev: that kernel alone on the caller's device array `grid`
 * of (5 kx + 1) nmem FP64 grids in the workspace's layout -- u | v | t | q | phi with nmem*kx grids each, member-major, then ps with
 * nmem grids -- holding the model's raw values as the inverse batch leaves them (q in g/kg, phi in m2/s2, ps as log(p/p0)); 16-byte
 * aligned; no max_batch check (it runs no transform).  spdy_output_pressure_dev: the single state, which is the one-member case of
 * the ensemble call with the `members` group only (as every single-state step call is the one-member case of its ensemble call).
 * Checks, in this order: a NULL plan, nmem < 1, max_batch < nmem*(3*kx+1) SPDY_ERR_ARG; nlev outside [1, SPDY_MAX_PLEV], a NULL
 * plev, a level that is not finite or not > 0, an unknown coord SPDY_ERR_ARG; no sigma levels SPDY_ERR_STATE; a NULL required
 * pointer, no output group, an output pointer not 8-byte aligned SPDY_ERR_ARG; a host-only plan SPDY_ERR_NO_DEVICE last.  A
 * failing call enqueues nothing and sets the text of spdy_last_error.                                                            */
enum { SPDY_MAX_PLEV = 32, SPDY_PLEV_LINEAR_P = 0, SPDY_PLEV_LOG_P = 1 };
int spdy_ens_output_pressure_dev(spdy_plan *plan, int nmem, const double *vor, const double *div, const double *t,
                                 const double *q, const double *phi, const double *ps, const int *d_use, int nlev,
                                 const double *plev, int coord, const spdy_output_fields *members,
                                 const spdy_output_fields *mean, const spdy_output_fields *spread, float *below);
int spdy_ens_output_pressure_grid_dev(spdy_plan *plan, int nmem, const double *grid, const int *d_use, int nlev,
                                      const double *plev, int coord, const spdy_output_fields *members,
                                      const spdy_output_fields *mean, const spdy_output_fields *spread, float *below);
int spdy_output_pressure_dev(spdy_plan *plan, const double *vor, const double *div, const double *t, const double *q,
                             const double *phi, const double *ps, int nlev, const double *plev, int coord, float *u_out,
                             float *v_out, float *t_out, float *q_out, float *phi_out, float *ps_out);

/* Column physics (spdy_moist_columns_dev, spdy_moist_physics_dev, spdy_radiation_down_dev, spdy_radiation_up_dev,
 * spdy_surface_fluxes_dev, spdy_pbl_dev, spdy_column_physics_dev, spdy_physics_dev) checks its arguments in one order, and the first check that
 * fails gives the code: a NULL plan, kx outside [5, 16] and nb outside [0, max_batch] SPDY_ERR_ARG; no sigma levels, then
 * (radiation, the chain) no date, then (surface fluxes, the chain) no orography, SPDY_ERR_STATE; a NULL required pointer
 * SPDY_ERR_ARG; then the call's own conditions (spdy_moist_physics_dev, spdy_physics_dev: max_batch); a host-only plan SPDY_ERR_NO_DEVICE last. */

/* ---- column physics: the precipitation block of get_physical_tendencies (physics.f90:110-138) ----------------------------
 * Replaces, on the device, the thermodynamic fields (physics.f90:110-115: psg = exp(pslg), rps, qg = max(qg, 0), se = cp*tg +
 * phig), spec_hum_to_rel_hum per level (:117-119; humidity.f90:16-28, 46-79), deep convection (:126; convection.f90:26-235), the
 * scaling of the convective fluxes for k >= 2 (:128-131), icnv = kx - iptop (:133), large-scale condensation (:136;
 * large_scale_condensation.f90:32-83) and ttend = ttend + tt_cnv + tt_lsc, qtend = qtend + qt_cnv + qt_lsc (:138-139).  A host
 * "with physics" calls it between spdy_grid_tendencies_dev and the direct batch (tendencies.f90:203-206).  The blocks that follow
 * it in get_physical_tendencies have device forms of their own below (radiation, surface fluxes, boundary layer, and SPPT,
 * physics.f90:208-222, which is off in the reference's params.f90).
 * One thread per column; 5 <= kx <= 16 (SPDY_ERR_ARG otherwise), sigma levels as for the geopotential (SPDY_ERR_STATE without).
 * Results follow the reference's order of operations without contraction: decisions (convection or not, its top, condensation)
 * are the reference's wherever no decision is within rounding of its threshold.  Both calls can be captured in a graph; `out` is
 * read at call time.  The tables the block uses are spdy_get_table's sigl sigh grdsig grdscp wvi entr (physics.f90:12-39,
 * convection.f90:63-71).                                                                                                        */
typedef struct {                      /* per state; any member may be NULL = not written; nb states back to back            */
    double *precnv, *precls, *cbmf;   /* (ix,il)                                                                            */
    int *iptop, *icnv;                /* (ix,il): iptop after condensation, icnv before it (kx - iptop; -1 = no convection)   */
    double *qsat, *rh, *se;           /* (ix,il,kx)                                                                         */
} spdy_moist_out;
/* Gridded inputs of nb <= max_batch states (tg, qg, phig (ix,il,kx), pslg (ix,il) each); ttend / qtend (ix,il,kx) are updated in
 * place.  Inputs are not modified (the clamp of qg is local, as in the reference).                                                */
int spdy_moist_columns_dev(spdy_plan *plan, int nb, const double *tg, const double *qg, const double *phig,
                           const double *pslg, double *ttend, double *qtend, const spdy_moist_out *out);
/* One model state from its spectra -- time level 1 as get_grid_point_tendencies passes it (tendencies.f90:203-204): t, q =
 * tr(:,:,:,1,1), phi (the geopotential of t(:,:,:,1), spdy_geopotential_dev), ps (mx,nx).  ONE inverse launch of the 3 kx + 1 plain
 * fields (the four-segment inverse path, kcos 1, physics.f90:102-107 for the fields this block reads) into plan workspace, then the
 * column kernel.  ttend / qtend are the operands spdy_grid_tendencies_dev documents (plain_out[kx:2kx], [2kx:3kx]).  max_batch >=
 * 3 kx + 1.  spdy_moist_workspace allocates the workspace ((3 kx + 1) grids) ahead of time, e.g. before a graph capture.        */
int spdy_moist_workspace(spdy_plan *plan);
int spdy_moist_physics_dev(spdy_plan *plan, const double *t, const double *q, const double *phi, const double *ps,
                           double *ttend, double *qtend, const spdy_moist_out *out);

/* ---- column physics: radiation (physics.f90:146-166 and :180-186) -----------------------------------------------------------
 * The reference splits radiation in two halves with the surface fluxes between them, and so does the device: the DOWN half
 * (compute_sw set: gse, clouds with qcloud = qa(:,:,kx-1), the shortwave fluxes, tt_rsw = dfabs*rps*grdscp and the longwave
 * transmissivities tau2 / stratc; always: the downward longwave fluxes) and the UP half (the upward longwave fluxes from the
 * caller's surface temperature ts and surface emission fsfcu = slru(:,:,3), tt_rlw = dfabs*rps*grdscp, then
 * ttend = (ttend + tt_rsw) + tt_rlw in place).  A host with physics calls spdy_moist_columns_dev, the down half, the surface
 * fluxes (spdy_surface_fluxes_dev, which read ssrd and slrd and give ts and fsfcu), then the up half.
 * What the reference keeps in module state (tau2, stratc, flux) is the caller's RADIATION STATE: device memory of
 * nb * spdy_radiation_state_size(plan) doubles, one block per model state, kept across steps (and graph replays).  The first
 * call on a state must have compute_sw = 1, as the reference's first step has (mod(1, nstrad) == 1).  On steps without
 * shortwave the reference reads tt_rsw uninitialised (a local array without save); the device holds the last shortwave call's
 * tt_rsw in the state instead, as ssrd, ssr, tsr and tau2 are held -- a documented deviation.
 * Boundary fields: spdy_radiation_set_date makes the zonal forcing of a date (get_zonal_average_fields + solar,
 * shortwave_radiation.f90:238-329) -- on a device plan it also copies them into plan memory, stream-ordered on the plan's
 * stream, so a captured graph picks up a new date on its next replay (not callable during a capture).  Per column the caller
 * passes the land fraction fmask and the surface albedo albsfc (spdy_rad_surface).
 * Inputs: tg, qg, phig (ix,il,kx), pslg (ix,il) as for spdy_moist_columns_dev (qg is clamped locally), and the moist block's
 * rh (ix,il,kx), precnv, precls (ix,il) and iptop (int, ix,il); rh / precnv / precls / iptop / sfc are read with compute_sw
 * only and may be NULL otherwise.  fband(nint(T)) is indexed with the index clamped to [100, 400], so any temperature is safe.
 * Checks: kx outside [5, 16] SPDY_ERR_ARG; no sigma levels or no date set SPDY_ERR_STATE; a NULL required pointer with nb > 0
 * SPDY_ERR_ARG; a host-only plan SPDY_ERR_NO_DEVICE.  Both halves can be captured in a graph; `out` is read at call time.    */
typedef struct {                      /* per state, (ix,il) each, nb states back to back                                      */
    const double *fmask, *albsfc;     /* land fraction [0, 1], surface albedo                                                  */
} spdy_rad_surface;
typedef struct {                      /* per state; any member may be NULL = not written                                      */
    double *cloudc, *clstr;           /* (ix,il) clouds: total and stratiform cover      -- compute_sw calls only             */
    int *icltop;                      /* (ix,il) cloud top level (kx + 1 = none)           -- compute_sw calls only             */
    double *ssrd, *ssr, *tsr;         /* (ix,il) shortwave: surface down, surface net, top net -- compute_sw calls only (held)  */
    double *slrd, *slr, *olr;         /* (ix,il) longwave: surface down (down half), surface net up and outgoing (up half)      */
    double *tt_rsw, *tt_rlw;          /* (ix,il,kx) heating rates: tt_rsw on compute_sw down calls, tt_rlw on up calls        */
} spdy_rad_out;
int spdy_radiation_set_date(spdy_plan *plan, double tyear);   /* tyear: fraction of the year, 0 = 1 January 0h                */
int spdy_radiation_state_size(const spdy_plan *plan);        /* doubles per model state (> 0), or an SPDY_ERR code          */
int spdy_radiation_down_dev(spdy_plan *plan, int nb, int compute_sw, const double *tg, const double *qg, const double *phig,
                            const double *pslg, const double *rh, const double *precnv, const double *precls, const int *iptop,
                            const spdy_rad_surface *sfc, double *state, const spdy_rad_out *out);
int spdy_radiation_up_dev(spdy_plan *plan, int nb, const double *tg, const double *pslg, const double *ts, const double *fsfcu,
                          double *state, double *ttend, const spdy_rad_out *out);

/* ---- column physics: surface fluxes (physics.f90:169-170) and the boundary layer (:193-205) ---------------------------------
 * spdy_surface_fluxes_dev is get_surface_fluxes with lfluxland = .true. (surface_fluxes.f90:97-295) between the radiation halves:
 * it reads the down half's ssrd / slrd, the winds and the lowest two levels, and writes what the up half needs -- ts (= tsfc) and
 * fsfcu (= slru(:,:,3)) -- and flux3, the four averaged fluxes ustr3 vstr3 shf3 evap3 (4 (ix,il) fields per state) that
 * spdy_pbl_dev reads.  spdy_pbl_dev is get_vertical_diffusion_tend (vertical_diffusion.f90:57-142: shallow convection, moisture
 * diffusion where sigh(k) > 0.5, damping of super-adiabatic lapse rates) on the moist block's se, rh, qsat and icnv, then the
 * surface-flux tendencies of level kx and utend += ut_pbl, vtend += vt_pbl, ttend += tt_pbl, qtend += qt_pbl in place
 * (physics.f90:197-205).  ut_pbl / vt_pbl are zero above level kx, so utend / vtend are read and written at level kx only (the
 * reference's + 0.0 elsewhere changes no bit but the sign of a -0.0).  It follows the up half: the reference sums
 * (ttend + tt_rsw) + tt_rlw before + tt_pbl.
 * SPPT (physics.f90:208-222; sppt_on is .false. in params.f90) is the spdy_*_sppt_dev form of the chain, below ("SPPT").
 * Not built: the second get_surface_fluxes call
 * (sea_coupling_flag > 0, lfluxland = .false.: the reference's sea model stops for those flags and that path reads ks unset).
 * Reproduced as the reference has them: fhum0 = 0, so q1 = qa(:,:,kx) and the relative humidity is never read (rh is no argument
 * of the surface call); hfluxn(:,:,2) = .. - slru + shf + alhc*evap; t0 computed twice; ftemp0*t1 + gtemp0*t2 evaluated.
 * Boundary fields per column: spdy_sfc_boundary (the land model's stl_am / soilw_am, the sea model's sst_am, mod_radcon's snowc,
 * alb_l, alb_s).  spdy_surface_set_orography takes the surface geopotential phis0 (host, (ix,il)), keeps it and forog
 * (set_orog_land_sfc_drag, surface_fluxes.f90:300-309; spdy_get_table "phis0", "forog") in plan memory, copied on the plan's
 * stream like the fields of spdy_radiation_set_date (not callable during a capture); without it the surface call is
 * SPDY_ERR_STATE.  The level tables of the vertical diffusion are spdy_get_table's vd_scalars (cshc cvdi fshcq fshcse fvdiq
 * fvdise), vd_rsig, vd_rsig1, vd_drh0, vd_fvdiq2 (kx each; vd_drh0 / vd_fvdiq2 entry k-1 belong to the levels k, k+1).
 * spdy_column_physics_dev is the whole of physics.f90:110-205 on gridded states: the five calls in the reference's order (moist,
 * down, surface, up, boundary layer) with the intermediates in plan workspace (spdy_column_physics_workspace allocates it ahead
 * of a capture: (3 kx + 12) grids for each of max_batch states).  A member of `out` that is set takes the place of the workspace
 * field.  ssrd is written by compute_sw calls and read by every call, so it stays where the last compute_sw call put it: the
 * workspace, or the caller's rad.ssrd, which must then be passed on the calls without shortwave too.  All calls can be captured
 * in a graph; `out` is read at call time.                                                                                       */
typedef struct {                      /* (ix,il) per state, nb states back to back, device pointers, all required              */
    const double *fmask;              /* land fraction [0, 1]                                                                  */
    const double *sst;                /* sea surface temperature (sst_am)                                                      */
    const double *stl, *soilw;        /* land surface temperature (stl_am), soil water availability (soilw_am)                 */
    const double *snowc, *alb_l, *alb_s;   /* snow cover, land and sea albedo (mod_radcon)                                     */
} spdy_sfc_boundary;
typedef struct {                      /* per state; any member may be NULL = not written                                      */
    double *ustr, *vstr, *shf, *evap, *slru;   /* (ix,il,3): land, sea, weighted by the land fraction                          */
    double *hfluxn;                   /* (ix,il,2): net heat flux into land and sea (the land and sea models' input)           */
    double *tskin, *u0, *v0, *t0;     /* (ix,il)                                                                              */
} spdy_sfc_out;
typedef struct {                      /* per state; any member may be NULL = not written                                      */
    double *ut_pbl, *vt_pbl;          /* (ix,il): level kx (zero above)                                                       */
    double *tt_pbl, *qt_pbl;          /* (ix,il,kx)                                                                           */
} spdy_pbl_out;
typedef struct {                      /* per state; any member may be NULL                                                    */
    spdy_moist_out moist;
    spdy_rad_out rad;
    spdy_sfc_out sfc;
    spdy_pbl_out pbl;
    double *ts, *fsfcu;               /* (ix,il): the surface call's required outputs                                         */
} spdy_column_physics_out;
int spdy_surface_set_orography(spdy_plan *plan, const double *phis0);
int spdy_surface_fluxes_dev(spdy_plan *plan, int nb, const double *ug, const double *vg, const double *tg, const double *qg,
                            const double *phig, const double *pslg, const double *ssrd, const double *slrd,
                            const spdy_sfc_boundary *bnd, double *ts, double *fsfcu, double *flux3, const spdy_sfc_out *out);
int spdy_pbl_dev(spdy_plan *plan, int nb, const double *qg, const double *phig, const double *pslg, const double *se,
                 const double *rh, const double *qsat, const int *icnv, const double *flux3, double *utend, double *vtend,
                 double *ttend, double *qtend, const spdy_pbl_out *out);
int spdy_column_physics_workspace(spdy_plan *plan);
int spdy_column_physics_dev(spdy_plan *plan, int nb, int compute_sw, const double *ug, const double *vg, const double *tg,
                            const double *qg, const double *phig, const double *pslg, const spdy_sfc_boundary *bnd,
                            const double *albsfc, double *rad_state, double *utend, double *vtend, double *ttend, double *qtend,
                            const spdy_column_physics_out *out);
/* The chain as ONE launch (spdy_plan_set_option "physics_fused"; csrc/spdy_column_chain.hip): one thread runs the six blocks for
 * its column with the same instructions as the five calls, so the results are the same bits.  precnv, precls, iptop, icnv, slrd,
 * ts, fsfcu and the four averaged fluxes then pass from block to block in registers and are stored only where a member of `out`
 * asks for them; se, rh, qsat go through the workspace as before, and ssrd and the radiation state are written as before.
 *
 * spdy_physics_dev is what get_grid_point_tendencies calls (tendencies.f90:203-206; physics.f90:94-205): ONE model state from the
 * spectra of time level 1 -- vor, div, t, q = tr(:,:,:,1,1), phi (spdy_geopotential_dev of t) (mx,nx,kx) complex, ps (mx,nx).
 * ONE inverse launch (the segmented inverse path: kx (vor, div) pairs through uvspec with kcos 2, and the 3 kx + 1 plain fields t,
 * q, phi, ps with kcos 1; physics.f90:94-104) into plan workspace, then the chain on those grids -- by default as one launch,
 * with "physics_fused" 0 as the five calls.  utend, vtend, ttend, qtend are the operands spdy_grid_tendencies_dev documents
 * (u_out[0:kx], v_out[0:kx], plain_out[kx:2kx], plain_out[2kx:3kx]), updated in place; bnd, albsfc, rad_state and out as for
 * spdy_column_physics_dev with nb = 1.  max_batch >= 3 kx + 1 (SPDY_ERR_ARG otherwise).  spdy_physics_workspace allocates the
 * workspace ((5 kx + 1) grids and one state's chain workspace of (3 kx + 12) grids) ahead of time, e.g. before a graph capture;
 * with it spdy_physics_dev allocates nothing and can be captured.                                                              */
int spdy_physics_workspace(spdy_plan *plan);
int spdy_physics_dev(spdy_plan *plan, int compute_sw, const double *vor, const double *div, const double *t, const double *q,
                     const double *phi, const double *ps, const spdy_sfc_boundary *bnd, const double *albsfc, double *rad_state,
                     double *utend, double *vtend, double *ttend, double *qtend, const spdy_column_physics_out *out);
/* the same for nmem members of an ensemble ("ensemble time step" above: layout, checks) */
int spdy_ens_physics_workspace(spdy_plan *plan, int nmem);
int spdy_ens_physics_dev(spdy_plan *plan, int nmem, int compute_sw, const double *vor, const double *div, const double *t,
                         const double *q, const double *phi, const double *ps, const spdy_sfc_boundary *bnd, const double *albsfc,
                         double *rad_state, double *utend, double *vtend, double *ttend, double *qtend,
                         const spdy_column_physics_out *out);

/* ---- SPPT: stochastically perturbed parametrisation tendencies (sppt.f90, physics.f90:85-88 and :207-222) -----------------------
 * The reference's model-error scheme: a random pattern, AR(1) in time per spectral coefficient, multiplies the physics' part of
 * each tendency.  A spdy_sppt is the pattern, device-resident and owned by the object:
 *   create    on a plan (max_batch >= kx on a device plan) for nsteps steps per day; mu: kx doubles on the host, the taper per
 *             level, top down (NULL = all ones, the reference's).  Host tables (spdy_sppt_table, like spdy_get_table; served by a
 *             host-only plan too; a buffer with cap below the table's length is SPDY_ERR_ARG): "phi" (1) = exp(-(24/nsteps)/6.0);
 *             "f0" (1) = sqrt(stddev**2 (1 - phi**2) / (2 sum_{n=1..trunc} (2n+1) exp(-0.5 (len_decorr/rearth)**2 n(n+1)))) with
 *             stddev = 0.33 (float32, widened) and len_decorr = 500000; "sigma" (mx,nx) = f0 exp(-0.25 len_decorr**2 el2) over the
 *             whole rectangle, sigma(1,1) = f0 (the reference perturbs the global mean too), the same on every level; "mu" (kx);
 *             "first" (1) = (1 - phi**2)**(-0.5).  Lifetime: the plan section's rule.
 *   advance   gen_sppt() without its return copy, three launches: (1) eta is drawn, or copied from d_eta ((mx,nx,kx) complex,
 *             device; NULL = draw), and each part clipped to +-10; the counter `draws` (64 bits, in the object's DEVICE memory) is
 *             read on the device: 0 gives spec = first * sigma * eta, otherwise spec = phi * spec + sigma * eta; (2) the plan's
 *             inverse transform of the kx fields, kcos 1 -- the reference never truncates sppt_spec and draws imaginary parts for
 *             m = 0, its spec_to_grid reads neither and neither does the plan's; (3) the clip to +-1 into "pattern", and
 *             draws += 1, with or without d_eta.  Nothing is allocated, so it can be captured: ONE captured advance serves the
 *             first step and every later one, and each replay draws new noise.
 *   reset     a new seed and draws = 0 (the next advance is a first one); stream-ordered, not callable during a capture.
 *   field     device pointers that never change: "eta", "spec" (mx,nx,kx) complex, "pattern" (ix,il,kx).
 *   draws     downloads the counter (synchronises the plan's stream).
 * The generator (csrc/spdy_sppt.hip) is Philox4x32-10 -- multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9,
 * 0xBB67AE85 -- with key (seed & 0xffffffff, seed >> 32) and counter (coefficient index in storage order, part, draws & 0xffffffff,
 * draws >> 32), part 0 for the real and 1 for the imaginary part.  Of the output words w0..w3
 *     r1 = (double((w0 >> 5) * 2**26 + (w1 >> 6)) + 1) * 2**-53   in (0, 1],
 *     r2 =  double((w2 >> 5) * 2**26 + (w3 >> 6))      * 2**-53   in [0, 1),
 * and the part is the reference's randn (sppt.f90:102-116) as written: u = sqrt(-2 log r1), v = (2.0f * 6.28318530718f) * r2 (the
 * float32 product 12.566370964050293: 4 pi, not 2 pi), u sin v.  A coefficient's noise depends on (seed, draws, index) only.
 *
 * The application: spdy_column_physics_sppt_dev / spdy_physics_sppt_dev are spdy_column_physics_dev / spdy_physics_dev followed
 * by physics.f90:212-221: per level k each of utend, vtend, ttend, qtend becomes
 *     (1 + pattern * mu(k)) * (tend - tend_dyn) + tend_dyn,        tend_dyn = the value at entry,
 * in this order, without contraction.  ut_pbl / vt_pbl are zero above level kx, so utend / vtend are left alone there (that
 * changes no bit but the sign of a -0.0, as for spdy_pbl_dev).  d_pattern: (ix,il,kx) per state, nb states, device, already
 * clipped; mu: kx doubles on the host (NULL = 1), read at call time like `out`.  spdy_physics_sppt_dev reads s's current pattern
 * and mu and does NOT advance s: a step calls spdy_sppt_advance_dev, then spdy_physics_sppt_dev (the reference advances once per
 * physics call, both start-up steps included).  "physics_fused" selects the form as for the calls without SPPT, and both forms
 * give the same bits: the five calls between a kernel that saves the dynamics tendencies and one that applies the factor (two
 * more launches), or the one-launch kernel's SPPT instantiation (no more launches: the thread keeps level kx of utend and vtend
 * in registers and passes ttend and qtend through the workspace).  Everything else -- `out`, the radiation state, the checks and
 * their order (d_pattern / s count as required pointers; s of another plan SPDY_ERR_ARG) -- is as without SPPT.  The _workspace
 * calls allocate what the calls without SPPT need and (2 kx + 2) grids per state for the dynamics tendencies (max_batch states /
 * one state) ahead of a capture.
 *
 * The ensemble form ("ensemble time step" above): a spdy_sppt made by spdy_ens_sppt_create holds nmem patterns, member-major in the
 * layout of every other ensemble array -- "eta" and "spec" (mx,nx,kx,nmem) complex, "pattern" (ix,il,kx,nmem), member e starting
 * e*kx fields in -- and one {draws, seed} pair per member in device memory; the tables are shared.  seeds: nmem values on the
 * host.  A device plan needs max_batch >= nmem*kx.  spdy_sppt_create, _reset and _draws are the one-member / member-0 case of
 * spdy_ens_sppt_create, _reset and _draws; spdy_sppt_members gives nmem (a host-only plan answers it too); _table, _field, _destroy
 * and spdy_sppt_advance_dev work on an object of any nmem, d_eta then being (mx,nx,kx,nmem).  The advance is the same three
 * launches whatever nmem is: the noise kernel takes the member from blockIdx.y, reads that member's counter and seed, and counts
 * the generator's coefficient index INSIDE the member (0 .. mx*nx*kx-1), so member e draws exactly what a one-member object with
 * seeds[e] draws; the first / AR(1) branch is each member's own, so one launch may take the first-draw branch for a member just
 * reset (spdy_ens_sppt_reset: that member only) and the AR(1) branch for the others; ONE inverse transform of nmem*kx fields; the
 * clip of all members, one thread per member counting that member's advance.  Members are fields of a batch: nothing one member
 * holds, non-finite values included, changes a bit of another member's eta, spec, pattern or counter.
 * spdy_ens_physics_sppt_dev is spdy_ens_physics_dev followed by physics.f90:212-221 per member with that member's pattern and the
 * shared mu: ONE inverse launch of time level 1 of all members, then the chain's SPPT form with nb = nmem, in both
 * "physics_fused" forms the same bits; it does not advance s.  Checks as spdy_ens_physics_dev with s a required pointer; then s of
 * another plan, then spdy_sppt_members(s) != nmem SPDY_ERR_ARG (spdy_physics_sppt_dev: an s of more than one member).
 * spdy_ens_physics_sppt_workspace(nmem) allocates what spdy_ens_physics_workspace does and (2 kx + 2) grids per member.  Checks
 * of the object calls: a NULL plan / object, nmem < 1, NULL seeds or result pointer, a member outside [0, nmem) SPDY_ERR_ARG; an
 * open capture (create, reset, draws) SPDY_ERR_STATE; a host-only plan SPDY_ERR_NO_DEVICE last.                                */
typedef struct spdy_sppt spdy_sppt;
int spdy_sppt_create(spdy_plan *plan, int nsteps, const double *mu, unsigned long long seed, spdy_sppt **s);
int spdy_ens_sppt_create(spdy_plan *plan, int nmem, int nsteps, const double *mu, const unsigned long long *seeds, spdy_sppt **s);
int spdy_sppt_members(const spdy_sppt *s);
int spdy_sppt_destroy(spdy_sppt *s);
int spdy_sppt_reset(spdy_sppt *s, unsigned long long seed);
int spdy_ens_sppt_reset(spdy_sppt *s, int member, unsigned long long seed);
int spdy_sppt_table(const spdy_sppt *s, const char *name, double *buf, int cap);
int spdy_sppt_field(spdy_sppt *s, const char *name, double **d_ptr);
int spdy_sppt_draws(spdy_sppt *s, long long *draws);
int spdy_ens_sppt_draws(spdy_sppt *s, int member, long long *draws);
int spdy_sppt_advance_dev(spdy_sppt *s, const double *d_eta);
int spdy_column_physics_sppt_workspace(spdy_plan *plan);
int spdy_column_physics_sppt_dev(spdy_plan *plan, int nb, const double *d_pattern, const double *mu, int compute_sw,
                                 const double *ug, const double *vg, const double *tg, const double *qg, const double *phig,
                                 const double *pslg, const spdy_sfc_boundary *bnd, const double *albsfc, double *rad_state,
                                 double *utend, double *vtend, double *ttend, double *qtend, const spdy_column_physics_out *out);
int spdy_physics_sppt_workspace(spdy_plan *plan);
int spdy_physics_sppt_dev(spdy_plan *plan, spdy_sppt *s, int compute_sw, const double *vor, const double *div, const double *t,
                          const double *q, const double *phi, const double *ps, const spdy_sfc_boundary *bnd, const double *albsfc,
                          double *rad_state, double *utend, double *vtend, double *ttend, double *qtend,
                          const spdy_column_physics_out *out);
int spdy_ens_physics_sppt_workspace(spdy_plan *plan, int nmem);
int spdy_ens_physics_sppt_dev(spdy_plan *plan, int nmem, spdy_sppt *s, int compute_sw, const double *vor, const double *div,
                              const double *t, const double *q, const double *phi, const double *ps, const spdy_sfc_boundary *bnd,
                              const double *albsfc, double *rad_state, double *utend, double *vtend, double *ttend, double *qtend,
                              const spdy_column_physics_out *out);

/* ---- surface models: the slab land, sea and ice models and the daily forcing (coupler.f90, land_model.f90, sea_model.f90,
 * forcing.f90) -------------------------------------------------------------------------------------------------------------
 * The reference's main loop (speedy.f90:27-54) calls set_forcing(1) on the first step of every day and couple_sea_land after
 * EVERY step; the next step's surface fluxes read what they leave.  A spdy_surface_model holds all of it in device memory, so a
 * run with physics exchanges nothing with the host between outputs:
 *   create    takes the fields as the reference holds them after land_model_init / sea_model_init (host arrays; reading files,
 *             fillsf, forchk and the soil-water formula stay with the caller): fmask, alb0 (ix,il); stl12, snowd12, soilw12,
 *             sst12, sice12 (ix,il,12); sstan3 (ix,il,3; may be NULL without SPDY_SURFACE_SST_ANOMALY).  It builds on the host
 *             and keeps in device memory fmask_l, fmask_s, rhcapl, cdland (land_model.f90:75-87, :159-180) and rhcaps, rhcapi,
 *             cdsea, cdice (sea_model.f90:137-150, :204-250) for the time step delt [s]; spdy_surface_model_table reads them
 *             like spdy_get_table.  flags: SPDY_SURFACE_LAND_COUPLING (land_coupling_flag), SPDY_SURFACE_ICE_COUPLING
 *             (ice_coupling_flag), SPDY_SURFACE_SST_ANOMALY (sst_anomaly_coupling_flag); the reference's defaults are all
 *             three (SPDY_SURFACE_DEFAULT).  On a host-only plan create builds the tables; every device call is then
 *             SPDY_ERR_NO_DEVICE.  Lifetime: the plan section's rule.
 *   set_date  imont1 (1 .. 12), tmonth and tyear as date.f90:147-151 makes them (float32 expressions, widened): the host
 *             computes the weights and months of forin5 / forint (interpolation.f90:16-69) and copies them to model memory on
 *             the plan's stream, then calls spdy_radiation_set_date(tyear).  Not callable during a capture; a captured call
 *             picks the new date up on its next replay.  spdy_surface_model_set_sst_anomaly replaces the window sstan3
 *             (obs_ssta's shift, sea_model.f90:366-384; the file read is the caller's), stream-ordered likewise.
 *   couple    the whole of couple_sea_land(day) as ONE launch, one thread per column: the three land and three sea
 *             interpolations, the adjustment over the freezing point (sea_model.f90:284-305), with day == 0 the initialisation
 *             of stl_lm, sst_om (= 0), tice_om, sice_om, otherwise run_land_model and run_sea_model, then stl_am, snowd_am,
 *             soilw_am, sst_am, sice_am, tice_am, sstan_am, ssti_om.  hfluxn (ix,il,2), shf, evap (ix,il,3), ssrd (ix,il) are the
 *             arrays spdy_physics_dev writes through `out` (sfc.hfluxn, sfc.shf, sfc.evap, rad.ssrd); NULL is allowed with
 *             day == 0 only.  No contraction, as in the column physics.  Capturable with day > 0 (day == 0, the initialisation,
 *             is SPDY_ERR_STATE inside a capture: it has to have run before forcing or couple(day > 0) are accepted).
 *   forcing   set_forcing(1) parts 2 and 4 (forcing.f90:55-62, :84-99): one column kernel makes snowc, alb_l, alb_s, albsfc and
 *             corh = refrh1*(qref - qsfc), then the plan's direct transform of that one field writes the caller's qcorh (mx,nx)
 *             (device).  Needs the orography (spdy_surface_set_orography).  Capturable.  tcorh does not depend on time and is
 *             the caller's.
 *   boundary  hands out the model's own arrays for spdy_physics_dev (bnd->fmask = fmask_l; sst_am, stl_am, soilw_am, snowc,
 *             alb_l, alb_s) and albsfc.  The pointers never change, so a captured step sees each update on its next replay.
 *   field     every prognostic and diagnostic field by the reference's name: stlcl_ob snowdcl_ob soilwcl_ob stl_lm stl_am
 *             snowd_am soilw_am sstcl_ob sicecl_ob ticecl_ob sstan_ob sst_om tice_om sice_om sst_am sstan_am sice_am tice_am
 *             ssti_om snowc alb_l alb_s albsfc corh, and the constants fmask_l fmask_s alb0 rhcapl cdland rhcaps rhcapi cdsea
 *             cdice (device pointers to (ix,il) doubles; writable, e.g. for a restart).
 * Order of calls of one step: on the first step of a day forcing; the step {spdy_physics_dev ... dynamics}; the
 * host's newdate, and set_date when the day changed (and set_sst_anomaly where obs_ssta would run); couple(day).
 * Checks: a NULL required pointer SPDY_ERR_ARG; a host-only plan SPDY_ERR_NO_DEVICE; couple or forcing before set_date, and
 * forcing or couple(day > 0) before couple(0), SPDY_ERR_STATE.
 * nmem members (spdy_ens_surface_model_create; spdy_surface_model_create is that call with nmem = 1; nmem < 1 SPDY_ERR_ARG): the
 * same object type.  Held once: what no kernel writes -- fmask_s, alb0, rhcapl, cdland, rhcaps, rhcapi, cdsea, cdice, the five
 * 12-month fields, sstan3 and the date, which set_date, set_sst_anomaly and table serve unchanged: the date and the anomaly window
 * are the ensemble's.  Held per member, (ix,il,nmem) each (member e of a field is ix*il doubles after member e - 1): every field
 * couple or forcing writes, stlcl_ob .. corh in field's list, and fmask_l, replicated, since the physics takes every boundary field
 * per state.  So boundary hands out (ix,il,nmem) arrays, the shape spdy_ens_physics_dev takes, and corh of all members is one stack
 * of nmem grids.  couple takes hfluxn (ix,il,2,nmem), shf, evap (ix,il,3,nmem), ssrd (ix,il,nmem) -- what spdy_ens_physics_dev writes
 * through `out` -- and is ONE launch with the member in blockIdx.y; forcing is one such launch and ONE spdy_grid_to_spec_dev of nmem
 * fields into the caller's qcorh (mx,nx,nmem) (nmem > max_batch: SPDY_ERR_ARG).  The member enters as uniform base offsets only: a
 * member's fields are bit for bit those of a single model given the same inputs.  field returns the base of the (ix,il,nmem) stack
 * of a per-member field; spdy_surface_model_members(m, name) is nmem for such a field, 1 for a field held once, SPDY_ERR_ARG for an
 * unknown name, and with name NULL the object's nmem.
 * Not built: sea_coupling_flag > 0 (the reference stops for it, sea_model.f90:188-198: no ocean-model climatology, hfseacl = 0,
 * beta = 1) and the ablco2 trend (increase_co2 is a .false. parameter, shortwave_radiation.f90).                                */
typedef struct spdy_surface_model spdy_surface_model;
typedef struct {                      /* host arrays, j = 0 southernmost                                                      */
    const double *fmask, *alb0;       /* (ix,il)                                                                              */
    const double *stl12, *snowd12, *soilw12, *sst12, *sice12;   /* (ix,il,12)                                                  */
    const double *sstan3;             /* (ix,il,3)                                                                            */
} spdy_surface_clim;
enum { SPDY_SURFACE_LAND_COUPLING = 1, SPDY_SURFACE_ICE_COUPLING = 2, SPDY_SURFACE_SST_ANOMALY = 4, SPDY_SURFACE_DEFAULT = 7 };
int spdy_surface_model_create(spdy_plan *plan, const spdy_surface_clim *host, double delt, int flags, spdy_surface_model **m);
int spdy_ens_surface_model_create(spdy_plan *plan, int nmem, const spdy_surface_clim *host, double delt, int flags, spdy_surface_model **m);
int spdy_surface_model_destroy(spdy_surface_model *m);
int spdy_surface_model_table(const spdy_surface_model *m, const char *name, double *buf, int cap);
int spdy_surface_model_set_date(spdy_surface_model *m, int imont1, double tmonth, double tyear);
int spdy_surface_model_set_sst_anomaly(spdy_surface_model *m, const double *sstan3);
int spdy_surface_model_couple_dev(spdy_surface_model *m, int day, const double *hfluxn, const double *shf, const double *evap,
                                  const double *ssrd);
int spdy_surface_model_forcing_dev(spdy_surface_model *m, double *qcorh);
int spdy_surface_model_boundary(spdy_surface_model *m, spdy_sfc_boundary *bnd, const double **albsfc);
int spdy_surface_model_field(spdy_surface_model *m, const char *name, double **d_ptr);
int spdy_surface_model_members(const spdy_surface_model *m, const char *name);

/* ---- diagnostics: the run's guard (check_diagnostics, diagnostics.f90:16-75) ------------------------------------------------------
 * The one call of the reference's main loop (speedy.f90:27-54) that looks at the state after every step: per level k, from the
 * spectra of time level 2,
 *     reke(k) = sum_{m=2..mx} sum_{n=1..nx} elm2(m,n) |vor(m,n,k)|**2      (the reference's -Re(inverse_laplacian(vor) conjg(vor)):
 *     deke(k) = the same over div                                           the zonal column m = 1 left out, the whole rectangle)
 *     temp(k) = sqrt(0.5) * Re t(1,1,k)                                     (sqrt(0.5) in float32, widened: 0.707106769084930...)
 * and the run stops when for any level reke > 500, deke > 500, temp < 180 or temp > 320.  A spdy_diagnostics keeps all of it in
 * device memory, so the guard runs inside a captured, replayed step and nothing is downloaded for it:
 *   create    on a plan; owns history -- capacity rows of (3,kx) doubles reke | deke | temp, the memory order of the reference's
 *             diag(kx,3); step s goes to row s mod capacity --, the four limits, and per level a state: the number of the next
 *             step (64 bits; first_step >= 0 at first), the level's first offending step with the mask of what tripped there, and
 *             the level's three numbers of the run's first offending step, outside the ring so that no wrap overwrites them.  On a
 *             host-only plan create succeeds and every device call is SPDY_ERR_NO_DEVICE.  Lifetime: the plan section's rule.
 *   check_dev ONE launch on three device arrays of (mx,nx,kx) complex spectra and the plan's elm2; one workgroup per level.  It
 *             allocates nothing and takes no host value that changes from step to step: a captured call records step s, s + 1, ...
 *             on successive replays, with the pointers it was captured with.  temp is one load and one multiply, bit for bit the
 *             reference's; the sums have a fixed thread-to-coefficient map and a fixed reduction tree and no atomics, so they are
 *             the same bits on every run and within 2 (mx nx - 1) 2**-53 of the reference's sequential sums (every term is >= 0).
 *             Mask bits: SPDY_DIAG_REKE, _DEKE, _TEMP_LOW, _TEMP_HIGH are the reference's four comparisons, strict, as written (a
 *             NaN satisfies none: the reference would run on); SPDY_DIAG_NONFINITE is set when any of the level's three numbers
 *             is not finite.  A level's first nonzero mask is sticky: later in-range steps do not clear it, later offences do
 *             not replace it.
 *   set_limits reke, deke, temp low, temp high (host; NULL = 500, 500, 180, 320); reset: a new next step, no offence, an empty
 *             history.  Both stream-ordered, not callable during a capture; a captured check_dev uses them on its next replay.
 *   status    synchronises the plan's stream and downloads the state: next_step; bad_step = -1 when nothing has tripped,
 *             otherwise the earliest offending step over all levels, bad_level the lowest level index (0-based) that tripped at
 *             that step, bad_mask the OR of the masks of all levels that tripped at it, bad_row the (3,kx) row of that step (left
 *             alone when nothing tripped).  Any of the five result pointers may be NULL.  SPDY_ERR_STATE inside a capture, or if
 *             the levels' step counters disagree (a check_dev still in flight on another stream).
 *   read      synchronises and downloads count rows starting at step into rows (count,3,kx); SPDY_ERR_ARG for steps not yet
 *             written (or from before the last reset) or already overwritten; SPDY_ERR_STATE inside a capture.
 *   field     device pointers that never change: "history", "state", "limits".
 *   format    host only, no object needed: the reference's three lines (diagnostics.f90:72-74) for one (3,kx) row -- ' step =',
 *             i6, ' reke =', then f8.2 fields; the deke and temp lines with 13x; for kx > 10 Fortran's format reversion: each
 *             further record holds up to ten f8.2 fields and nothing else.  Every record ends with a newline.  Returns the
 *             number of characters without the terminator (buf NULL: the size query); cap below that + 1 is SPDY_ERR_ARG.
 * A device-resident main loop: forcing, step, check_dev on time level 2, couple; status once per output interval.
 * nmem members (spdy_ens_diagnostics_create; spdy_diagnostics_create is that call with nmem = 1; nmem < 1 SPDY_ERR_ARG): the same
 * object type.  check_dev takes one time level of the ensemble, (mx,nx,kx,nmem) complex, and is ONE launch on a (kx, nmem) grid
 * with the same thread-to-coefficient map and reduction tree: member e's numbers are bit for bit a single object's on its slice.
 * History row s holds (3,kx,nmem): member e's (3,kx) block starts at ((s mod capacity)*nmem + e)*3*kx doubles.  The state is
 * [nmem][kx] records, and the sticky first offence is per member: the scan for an earlier offence reads the member's own levels
 * only, so a member that leaves the range freezes its own saved row while every other member's row and ring go on following the
 * step.  The limits are shared.  Host calls by member, not callable inside a capture:
 *   spdy_ens_diagnostics_status(d, member, ...) and spdy_ens_diagnostics_read(d, member, step, count, rows) are status and read for
 *             one member (rows (count,3,kx)); a member outside [0, nmem) is SPDY_ERR_ARG.  The unsuffixed status and read on an
 *             object with nmem > 1 are SPDY_ERR_ARG.
 *   spdy_ens_diagnostics_stopped(d, bad_step)  one synchronisation and one download: bad_step[e] (nmem values) = -1 or member e's
 *             first offending step; returns the number of members that tripped.
 * Checks: a NULL object, NULL spectra, rows or name, capacity < 1, a negative step: SPDY_ERR_ARG.                               */
enum { SPDY_DIAG_REKE = 1, SPDY_DIAG_DEKE = 2, SPDY_DIAG_TEMP_LOW = 4, SPDY_DIAG_TEMP_HIGH = 8, SPDY_DIAG_NONFINITE = 16 };
typedef struct spdy_diagnostics spdy_diagnostics;
int spdy_diagnostics_create(spdy_plan *plan, int capacity, long long first_step, spdy_diagnostics **d);
int spdy_ens_diagnostics_create(spdy_plan *plan, int nmem, int capacity, long long first_step, spdy_diagnostics **d);
int spdy_diagnostics_destroy(spdy_diagnostics *d);
int spdy_diagnostics_set_limits(spdy_diagnostics *d, const double *limits);
int spdy_diagnostics_reset(spdy_diagnostics *d, long long next_step);
int spdy_diagnostics_check_dev(spdy_diagnostics *d, const double *vor, const double *div, const double *t);
int spdy_diagnostics_status(spdy_diagnostics *d, long long *next_step, long long *bad_step, int *bad_level, int *bad_mask,
                            double *bad_row);
int spdy_diagnostics_read(spdy_diagnostics *d, long long step, int count, double *rows);
int spdy_ens_diagnostics_status(spdy_diagnostics *d, int member, long long *next_step, long long *bad_step, int *bad_level, int *bad_mask,
                                double *bad_row);
int spdy_ens_diagnostics_read(spdy_diagnostics *d, int member, long long step, int count, double *rows);
int spdy_ens_diagnostics_stopped(spdy_diagnostics *d, long long *bad_step);
int spdy_diagnostics_field(spdy_diagnostics *d, const char *name, void **d_ptr);
int spdy_diagnostics_format(int kx, long long step, const double *row, char *buf, int cap);

/* ---- ensemble analysis: the LETKF update of all members on the device -----------------------------------------
 * The reference has no analysis; this section defines one, and tests/letkf.py restates it in NumPy.  A forecast-analysis cycle
 * then stays in device memory: Ensemble steps, spdy_ens_letkf_dev, first_step again.
 * State analysed, per member: the gridded true wind u, v, t, q (the model's g/kg), each with kx levels, and ps = log(p/p0).  An
 * observation {var: SPDY_OBS_*; lev 0..kx-1 (ignored for PS); lon, lat in degrees; value; error > 0} is in those units.
 *   operator      H is bilinear in longitude and latitude at model level lev.  Column i is at i*360/ix, periodic; row j at
 *                 -/+ asin(sia_half), south first (geometry.f90:70-75); poleward of the outermost row that row has weight 1.  The
 *                 four points are (j0,i0) (j0,i1) (j1,i0) (j1,i1) with weights (1-a)(1-b), a(1-b), (1-a)b, ab, and
 *                 hx_e = ((w0 x0 + w1 x1) + w2 x2) + w3 x3; hxmean = (sum of hx_e, e ascending) / E; Y_e = hx_e - hxmean;
 *                 d = value - hxmean.
 *   localisation  w = GC(dist/c_h) GC(|ln fsg[k] - ln sigma_o|/c_v) for column c, level k and observation o: GC the fifth-order
 *                 function of Gaspari and Cohn (support r < 2), c_h = sigma_h sqrt(10/3), c_v = sigma_v sqrt(10/3), sigma_o =
 *                 fsg[lev] (1 for PS), dist = 2 rearth asin(min(1, |p_c - p_o|/2)) on unit vectors, rearth = 6.371e6 m.
 *                 sigma_v <= 0: no vertical factor.  An observation with w == 0 takes no part in any operation.
 *   local problem r_o = w_o / error_o^2; C = sum_o r_o Y_o Y_o^T, b = sum_o r_o Y_o d_o, each element summed over o ascending;
 *                 A = (E-1)/rho I + C = V Lambda V^T; wbar = V Lambda^-1 V^T b; W = V diag(sqrt((E-1)/lambda_i)) V^T;
 *                 T = W + wbar 1^T - I.
 *   increments    dx_e = sum_f (x_f - xmean) T[f][e] for every analysed variable at (c, k); ps uses T of level kx-1.  With no
 *                 observation in range and rho = 1, T and the increments are exactly zero; with rho != 1 they are pure inflation.
 * spdy_letkf_create allocates everything the calls below use (observation tables for max_obs observations, (4 kx + 1) nmem grids
 * and as many spectra) and runs one inverse and one direct batch of the analysis' shape, so nothing is allocated afterwards and
 * both *_dev calls can be captured.  2 <= nmem <= 32 and the local problems of kx levels must fit a compute unit's LDS (kx = 16 at
 * nmem = 32 does); max_batch >= nmem (2 kx + 1); the plan needs sigma levels (their ln fsg is read here, once).
 * spdy_letkf_set_localization: sigma_h in metres (> 0), sigma_v in ln sigma, rho > 0; read when an analysis call is enqueued, so a
 * captured graph keeps the values of its capture.  spdy_letkf_set_obs validates every field of every observation before it
 * changes anything, builds the stencils, unit vectors, ln sigma_o and 1/error^2 on the host and uploads them (stream-ordered,
 * synchronising; not inside a capture; should a copy fail, SPDY_ERR_HIP, the object is left with no observations, not with a
 * mixture; the errors themselves are kept on the device too, for spdy_nature_observe_dev, which may write the values in
 * set_obs' place: "nature run" below); the device arrays do not move, so a captured analysis replays with the observations of
 * the latest set_obs as long as their number is that of the capture.  spdy_letkf_table (the host side; returns the count; buf NULL
 * = count only): "stencil_index" (4 per observation, j*ix+i as doubles), "stencil_weight" (4), "unit" (3), "lnsigma", "rinv".
 * spdy_letkf_field (device, valid after an analysis call): "hx" (nmem per observation), "hxmean", "y" (nmem), "departure"; and
 * "value", the observation values the next analysis reads (valid after set_obs or spdy_nature_observe_dev); "grid", the grid
 * workspace of (4 kx + 1) nmem grids (the gridded ensemble after spdy_nature_verify_dev, the increments after spdy_ens_letkf_dev).
 * spdy_letkf_analyse_grid_dev: the ensemble on the grid, member-major, u .. q (ix,il,kx,nmem), ps (ix,il,nmem); the increments in
 * the same shapes; an output may be its input.  Two launches: the observation kernel, then one workgroup per grid column that
 * scans the observations in chunks, keeps those in range in ascending order (ballot and prefix counts, no atomics), forms C and b
 * of every level in LDS, solves each level by a parallel cyclic Jacobi (round-robin pairs; an odd E is padded by a decoupled
 * row; sweeps end at convergence or after a fixed count) and writes the increments.  Any number of observations may be in range
 * of a column.  Results are bit-reproducible, and a column's result depends on no observation out of its range.
 * spdy_ens_letkf_dev: the analysis of time level 1 of an ensemble ("ensemble time step" above: layout), in place -- ONE
 * spdy_inverse_batch_segs_dev (nmem*kx pairs, the segments t | q of nmem*kx fields and ps of nmem, read in place), the two
 * kernels, ONE spdy_direct_batch_dev (nmem*kx pairs with kcos = 2, 2 nmem kx + nmem plain fields), and a kernel that adds
 * vdspec(du, dv) to vor and div and grid_to_spec(dt | dq | dps) to t, q and ps; a spectral increment equal to zero leaves the
 * coefficient's bits, so with no observations and rho = 1 the state is unchanged.  Five launches whatever nmem is -- six where the
 * direct batch streams (16 MB of grids or more: spdy_direct_batch_dev then goes out as its two launches).  Time level 2
 * is not touched and phi is stale afterwards: the run continues with first_step, as a model started from an analysis does.
 * Members are coupled by construction: a non-finite member makes every column it touches non-finite (as NaN, after the full
 * count of sweeps); spdy_mask_ens_letkf_dev ("member mask" below) analyses the members a device mask names and leaves the others alone.
 * Weight interpolation (Yang, Kalnay, Hunt and Bowler 2009): T varies slowly in space, because the localisation function is smooth
 * over several grid spacings, so the local problems may be solved on a coarse subset of the columns only, and every other column
 * gets T by bilinear interpolation from the four coarse columns around it.
 *   stride        (si, sj): si divides ix, 1 <= si <= ix/2, 1 <= sj <= il-1.  Coarse longitudes i = 0, si, 2 si, ..., periodic;
 *                 coarse rows j = 0, sj, 2 sj, ... together with il-1, so the last latitude interval may be shorter than sj.  A
 *                 coarse column is a grid column j*ix+i with i and j both coarse; the coarse list has them in ascending order.
 *   stencil       of grid column (i, j): i0 = (i/si) si, i1 = (i0 + si) mod ix, a = (i - i0)/si; j0 the largest coarse row <= j, j1
 *                 the next coarse row, or j0 itself when j == il-1; b = (j - j0)/(j1 - j0), 0 when j1 == j0.  The points (j0,i0)
 *                 (j0,i1) (j1,i0) (j1,i1) with weights (1-a)(1-b), a(1-b), (1-a)b, ab: the operator's order and form.  The
 *                 interpolation is in index space: longitude is uniform and the Gaussian rows are uniform to within a fraction
 *                 of a percent, so no latitude enters.
 *   transform     for level k, T[f][e] = ((w0 T0[f][e] + w1 T1[f][e]) + w2 T2[f][e]) + w3 T3[f][e]; a term whose weight is exactly
 *                 zero is neither read nor added, and the first term present starts the sum.  So at a coarse column T is 1.0 * T0,
 *                 bit for bit the solved T; on a coarse row or a coarse longitude only two terms exist; and a column depends on no
 *                 coarse column outside its stencil.
 *   increments    exactly those above on the interpolated T: the mean over the members ascending, dx_e = sum_f (x_f - xmean)
 *                 T[f][e] with f ascending, ps with T of level kx-1.  The local problem at a coarse column is the one above,
 *                 unchanged: the observations in range of that column, the same ascending sums, the same Jacobi.
 * Consequences: with no observation and rho = 1 every T is exactly zero and so is every increment; a fine column's result depends
 * only on the observations in range of its stencil's coarse columns, not on those in its own range; pure inflation by rho != 1 is
 * exact at coarse columns and holds to a few ulps elsewhere, because the weights do not sum to 1 exactly.
 * spdy_letkf_set_weight_stride: (1, 1), the default after create, is the path above exactly -- the same kernels, the same launch
 * count, no weight buffer.  Any other stride builds the coarse list and every column's stencil (indices into the coarse list) on
 * the host, uploads them and allocates the weight buffer, ncoarse kx nmem nmem doubles laid out [coarse][k][f][e]; stream-ordered
 * and synchronising like set_obs.  It works on a host-only plan, where it builds the tables only.  A graph captured before a
 * change of stride has to be captured again.  spdy_letkf_table then also gives "coarse_columns" (the grid indices, as doubles),
 * "interp_index" (4 per grid column; an entry of weight zero repeats the first index) and "interp_weight" (4 per grid column);
 * at stride (1, 1) all three have count 0.  spdy_letkf_field gives "weights", the device weight buffer, valid after an analysis
 * call at a stride other than (1, 1); SPDY_ERR_STATE at stride (1, 1).  At such a stride spdy_letkf_analyse_grid_dev is three
 * launches -- the observation kernel, the transform kernel on the coarse columns only, which writes T of every level into the
 * weight buffer instead of increments, and a kernel over all grid columns that interpolates T and forms the increments -- and
 * spdy_ens_letkf_dev six (seven where the direct batch streams); both remain capturable, nothing is allocated in the call.
 * Checks, in this order -- create: a NULL plan, nmem outside [2, 32], max_obs < 0, a NULL result pointer, max_batch, the LDS
 * size SPDY_ERR_ARG; no sigma levels, an open capture SPDY_ERR_STATE.  set_obs: a NULL object, nobs outside [0, max_obs], NULL
 * observations, the first invalid field of the first invalid observation (var, lev, lon, lat, value, error) SPDY_ERR_ARG; an open
 * capture SPDY_ERR_STATE.  The *_dev calls: a NULL object SPDY_ERR_ARG; no localisation set SPDY_ERR_STATE; a NULL pointer
 * SPDY_ERR_ARG; a host-only plan SPDY_ERR_NO_DEVICE last (spdy_letkf_field: after its name check, and after SPDY_ERR_STATE for "weights" at stride (1, 1)).
 * set_weight_stride: a NULL object, an invalid stride SPDY_ERR_ARG (nothing changes); an open capture SPDY_ERR_STATE; a failed
 * allocation or copy SPDY_ERR_HIP, and the object is left at stride (1, 1).  create, set_localization, set_obs, set_weight_stride
 * and table work on a host-only plan.  A failing call enqueues nothing.                                                         */
typedef struct spdy_letkf spdy_letkf;
enum { SPDY_OBS_U, SPDY_OBS_V, SPDY_OBS_T, SPDY_OBS_Q, SPDY_OBS_PS };
typedef struct {
    int var, lev;
    double lon, lat, value, error;
} spdy_obs;
int spdy_letkf_create(spdy_plan *plan, int nmem, int max_obs, spdy_letkf **l);
int spdy_letkf_destroy(spdy_letkf *l);
int spdy_letkf_set_localization(spdy_letkf *l, double sigma_h_m, double sigma_v_lnsigma, double rho);
int spdy_letkf_set_obs(spdy_letkf *l, int nobs, const spdy_obs *host);
int spdy_letkf_set_weight_stride(spdy_letkf *l, int si, int sj);
int spdy_letkf_table(const spdy_letkf *l, const char *name, double *buf, int cap);
int spdy_letkf_field(spdy_letkf *l, const char *name, double **d_ptr);
int spdy_letkf_analyse_grid_dev(spdy_letkf *l, const double *ug, const double *vg, const double *tg, const double *qg,
                                const double *psg, double *du, double *dv, double *dt, double *dq, double *dps);
int spdy_ens_letkf_dev(spdy_letkf *l, double *vor, double *div, double *t, double *q, double *ps);

/* ---- ensemble analysis, observations at a pressure --------------------------------------------------------------
 * Radiosondes, aircraft and satellite winds report at a pressure.  In a sigma model the level that brackets a pressure differs from
 * member to member and from column to column, because every member has its own surface pressure; so the operator interpolates in
 * the vertical per member.  tests/letkfpressure.py restates this subsection in NumPy.
 * spdy_pobs_set is spdy_letkf_set_obs for a network in which any observation of u, v, t or q may be given at a pressure: with
 * lev == SPDY_OBS_AT_P the observation sits at p, in Pa, finite and > 0; with lev in 0..kx-1 it is the model-level observation
 * above and p is ignored; for SPDY_OBS_PS lev and p are both ignored.  Checks, in this order: a NULL object SPDY_ERR_ARG ("null
 * analysis object"), a destroyed plan SPDY_ERR_STATE, nobs outside [0, max_obs], NULL observations, the first invalid field of the
 * first invalid observation -- var, lev (an at-pressure observation on a plan with kx < 2 fails here), p, lon, lat, value, error --
 * SPDY_ERR_ARG; an open capture SPDY_ERR_STATE.  A rejected call changes nothing.  Stream-ordered and synchronising like set_obs;
 * works on a host-only plan.  A set without any at-pressure observation leaves the object exactly as spdy_letkf_set_obs would: the
 * same kernels, the same launch count, the same bits.  A later spdy_letkf_set_obs returns it to a pure model-level network.  The
 * arrays this needs come with spdy_letkf_create: nothing is allocated here or in an analysis call.  A graph captured with a network
 * of one kind has to be captured again after a set of the other kind; between networks of one kind it replays as before.  (A
 * stale graph computes something else, it does not leave its arrays: on the device an at-pressure observation has level 0 and a
 * flag of its own, so the plain observation kernel reads it as an observation on level 0.)
 *   operator      linear in ln p only.  x_o = ln(p_o / p0), p0 = 1e5 Pa, formed on the host by the C library's log at
 *                 spdy_pobs_set, so the device needs no transcendental.  For member e and stencil point s (the four points and
 *                 weights of the operator above, all four evaluated whatever their weight) the column's coordinate is X_k =
 *                 ps_e[s] + ln fsg[k], and z_{e,s} is the value at x_o by np.interp's rule ("pressure-level output" above, linear
 *                 in ln p): with kb the number of k in 1..kx-2 with X_k <= x_o, level 0's bits where x_o <= X_0, level kx-1's
 *                 bits where x_o >= X_{kx-1}, else f[kb] + w (f[kb+1] - f[kb]) with w = (x_o - X_kb) / (X_{kb+1} - X_kb), every
 *                 operation rounded once.  hx_e = ((w0 z0 + w1 z1) + w2 z2) + w3 z3; hxmean, Y and d as above, e ascending.
 *   localisation  the observation's vertical position is that of its pressure under the ensemble-mean surface pressure at its
 *                 place: pb_e = ((w0 ps_e[i0] + w1 ps_e[i1]) + w2 ps_e[i2]) + w3 ps_e[i3], psbar = (sum of pb_e, e ascending) / E,
 *                 ln sigma_o = x_o - psbar.  It is written, on every analysis call, to the device array the local analyses read:
 *                 a captured analysis localises with the ensemble of the replay.  Model-level and PS observations keep theirs.
 *   use           an at-pressure observation is out of column in a call if for some member and some of its four points x_o < X_0
 *                 or x_o > X_{kx-1}; a target exactly on an end level is in the column; a non-finite ps makes neither comparison
 *                 true, rejects nothing and propagates as NaN.  The values of an out-of-column observation would be an end
 *                 level's, an extrapolation: its r is exactly 0 in this call -- it enters no sum, by "an observation with w == 0
 *                 takes no part" -- while its hx, hxmean, Y and d are still written, for diagnostics.  The local analyses read a
 *                 per-call copy of 1/error^2 for this; the host table "rinv" stays 1/error^2.
 * spdy_letkf_table: "lnp", ln(p/p0) of the at-pressure observations and 0 for the others, one per observation after spdy_pobs_set,
 * count 0 after spdy_letkf_set_obs; "lnsigma" gives ln(p/p0) for an at-pressure observation, its ln sigma_o at ps = 0.
 * spdy_letkf_field: "obs_lnsigma", ln sigma_o of every observation as the latest analysis call localised with it (for a
 * model-level network the uploaded table); "obs_used", 1.0 or 0.0 per observation (all 1.0 after a set and for a model-level
 * network).  The kernel, in the observation kernel's place only when the current network holds an at-pressure observation: a
 * workgroup owns whole observations, one thread per (observation, member) finds the four brackets from the four ps and loads the
 * levels they name by address, one thread per observation sums over the members; no atomics.  The launch counts above hold.
 * spdy_nature_observe_dev on such a network writes value_o = h_o + (noise * error_o) * z_o with h_o the same operator on the truth
 * and its ps, clamped to the end level where the truth is out of column; noise, counter and launch count as in "nature run".    */
enum { SPDY_OBS_AT_P = -1 };
typedef struct {
    int var, lev;
    double p, lon, lat, value, error;
} spdy_pobs;
int spdy_pobs_set(spdy_letkf *l, int nobs, const spdy_pobs *host);

/* ---- ensemble analysis and scores, member mask --------------------------------------------------------------------
 * The guard stops a member that leaves the range, and the output takes a mask ("ensemble output"); with these calls the analysis and
 * the scores do too, so a captured cycle keeps running when a member is lost.  d_use is nmem ints in device memory, non-zero = the
 * member is in use; it is read by the kernels when they run, not when the call is enqueued; NULL = all members, and the call is then
 * the unsuffixed one exactly: spdy_letkf_analyse_grid_dev, spdy_ens_letkf_dev, spdy_nature_verify_dev and
 * spdy_nature_verify_grid_dev are these calls with d_use = NULL, and launch the kernels they always launched, in the same number,
 * with the same bits.  Let U = (u_0 < u_1 < ... < u_{n-1}) be the members in use.
 *   n >= 2        the call is "ensemble analysis" (and "observations at a pressure") applied to the n-member ensemble (x_{u_0}, ...,
 *                 x_{u_{n-1}}), with every E of those definitions replaced by n: hxmean and Y over U ascending; A = (n-1)/rho I + C
 *                 with (n-1)/rho one IEEE division; W with sqrt((n-1)/lambda); the padded size n rounded up to even and the
 *                 round-robin order of that size; the means of the increment step over U; for an at-pressure network the
 *                 out-of-column test and the mean ps of ln sigma_o over U only.  So the results for the members in use are bit
 *                 for bit those of the unmasked call of an n-member object on the compacted members.
 *   not in use    such a member enters no operation whose result reaches another member or any shared quantity: it is skipped by
 *                 a select, never by a multiplication with zero, so it may hold NaN or anything else.  Its increments are written
 *                 as exactly 0.0 over its grids (spdy_mask_ens_letkf_dev: in the workspace, so the kernel that adds the spectral
 *                 increments leaves every bit of its spectra, NaN payloads included).  Its y is 0.0, its hx its own H x_e.
 *   n < 2         zero increments for every member, the state keeps its bits; hxmean and departure are the sums the rule gives
 *                 (n = 1: the member's own hx; n = 0: NaN, as the output's mean).
 *   weights       at a weight stride the buffer keeps its shape [ncoarse][kx][nmem][nmem]; the leading n x n block of each matrix,
 *                 in compact indices (f, e < n stand for u_f, u_e), is T, the rest is neither written nor read.
 *   scores        mbar = (sum over U ascending) / n, s2 = sum / (n - 1); n = 1 gives spread +0, n = 0 NaN in all three.  A member
 *                 not in use is never read into a score.
 * spdy_letkf_field "members_used": one double, nmem after an unmasked analysis call and n after a masked one -- two words of the
 * object's memory, the pointer is that of the kind of call enqueued (or captured) last, so ask after the call.
 * spdy_mask_from_diagnostics_dev(d, d_use): d_use[e] = 1 if member e of the guard has no sticky first offence at any level, else 0
 * (what spdy_ens_diagnostics_stopped reports as -1).  ONE launch, capturable, nothing allocated: {check_dev, this, masked verify,
 * masked analysis} needs no host.
 * Launches: a masked analysis call is its unmasked form with ONE small launch in front, which turns d_use into a table in the
 * object's memory (n, U and every member's compact index) that the masked forms of the kernels read: three launches for
 * spdy_mask_letkf_analyse_grid_dev (four at a weight stride), SIX for spdy_mask_ens_letkf_dev (seven at a weight stride; one more
 * each where the direct batch streams).  The launch shapes, the levels in flight and the LDS request stay those of nmem; the LDS
 * layout inside is that of n.  The masked verify calls read d_use as it is: three launches and two, as unmasked.  Nothing is
 * allocated; a captured graph holds the pointer d_use, not its contents: writing new contents and replaying is the supported way
 * to drop a member.  The calls carry a prefix of their own, spdy_mask_, not their objects' (DESIGN.md s23 says why).
 * Checks: those of the unsuffixed call in its order (d_use cannot be checked on the host); spdy_mask_from_diagnostics_dev: a NULL
 * object SPDY_ERR_ARG, a destroyed plan SPDY_ERR_STATE, a NULL d_use SPDY_ERR_ARG; a host-only plan SPDY_ERR_NO_DEVICE last.        */
int spdy_mask_letkf_analyse_grid_dev(spdy_letkf *l, const double *ug, const double *vg, const double *tg, const double *qg,
                                     const double *psg, double *du, double *dv, double *dt, double *dq, double *dps, const int *d_use);
int spdy_mask_ens_letkf_dev(spdy_letkf *l, double *vor, double *div, double *t, double *q, double *ps, const int *d_use);
int spdy_mask_from_diagnostics_dev(spdy_diagnostics *d, int *d_use);

/* ---- ensemble analysis, relaxation to the prior perturbations and spread ----------------------------------------
 * rho of spdy_letkf_set_localization inflates every column, observed or not.  Relaxation (RTPP: Zhang et al. 2004; RTPS: Whitaker
 * and Hamill 2012) acts where the analysis acted and is exactly 1 elsewhere.  tests/letkfrelax.py restates this section in NumPy.
 * It acts on the raw increments dx an analysis call forms, grid item by grid item; an item is one variable, one level and one
 * column, (4 kx + 1) per column in the order u | v | t | q | ps.  U: the members in use, all nmem without a mask, otherwise the
 * mask's ("member mask" above); n = |U|; every sum runs over U in ascending member order, every operation is one IEEE operation,
 * nothing is contracted:
 *     xm  = (sum x_e) / n            b_e = x_e - xm
 *     dm  = (sum dx_e) / n           a_e = b_e + (1 - rtpp) (dx_e - dm)          1 - rtpp is formed once, on the host
 *     sb  = sqrt((sum b_e^2) / (n - 1))
 *     sa  = sqrt((sum a_e^2) / (n - 1))
 *     f   = sa > 0 ? 1 + (rtps (sb - sa)) / sa : 1
 *     dx'_e = dm + (f a_e - b_e)
 * rtpp is applied first, rtps acts on the perturbations rtpp has relaxed; rtps = 0 gives f = 1.  A NaN propagates, as in the
 * analysis (sa = NaN gives f = 1 and NaN increments).  A member not in use keeps the exact 0.0 the analysis writes for it and is
 * not read; n < 2: zero increments for every member, as the masked analysis leaves them, and f = 1.  Three statements hold exactly:
 *   untouched     an item whose raw increments are all +0.0 (a column out of every observation's range with rho = 1) has a_e = b_e
 *                 up to the sign of a zero, so sa == sb, f == 1.0 and dx'_e == 0.0: the state keeps its bits there.
 *   rtpp = 1      a_e = b_e, so f == 1.0 and every member in use gets the same bits, dm: only the mean moves.
 *   both 0        the relaxation launch is not enqueued: the call has the launches, the graph nodes and the bits it always had.
 * spdy_relax_set(l, rtpp, rtps): both finite and in [0, 1], otherwise SPDY_ERR_ARG and nothing changes.  (0, 0) is the
 * state after create.  The values are read when an analysis call is enqueued, so a captured analysis keeps the values of its
 * capture.  The first setting that is not (0, 0) allocates a workspace of (4 kx + 1) nmem grids for the raw increments (307 MB
 * at T63 L16 with nmem = 32), which the object keeps from then on: that call synchronises the plan's stream and is refused with
 * SPDY_ERR_STATE inside a capture; if the allocation fails the object is left at (0, 0).  A host-only plan stores the values and
 * allocates nothing.  Every later setting changes two numbers and may be made at any time.  Checks: a NULL object SPDY_ERR_ARG, a
 * destroyed plan SPDY_ERR_STATE, then rtpp, then rtps.  The call carries a prefix of its own, as spdy_pobs_set and the spdy_mask_
 * calls do (DESIGN.md s23 says why).
 * With a setting other than (0, 0) every analysis call -- spdy_letkf_analyse_grid_dev, spdy_ens_letkf_dev and their masked forms,
 * at any weight stride, with any network -- has its transform or apply kernel write the raw increments into the workspace and
 * enqueues ONE launch more, which reads the ensemble and the workspace and writes the relaxed increments where the raw ones went
 * before; the increments may still take the place of the ensemble.  The masked form's results for the members in use are bit for
 * bit those of the relaxed call of an n-member object on the compacted members.  Bit-reproducible run to run.
 * spdy_letkf_field "inflation": f of every item of the latest relaxed call, (4 kx + 1) grids in the item order (ix,il each); part
 * of the object's main block, so the name is valid on every object (zero until the first relaxed call).                          */
int spdy_relax_set(spdy_letkf *l, double rtpp, double rtps);

/* ---- ensemble analysis, observations in time slots -----------------------------------------------------------------
 * The calls above take every observation as valid at the analysis time.  With these an observation is compared with each member's
 * forecast at the observation's own time, and one update uses all of them: the 4D-LETKF (Hunt et al. 2004; Hunt, Kostelich and
 * Szunyogh 2007, s4).  What is kept from an observation's time is per member only; everything that couples members is formed once,
 * at analysis time.  tests/letkfslots.py restates this section in NumPy.
 *   slots         the observations of the current network (spdy_letkf_set_obs or spdy_pobs_set) are divided into S contiguous
 *                 ranges by first[0..S]: first[0] = 0, first non-decreasing, first[S] = nobs; observation o is of slot s iff
 *                 first[s] <= o < first[s+1]; a slot may be empty; 1 <= S <= SPDY_MAX_SLOTS.  The order of the observations is not
 *                 touched: every sum over observations stays "o ascending".
 *   observing     a slot on an ensemble, for every observation o of the slot and every member e of nmem, in use later or not:
 *                 hx[o][e], the operator of "ensemble analysis" for a model-level or PS observation, that of "observations at a
 *                 pressure" for one at a pressure, every operation in that section's order -- the bits the plain analysis call
 *                 writes for the same member and state.  Only when the network holds an at-pressure observation (npobs > 0) also
 *                     slot_ps[o][e]  = ((w0 ps_e[i0] + w1 ps_e[i1]) + w2 ps_e[i2]) + w3 ps_e[i3]            the pb_e of that section
 *                     slot_out[o][e] = 1.0 if o is at a pressure and for some of its four points x_o < X_0 or x_o > X_{kx-1} with
 *                                      this member's ps, else 0.0; a target on an end level is in the column, a non-finite ps
 *                                      rejects nothing.
 *                 Nothing outside the slot's rows of these three arrays is written, and nothing per observation: hxmean, y,
 *                 departure, obs_lnsigma, obs_used and the per-call 1/error^2 stay as they are.
 *   analysis      an analysis call whose observation kernel is replaced by the finish kernel.  U: the members in use, all nmem
 *                 without a mask, otherwise the mask's ("member mask"); n = |U|; every sum over U ascending, by select:
 *                     hxmean_o = (sum_U hx[o][e]) / n        y[o][e] = e in U ? hx[o][e] - hxmean_o : 0.0
 *                     d_o      = value_o - hxmean_o          value as it stands when the kernel runs
 *                 and only when npobs > 0, ln sigma_o only for an at-pressure o:
 *                     ln sigma_o = x_o - (sum_U slot_ps[o][e]) / n
 *                     used_o   = (any e in U with slot_out[o][e] != 0) ? 0.0 : 1.0        reff_o = used_o ? rinv_o : 0.0
 *                 Everything after it is the analysis as it is -- transform, apply, relaxation, direct batch, spectral add -- masked
 *                 or not, at any weight stride, with any relaxation: C = sum_o r_o Y_o Y_o^T and b = sum_o r_o Y_o d_o with Y from
 *                 the slots' times, the increments dx_e = sum_f (x_f - xmean) T[f][e] on the ensemble passed to the analysis call.
 *                 For an at-pressure observation the vertical localisation and the out-of-column test use the surface pressure of
 *                 the slot's time: that is where the observation was.  n < 2: as under "member mask".
 * Four statements hold exactly:
 *   same state    if every non-empty slot was observed on the ensemble the slot analysis then gets, with the same mask, stride and
 *                 relaxation, the increments are bit for bit those of the plain call, and so are hx, hxmean, y, departure,
 *                 obs_lnsigma, obs_used, members_used, inflation and weights.
 *   isolation     observing slot s leaves every bit of the rows of hx, slot_ps and slot_out outside [first[s], first[s+1]) and of
 *                 every per-observation array; observing it again on another ensemble changes those rows only.
 *   late mask     a member the mask of the analysis call drops may hold NaN in its rows from any slot on: it enters nothing, and
 *                 the members in use get the bits of an n-member object that observed the same slots on the compacted members.
 *   one slot      S = 1 with first = {0, nobs}, observed on the analysed ensemble, is "same state"; a network with nobs == 0 gives
 *                 the plain call's result, zero increments at rho = 1.
 * spdy_slot_set(l, nslots, first): first has nslots + 1 entries; (0, NULL) returns the object to "no slots".  Host only, works on a
 * host-only plan, allocates nothing, may be called at any time.  The ranges are launch arguments, read when a call is enqueued: a
 * captured graph keeps the ranges of its capture and has to be captured again after a change.  Checks, in this order: a NULL object
 * SPDY_ERR_ARG ("null analysis object"), a destroyed plan SPDY_ERR_STATE; nslots outside [0, SPDY_MAX_SLOTS], a NULL first with
 * nslots > 0, first[0] != 0, a decreasing pair, first[nslots] != nobs SPDY_ERR_ARG.  A rejected call changes nothing.  The call
 * clears every slot's "observed" mark.  spdy_letkf_set_obs and spdy_pobs_set return the object to "no slots": their nobs and order
 * define the ranges.  spdy_letkf_table "slot_first": the nslots + 1 entries, count 0 with no slots.
 * spdy_slot_observe_grid_dev(l, slot, ug, vg, tg, qg, psg): the slot kernel on the caller's grids (the layout of
 * spdy_letkf_analyse_grid_dev).  spdy_slot_observe_dev(l, slot, vor, div, t, q, ps): time level 1 of the ensemble goes to the
 * object's grid workspace by the analysis' own inverse batch ("grid" then holds the gridded ensemble of that time, as after a
 * verify), and the slot kernel runs on it.  ONE launch after the transform: one thread per (observation of the slot, member), no
 * LDS, no atomics.  Nothing is allocated; both are capturable.  An empty slot enqueues nothing at all and is marked observed.  No
 * mask is needed: nothing shared is formed.  Checks: a NULL object SPDY_ERR_ARG, a destroyed plan SPDY_ERR_STATE; no slots set
 * SPDY_ERR_STATE; slot outside [0, nslots) SPDY_ERR_ARG; a NULL pointer SPDY_ERR_ARG; a host-only plan SPDY_ERR_NO_DEVICE last.
 * spdy_slot_analyse_grid_dev and spdy_slot_ens_letkf_dev: spdy_mask_letkf_analyse_grid_dev and spdy_mask_ens_letkf_dev as the
 * slot analysis; d_use NULL = all members.  The checks of those calls in their order and, before the device check: no slots set
 * SPDY_ERR_STATE; a non-empty slot not observed since the latest spdy_slot_set SPDY_ERR_STATE, the message names the slot.  The
 * marks are host-side, set when an observe is enqueued and not cleared by an analysis, so eager cycles and captured ones work alike.
 * Launches: those of the plain call of the same kind -- two on grids, five or six from spectra, one more at a weight stride, with
 * relaxation, with a mask -- with the finish kernel, one thread per observation over all nobs, in the observation kernel's place.
 * spdy_slot_nature_observe_dev(n, letkf, slot, noise): spdy_nature_observe_dev on the slot's range only -- value_o for o in the range
 * from the current truth by the same operator (an at-pressure observation clamped as there), the same draw, Philox counter (o, 0,
 * draws), then draws += 1; values outside the range keep their bits; an empty slot writes nothing and still counts.  Checks as
 * spdy_nature_observe_dev's, then no slots set SPDY_ERR_STATE, slot outside [0, nslots) SPDY_ERR_ARG, the device last.
 * spdy_letkf_field: "slot_ps", "slot_out", [nobs][nmem] each, part of the object's main block: the names are valid on every object.
 * The window ends at the analysis time: the analysed state is whatever arrays the analysis call gets.  A window centred on the
 * analysis time means handing spdy_slot_ens_letkf_dev a copy of the spectra kept at the centre; that is the caller's to do.
 * The calls carry a prefix of their own, as spdy_pobs_set and the spdy_mask_ calls do (DESIGN.md s23 says why).                  */
enum { SPDY_MAX_SLOTS = 32 };
int spdy_slot_set(spdy_letkf *l, int nslots, const int *first);
int spdy_slot_observe_grid_dev(spdy_letkf *l, int slot, const double *ug, const double *vg, const double *tg, const double *qg,
                               const double *psg);
int spdy_slot_observe_dev(spdy_letkf *l, int slot, const double *vor, const double *div, const double *t, const double *q,
                          const double *ps);
int spdy_slot_analyse_grid_dev(spdy_letkf *l, const double *ug, const double *vg, const double *tg, const double *qg, const double *psg,
                               double *du, double *dv, double *dt, double *dq, double *dps, const int *d_use);
int spdy_slot_ens_letkf_dev(spdy_letkf *l, double *vor, double *div, double *t, double *q, double *ps, const int *d_use);
struct spdy_nature;                   /* the nature run, "nature run" below */
int spdy_slot_nature_observe_dev(struct spdy_nature *n, spdy_letkf *letkf, int slot, double noise);

/* ---- ensemble analysis, background check and observation statistics ------------------------------------------------
 * The calls above take every observation at face value; one gross error damages every column within 2 c_h of it.  With these the
 * analysis tests every departure against spread plus error before the local analyses see it, and keeps, per group of observations,
 * the counts and sums an innovation table is made of -- on the device, so a captured cycle needs no host.  tests/letkfqc.py restates
 * this subsection in NumPy.  U: the members in use, all nmem without a mask, otherwise the mask's ("member mask"); n = |U|; every
 * sum over members runs over U ascending, by a select; every operation is one IEEE operation, nothing is contracted.
 *   check         after the observation stage of an analysis call -- the plain kernel, the at-pressure kernel or the slots' finish
 *                 kernel -- has written y_e and dep_o, for every observation o of the current network:
 *                     s2_o   = (sum_U y_e^2) / (n - 1)               each square rounded, then the sum, then one division
 *                     v_o    = s2_o + err_o * err_o                   err_o: the device's own copy of the error set_obs was given
 *                     rej_o  = dep_o * dep_o > g2 * v_o               g2 = gross * gross, formed once on the host
 *                     used_o = in_column_o && !rej_o                  in_column_o: what the observation stage wrote to obs_used
 *                                                                     (1 for a model-level network)
 *                     reff_o = used_o ? rinv_o : 0.0
 *                 A NaN makes the comparison false: it rejects nothing and propagates, as the out-of-column test does.  With
 *                 n < 2, or with gross == 0 (statistics only, below), the test is not made and nothing is rejected.  The local
 *                 analyses read reff: a rejected observation has r exactly 0 and, by "an observation with w == 0 takes no part",
 *                 enters no sum, so the increments are bit for bit those of the unchecked call on the network without the
 *                 rejected observations.  Its hx, hxmean, y and departure remain written, for diagnostics.
 *   groups        every observation has a group g_o in [0, ngroups), 1 <= ngroups <= SPDY_QC_MAX_GROUPS.  The default group is
 *                 the observation's variable (ngroups = 5); a caller may give a host table of nobs ints instead, for example the
 *                 instrument type or var * kx + lev.
 *   statistics    the object holds stats[SPDY_QC_SLOTS][SPDY_QC_MAX_GROUPS][10] doubles.  A call fills, of the slot it was enqueued
 *                 with (spdy_qc_set_slot), the ten numbers of every group g < ngroups, every time:
 *                     0 n_all   1 n_out   2 n_rej   3 n_used          counts, as doubles (check_o == 2, == 1, == 0 below)
 *                     4 sum dep   5 sum dep*dep   6 sum s2   7 sum err*err   8 sum dep*dep_b   9 sum dep_b
 *                 the sums over the group's used observations; each term is rounded once before it is added; dep_b is dep in an
 *                 analysis call ("stats-only" below otherwise).  An empty group gets exact zeros, a non-finite value stays in its
 *                 group's row.  The order of every sum is fixed: partial t, t = 0..1023, starts at +0.0 and takes the terms of the
 *                 group's used observations with o mod 1024 == t, o ascending; then for h = 512, 256, ..., 1 partial t becomes
 *                 partial t + partial (t + h) for every t < h; partial 0 is the sum.  The counts are formed the same way from
 *                 terms 1.0.  No atomics: two runs give the same bits, whatever the launch.
 * spdy_qc_set(l, gross, ngroups, group): gross finite and >= 0; group NULL: the default grouping, ngroups is ignored; otherwise
 * 1 <= ngroups <= SPDY_QC_MAX_GROUPS and group holds nobs ints for the current network, each in [0, ngroups); the table is copied.
 * A later spdy_letkf_set_obs or spdy_pobs_set returns the grouping to the default and keeps gross.  gross == 0 with the default
 * grouping is the state after create: OFF -- nothing more is enqueued, and every call above has the launches, graph nodes and bits
 * it always had.  gross == 0 with a grouping given: statistics without rejection, used_o is the observation stage's.  Checks, in this
 * order: a NULL object SPDY_ERR_ARG ("null analysis object"), a destroyed plan SPDY_ERR_STATE, gross, then with a grouping ngroups
 * and the first entry out of range SPDY_ERR_ARG; on a device plan an open capture SPDY_ERR_STATE.  A rejected call changes nothing.
 * On a device plan the call is stream-ordered and synchronises the plan's stream, like spdy_letkf_set_obs: it uploads the grouping,
 * and a setting that turns the check off gives "obs_used" back what the observation stage left (all 1.0 for a model-level
 * network).  The first setting that turns anything on allocates the qc block -- the grouping, the record, the kept departure and
 * the statistics, 20 bytes per observation of max_obs and 20 KB -- which the object keeps from then on; if the allocation fails the
 * object is left off.  A host-only plan stores the values and allocates nothing.
 * spdy_qc_set_slot(l, slot): the row of the statistics the next calls fill, 0 <= slot < SPDY_QC_SLOTS (0 after create).  Host only;
 * read when a call is enqueued, so a captured call keeps its slot.  Checks: a NULL object, a destroyed plan, then slot.
 * Once on, every analysis call on every route -- plain, masked, weight-interpolated, relaxed, from slots, on grids and from spectra
 * -- enqueues ONE launch more, between the observation stage and the transform, and the transform reads the per-call copy of
 * 1/error^2 whatever the network's kind.  One workgroup of 1024 threads per group walks the network in chunks of 1024; a thread
 * decides and writes the observations of its own group and keeps its partial sums in registers; one tree in LDS at the end.
 * spdy_letkf_field: "obs_used" reports used_o; "obs_check" [nobs]: 0.0 passed, 1.0 rejected by the check, 2.0 out of column -- out of
 * column wins -- of the latest analysis call with the check on; "obs_stats": the whole table.  Both names are of the qc block and
 * valid on every object of a device plan: asked for before any setting has made the block, the call makes it (it synchronises the
 * plan's stream then, and is refused with SPDY_ERR_STATE inside a capture) and leaves the check off; the arrays hold zeros.  "obs_rinv" [nobs]: reff_o, the per-call
 * copy of 1/error^2 the local analyses read -- part of the main block, written by every analysis call with the check on and by
 * every analysis of a network with observations at a pressure, zero until then.
 *   stats-only    spdy_qc_stats_grid_dev(l, ug, vg, tg, qg, psg, d_use, slot) and spdy_qc_stats_dev(l, vor, div, t, q, ps, d_use,
 *                 slot), for observation-minus-analysis and the products of Desroziers et al. (2005): the observation stage of the
 *                 analysis on the given ensemble (from spectra: after the analysis' inverse batch into the grid workspace), then the
 *                 check's launch in a mode that decides nothing.  used_o and check_o are those of the latest analysis call with
 *                 the check on, dep_b is that call's departure: both are kept in the qc block, which every such analysis call
 *                 writes.  Row `slot` is filled as above with dep the departure on the given state, so on the analysed state
 *                 sum dep*dep_b is sum d_oa d_ob over the analysis' used set.  It overwrites hx, hxmean, y and departure (and, for
 *                 a network with observations at a pressure, obs_lnsigma), as an analysis call does; obs_used and obs_check stay the
 *                 analysis'; no state changes.  It observes every observation on the state given, whatever slots are set.
 *                 d_use may be NULL.  Two launches on grids, one more with a mask; capturable.  Checks, in this order: a NULL
 *                 object SPDY_ERR_ARG, a destroyed plan SPDY_ERR_STATE; the check off, or no analysis call with the check on since
 *                 the network was set, SPDY_ERR_STATE; a NULL pointer, slot outside [0, SPDY_QC_SLOTS) SPDY_ERR_ARG; a host-only
 *                 plan SPDY_ERR_NO_DEVICE last.
 * The calls carry a prefix of their own, as spdy_pobs_set and the spdy_mask_ calls do (DESIGN.md s23 says why).                  */
enum { SPDY_QC_MAX_GROUPS = 64, SPDY_QC_SLOTS = 4 };
int spdy_qc_set(spdy_letkf *l, double gross, int ngroups, const int *group);
int spdy_qc_set_slot(spdy_letkf *l, int slot);
int spdy_qc_stats_grid_dev(spdy_letkf *l, const double *ug, const double *vg, const double *tg, const double *qg, const double *psg,
                           const int *d_use, int slot);
int spdy_qc_stats_dev(spdy_letkf *l, const double *vor, const double *div, const double *t, const double *q, const double *ps,
                      const int *d_use, int slot);

/* ---- ensemble analysis, adaptive inflation --------------------------------------------------------------------------
 * The scalar rho of spdy_letkf_set_localization is one number for a radiosonde-dense continent and an empty ocean.  With these calls
 * the object carries a field rho[kx][ncol] (level-major, column j * ix + i), which every analysis call reads in the scalar's place
 * and then advances from the call's own innovation statistics (Miyoshi 2011; Li et al. 2009), on the device: a captured cycle
 * advances the field on every replay.  tests/letkfinfl.py restates this subsection in NumPy.  U: the members in use, all nmem
 * without a mask, otherwise the mask's ("member mask"); n = |U|; sums over members run ascending; every operation is one IEEE
 * operation, nothing is contracted.
 *   per observation o, once per call:
 *       s2_o = (sum_e y_oe^2) / (n - 1)                       "background check"'s s2 with its bits: y of a member not in use is 0.0
 *                                                             and adds an exact zero
 *   per column c and level k, over the observations ascending, wh, w and r formed with the local analysis' own expressions (the
 *   chord, asin, Gaspari and Cohn's function, c_h, c_v, ln fsg_k, ln sigma_o) and the 1 / error^2 the call's local analyses read
 *   (reff: "obs_rinv" for a network with observations at a pressure or with the background check on, rinv otherwise), so the
 *   observations that enter the sums are exactly those that enter C of that column and level:
 *       wh = gc(dist(c, o) / c_h)                             skipped if wh == 0
 *       w  = c_v > 0 ? wh * gc(|ln fsg_k - ln sigma_o| / c_v) : wh
 *       r  = w * reff_o
 *       if r != 0:   p1 += r * (dep_o * dep_o);   p2 += r * s2_o;   p3 += w
 *   the update, with rho = rho[k][c] before the call and vb = sigma_b * sigma_b formed on the host:
 *       if p3 > 0 and p2 > 0:
 *           ro  = (p1 - p3) / p2                              the observed inflation: (d^T R^-1 d - trace) / trace(H P H^T R^-1)
 *           t   = (rho * p2 + p3) / p2
 *           vo  = (2 / p3) * (t * t)                          its error variance, p3 the effective number of observations
 *           g   = vb / (vo + vb)
 *           est = rho + g * (ro - rho)
 *           rho' = est finite ? fmin(fmax(est, rho_min), rho_max) : rho
 *       else rho' = rho
 *   A non-finite estimate leaves rho as it is: here a NaN does NOT propagate, unlike everywhere else in this header.  rho outlives
 *   the call, and a NaN in it would poison its column for the rest of the run.  (The test is made on est, before the bounds: fmin
 *   and fmax return their other argument for a NaN, so after them nothing non-finite would be left to see.)  With n < 2 neither
 *   launch writes anything.  ps is analysed with level kx-1's transform and so uses rho[kx-1].
 *   order within a call (Miyoshi's): the local analyses of this call use rho as it was before the call; the estimate is enqueued
 *   after everything else of the call -- after the relaxation's launch, if any -- and writes rho in place for the next call.
 * spdy_infl_set(l, on, sigma_b, rho_min, rho_max): sigma_b >= 0, 0 < rho_min <= rho_max, all finite.  sigma_b == 0 is legal: g = 0,
 * the field is used and frozen.  Checks, in this order: a NULL object SPDY_ERR_ARG, a destroyed plan SPDY_ERR_STATE, sigma_b,
 * rho_min, rho_max SPDY_ERR_ARG; then, where the call has to allocate, an open capture SPDY_ERR_STATE.  A rejected call changes
 * nothing.  OFF is the state after create: nothing more is enqueued, and every call above has the launches, graph nodes and bits it
 * always had.  The first "on" on a device plan allocates a block of its own -- rho[kx][ncol], filled with the object's scalar rho of
 * that moment; infl_parm[3][kx][ncol], p1 | p2 | p3 of the latest call, zeroed; obs_s2[max_obs] -- which the object keeps from then
 * on; that call synchronises the plan's stream, and if the allocation fails the object is left off.  Later settings change the four
 * numbers only; they are read when a call is enqueued, so a captured call keeps those of its capture.  A host-only plan stores the
 * values and allocates nothing.  spdy_letkf_table "adaptive_inflation" gives {on, sigma_b, rho_min, rho_max} as they are stored.
 * spdy_infl_fill(l, rho0): rho0 finite and > 0; fills the field uniformly (it makes the block if there is none, and leaves the
 * feature off then).  Stream-ordered, synchronises the plan's stream, refused inside a capture.  Checks: a NULL object, a destroyed
 * plan, rho0, a host-only plan SPDY_ERR_NO_DEVICE, an open capture.
 * While adaptive inflation is on the scalar rho is not read by the local analyses; spdy_letkf_set_localization, spdy_letkf_set_obs,
 * spdy_pobs_set, spdy_slot_set and spdy_qc_set leave the field alone, and so do the stats-only calls and spdy_slot_observe*,
 * which enqueue nothing of this.
 * Once on, every analysis call on every route -- plain, masked, weight-interpolated, relaxed, from slots, at-pressure, with the
 * background check, on grids and from spectra -- launches the local analyses in a form that reads the field (the diagonal of level
 * k of column c is (n - 1) / rho[k][c], one IEEE division: the bits an object with that scalar has) and enqueues TWO launches
 * more, last: one thread per observation writes obs_s2; one workgroup per grid column -- every column, whatever the weight stride:
 * the estimate does not depend on where transforms are solved -- scans the network as the local analysis does, lane k carries
 * level k's sums in registers, and updates rho.  An adaptive analysis has two graph nodes more than the same call with the
 * feature off, whatever the route and also for an empty network.  No atomics: two runs give the same bits.
 * spdy_letkf_field: "rho" [kx][ncol], writable -- a caller sets any field with a device copy and restarts a run from a saved one;
 * "infl_parm" [3][kx][ncol]; "obs_s2" [nobs].  The three names are valid on every object of a device plan: asked for before the
 * block exists, the call makes it (it synchronises then, and is refused with SPDY_ERR_STATE inside a capture) and leaves the
 * feature off.  The calls carry a prefix of their own (DESIGN.md s23 says why).                                                    */
int spdy_infl_set(spdy_letkf *l, int on, double sigma_b, double rho_min, double rho_max);
int spdy_infl_fill(spdy_letkf *l, double rho0);

/* ---- nature run: the truth of a twin experiment, observations drawn from it, an ensemble scored against it ------
 * The reference has none of this; this section defines it, and tests/nature.py restates it in NumPy.  With it a twin experiment's
 * cycle {nature step, ensemble steps, observe, verify the background, spdy_ens_letkf_dev, verify the analysis, first_step} is a
 * sequence of enqueues that one captured graph can hold; the host reads 3 (4 kx + 1) doubles per verified ensemble.
 * A spdy_nature is an object made on a plan (the plan section: one lifetime rule).  It owns, in one device block,
 *   truth         the gridded truth: u, v (true wind), t, q (g/kg) at kx levels and ps = log(p/p0), (4 kx + 1) grids -- one member
 *                 of the analysis' gridded layout; row f = v kx + k for variable v = 0..3 and level k, row 4 kx for ps;
 *   state         two 64-bit words {seed, draws};
 *   scores        a table [capacity][3][4 kx + 1] of doubles: rmse | bias | spread of every row, one slot per verified ensemble.
 * spdy_nature_create(plan, seed, capacity >= 1, &n): needs the sigma levels and max_batch >= 2 kx + 1, allocates everything and
 * runs the inverse batch of spdy_nature_set_state_dev once on zero spectra, so nothing is allocated afterwards and every *_dev call
 * can be captured; draws = 0.  spdy_nature_reset(n, seed): the seed, and draws = 0 (stream-ordered upload, synchronising, not in a
 * capture).  spdy_nature_draws: the counter (synchronising).  spdy_nature_field: "truth", "scores", "state" (the two words).
 * spdy_nature_set_state_dev(n, vor, div, t, q, ps): the single-state spectra of time level 1.  ONE spdy_inverse_batch_segs_dev,
 * the call spdy_ens_letkf_dev makes with nmem = 1 (kx pairs as true wind, the segments t | q of kx fields and ps of 1), into truth.
 * spdy_nature_observe_dev(n, letkf, noise): for the nobs observations of letkf's latest spdy_letkf_set_obs -- their values are
 * ignored, zeros will do: they define the network -- it writes letkf's device value table,
 *       h_o     = ((w0 x0 + w1 x1) + w2 x2) + w3 x3           the operator of the analysis, on the truth
 *       value_o = h_o + (noise * error_o) * z_o
 * error_o the error given to set_obs (the analysis object keeps it on the device), z_o the real part of SPPT's draw: Philox4x32-10
 * with counter (o, 0, draws lo, draws hi) and key (seed lo, seed hi) through the same randn, so the noise of an observation depends
 * on (seed, draws, o) only.  With noise == 0 the product is not formed: value_o has the bits of h_o.  A second launch then sets
 * draws += 1, so every replay of a captured observe draws fresh noise.  nobs == 0 writes nothing and still counts.  One thread per
 * observation, two launches (one with nobs == 0).  The next analysis call reads these values; set_obs overwrites them.
 * spdy_nature_verify_dev(n, letkf, vor, div, t, q, ps, slot): time level 1 of an ensemble of letkf's nmem members in the layout of
 * spdy_ens_letkf_dev goes to the grid by the call the analysis makes, into letkf's grid workspace (the next analysis overwrites it
 * anyway), and every row f is scored against the truth.  With g_j the plan's Gaussian weights of the rows, south first, divided by
 * their sum over j ascending, <a> = sum_j g_j ((sum_i a[j][i]) / ix) over j ascending, and per grid point
 *       d_e  = x_e - truth                                    the members' errors
 *       mbar = (sum_e d_e, e ascending) / E                   the error of the ensemble mean m: m - truth
 *       s2   = (sum_e (d_e - mbar)^2, e ascending) / (E - 1)  the sample variance: d_e - mbar is x_e - m
 *       rmse_f = sqrt(<mbar^2>)     bias_f = <mbar>     spread_f = sqrt(<s2>)
 * The mean is formed on the errors and not on the members because E equal values do not in general sum to E times the value in
 * floating point: on the errors an ensemble whose members all equal the truth scores exactly 0 in all three, and the subtraction
 * that cancels is done once, exactly where the members are close to the truth, before anything is rounded.
 * spdy_nature_verify_grid_dev(n, nmem, ug, vg, tg, qg, psg, slot) scores an ensemble that is on the grid already, in the layout of
 * spdy_letkf_analyse_grid_dev, 2 <= nmem <= 32: the two score launches alone, no analysis object.
 * scores[slot] receives rmse | bias | spread, (4 kx + 1) each.  Three launches: the inverse batch, one workgroup per (row,
 * latitude) that sums a latitude's points in a fixed tree, one thread per row that adds the latitudes.  No atomics; every sum is in
 * an order that does not depend on the launch; two runs are bit-equal; a row's scores depend on that row's grids only, so a
 * non-finite value makes the three scores of its row NaN and touches no other row.
 * Checks, in this order -- create: a NULL plan, capacity < 1, a NULL result pointer, max_batch SPDY_ERR_ARG; no sigma levels, an
 * open capture SPDY_ERR_STATE.  Every other call: a NULL object SPDY_ERR_ARG, a destroyed plan SPDY_ERR_STATE; observe and verify
 * then the analysis object in the same way and SPDY_ERR_ARG if it is of another plan; then noise < 0 or not finite, nmem outside [2, 32], slot
 * outside [0, capacity), a NULL pointer, an unknown field name SPDY_ERR_ARG; an open capture SPDY_ERR_STATE (reset, draws); a host-only
 * plan SPDY_ERR_NO_DEVICE last.  create works on a host-only plan.  A failing call enqueues nothing.                            */
typedef struct spdy_nature spdy_nature;
int spdy_nature_create(spdy_plan *plan, unsigned long long seed, int capacity, spdy_nature **n);
int spdy_nature_destroy(spdy_nature *n);
int spdy_nature_reset(spdy_nature *n, unsigned long long seed);
int spdy_nature_draws(spdy_nature *n, long long *count);
int spdy_nature_field(spdy_nature *n, const char *name, double **d_ptr);
int spdy_nature_set_state_dev(spdy_nature *n, const double *vor, const double *div, const double *t, const double *q, const double *ps);
int spdy_nature_observe_dev(spdy_nature *n, spdy_letkf *letkf, double noise);
int spdy_nature_verify_dev(spdy_nature *n, spdy_letkf *letkf, const double *vor, const double *div, const double *t, const double *q,
                           const double *ps, int slot);
int spdy_nature_verify_grid_dev(spdy_nature *n, int nmem, const double *ug, const double *vg, const double *tg, const double *qg,
                                const double *psg, int slot);
/* the two verify calls under a member mask ("member mask" above): d_use NULL = the calls above */
int spdy_mask_nature_verify_dev(spdy_nature *n, spdy_letkf *letkf, const double *vor, const double *div, const double *t, const double *q,
                                const double *ps, const int *d_use, int slot);
int spdy_mask_nature_verify_grid_dev(spdy_nature *n, int nmem, const double *ug, const double *vg, const double *tg, const double *qg,
                                     const double *psg, const int *d_use, int slot);

/* ---- HIP graphs: replaying a fixed sequence of device-resident calls --------------------------------
 * A model step is the same sequence of small launches every time (tendencies.f90:89-107, :212-234,
 * time_stepping.f90:56-121: ~90 inverse and ~70 direct transforms plus the spectral operators, 7 horizontal
 * diffusions and implicit_terms at T30 L8).  At those batch sizes a launch costs as much as the kernel, so the
 * sequence can be recorded once and replayed as one graph launch:
 *     spdy_graph_begin(plan);  <any *_dev calls on this plan>;  spdy_graph_end(plan, &g);  spdy_graph_launch(g); ...
 * Between begin and end nothing executes; the calls are captured from the plan's stream (which must not be the
 * legacy default stream) with the pointer arguments they were given.  Host-pointer entry points, profiling and
 * spdy_plan_synchronize are refused while a capture is open (SPDY_ERR_STATE).  spdy_graph_launch enqueues the
 * whole sequence on the plan's stream.  (The reference has no counterpart: it calls the transforms one field
 * at a time, spectral.f90:98-122.)                                                                          */
typedef struct spdy_graph spdy_graph;
int spdy_graph_begin(spdy_plan *plan);
int spdy_graph_end(spdy_plan *plan, spdy_graph **graph);
int spdy_graph_launch(spdy_graph *graph);
int spdy_graph_destroy(spdy_graph *graph);
/* Number of nodes of a captured graph (one per kernel launch / collective of the captured calls): what bench.py and the
 * step tests report as "launches per step". */
int spdy_graph_num_nodes(spdy_graph *graph, int *nodes);

#ifdef __cplusplus
}
#endif
#endif /* SPDY_H */
