// Fused, persistent, wave-specialised T30 kernels (included by spdy_kernels.hip; shares its radix templates).
//
// One 448-thread workgroup per CU (7 waves) walks over tiles of BT = 2 fields.  A whole transform
// (Legendre contraction on the matrix cores + 48 row FFTs per field) happens inside LDS, so HBM sees
// exactly the algorithmic bytes: spec in / grid out (inverse) or grid in / spec out (direct).
//
// Roles (decided once, two separate persistent loops that meet at one s_barrier per step):
//   * waves 0..3, "Legendre waves": each owns 8 zonal wavenumbers and keeps the matrix-core A operands
//     of those (60 / 72 doubles per lane) RESIDENT in VGPRs for the whole kernel -- the Legendre table
//     is read from L2 once per workgroup instead of once per tile (that re-streaming was 2x the
//     tile's HBM bytes);
//   * waves 4..6, "FFT waves": each owns 32 grid rows of the tile and does everything for them
//     wave-locally (no barrier inside): the global<->LDS transposes, the row FFTs, the register
//     prefetch of the next tile.
// The two groups work on consecutive tiles through double-buffered LDS (direct: FFT waves fill
// buffer k while Legendre waves drain buffer k-1; inverse: the other way round), so the FP64 phases
// of one group overlap the memory phases of the other inside a single CU.
//
// Matrix cores: v_mfma_f64_4x4x4_4b_f64 -- four independent 4x4x4 blocks per instruction, 16 cycles,
// same flop rate as the 16x16x4 form (measured on gfx950: 69.9 vs 67.9 TFLOP/s; FP64 MFMA and FP64
// VALU share one datapath, so padded tiles steal time from the FFTs).  With 2 fields the N
// dimension (field x re/im) is exactly 4, the blocks tile latitudes (inverse) or total-wavenumber
// rows (direct) 4 at a time, and both parities are packed into one instruction where a parity alone
// would leave blocks empty.  Lane layout (probed, tools/mfma_4x4x4_layout.hip):
//     block = (lane>>2)&3 ;  A: i = lane&3, k = lane>>4 ;  B: j = lane&3, k = lane>>4 ;
//     D: j = lane&3, i = lane>>4.
// Legendre wave w owns zonal wavenumbers m'(s,w), s = 0..7, all in [4s, 4s+3]: the k-step count of
// slot s is bounded at compile time by 4 - (s>>1) per parity and the four waves carry equal work.
#ifdef SPDY_TRACE_TAIL      /* record the LAST eight steps of the walk instead of the first eight */
#define SPDY_TRACE_STEP(k_, ks_) ((k_) - ((ks_) + 2 - 8))
#else
#define SPDY_TRACE_STEP(k_, ks_) (k_)
#endif
#ifdef SPDY_PHASE_TRACE
// Debug-only phase timestamps (s_memtime) of workgroup 0: [kernel 0/1][step < 8][mark < 8][wave < 7 (8 slots)]
__device__ long long g_phase_trace[2 * 8 * 8 * 8];
#define PHASE_MARK(kern, mark)                                                                        \
    do {                                                                                              \
        if (blockIdx.x == 0 && lane == 0 && (unsigned)titer < 8u)                                             \
            g_phase_trace[(((kern) * 8 + titer) * 8 + (mark)) * 8 + w] = __builtin_amdgcn_s_memtime(); \
    } while (0)
// whole-kernel timeline of workgroups 0 and gridDim-1:
// [kernel][wg 0/last][wave][0 = entry, 1+k = top of step k (k < 25), 26..30 = prologue marks, 31 = exit]
__device__ long long g_timeline[2 * 2 * 8 * 32];
// ... and entry / exit of EVERY workgroup in the 100 MHz real-time counter (comparable across the chip): [kernel][wg < 512][2]
__device__ long long g_wg_span[2 * 512 * 2];
#define TL_MARK(kern, idx)                                                                            \
    do {                                                                                              \
        const int i_ = (idx);                                                                         \
        if ((i_ == 0 || i_ == 31) && threadIdx.x == (i_ == 0 ? 0 : 64 * (w)) && (threadIdx.x == 0 || (w) == 4) && blockIdx.x < 512) \
            g_wg_span[((kern) * 512 + blockIdx.x) * 2 + (i_ == 31)] = __builtin_amdgcn_s_memrealtime(); \
        if ((blockIdx.x == 0 || blockIdx.x == gridDim.x - 1) && lane == 0 && i_ < 32)                 \
            g_timeline[(((kern) * 2 + (blockIdx.x ? 1 : 0)) * 8 + w) * 32 + i_] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#elif defined(SPDY_WG_SPAN)
// Only the entry / exit of every workgroup (two stores per workgroup: does not perturb the walk) -- tools/wg_span.py
__device__ long long g_wg_span[2 * 512 * 2];
#define PHASE_MARK(kern, mark) do { } while (0)
#define TL_MARK(kern, idx)                                                                            \
    do {                                                                                              \
        const int i_ = (idx);                                                                         \
        if ((i_ == 0 || i_ == 31) && threadIdx.x == (i_ == 0 ? 0 : 64 * (w)) && (threadIdx.x == 0 || (w) == 4) && blockIdx.x < 512) \
            g_wg_span[((kern) * 512 + blockIdx.x) * 2 + (i_ == 31)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define PHASE_MARK(kern, mark) do { } while (0)
#define TL_MARK(kern, idx) do { } while (0)
#endif

// Streaming (non-temporal) access to a transform's grid-side array.  A large batch passes through the caches once: with the
// default policy its lines are allocated in L2 and the 256 MB Infinity Cache anyway, and the write-back of one kernel's
// output then runs into the next kernel's reads (measured at T30, B = 6144: direct 82 -> 62 us with nt loads, inverse 63 ->
// 57 us with nt stores; nt on the SPECTRA is a loss -- they are re-read by the next kernel while still cached).  Small,
// model-shaped batches keep the default policy: their consumer kernels find the data in L2.  STREAM is a template
// parameter of the fused kernels, chosen per launch by stream_policy().
typedef double spdy_d2v __attribute__((ext_vector_type(2)));
template <bool STREAM>
__device__ __forceinline__ double2 grid_load2(const double2 *p)
{
    if (STREAM) {
        const spdy_d2v v = __builtin_nontemporal_load(reinterpret_cast<const spdy_d2v *>(p));
        return make_double2(v.x, v.y);
    }
    return *p;
}
template <bool STREAM>
__device__ __forceinline__ void grid_store2(double2 *p, double2 v)
{
    if (STREAM) {
        spdy_d2v w;
        w.x = v.x;
        w.y = v.y;
        __builtin_nontemporal_store(w, reinterpret_cast<spdy_d2v *>(p));
    } else
        *p = v;
}
// Spectra stores of the direct kernel's copy-out.  A streaming launch (STREAM) writes them through to memory (sc0 sc1): with
// the default write-back policy up to 32 MB of them are still dirty in the eight L2s when the kernel ends, and the
// end-of-kernel release has to flush them before the next kernel may start (61.8 -> 59.5 us per launch at B = 6144; the
// inverse kernel that reads them next is unaffected -- they reach it through the Infinity Cache either way; `nt` instead
// costs that kernel 9 us).  Model-sized launches keep the default policy: their consumer is faster with it (T30 L8 step
// 34.7 vs 35.1 us).  The store is followed by two wait states, so its data registers may be rewritten at once.
// (experiment knob SPDY_G2S_SPEC_POLICY: 0 default everywhere, 1 sc1, 2 sc0 sc1, 3 nt)
#ifndef SPDY_G2S_SPEC_POLICY
#define SPDY_G2S_SPEC_POLICY 2
#endif
__device__ __forceinline__ void store2_wt(double2 *p, double2 v)
{
    spdy_d2v w;
    w.x = v.x;
    w.y = v.y;
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" :: "v"(p), "v"(w) : "memory");
}
template <bool STREAM>
__device__ __forceinline__ void spec_store2(double2 *p, double2 v)
{
    if (STREAM && SPDY_G2S_SPEC_POLICY != 0) {
        spdy_d2v w;
        w.x = v.x;
        w.y = v.y;
#if SPDY_G2S_SPEC_POLICY == 1
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(w) : "memory");
#elif SPDY_G2S_SPEC_POLICY == 3
        asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" :: "v"(p), "v"(w) : "memory");
#else
        asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" :: "v"(p), "v"(w) : "memory");
#endif
    } else
        *p = v;
}
#define G2S_SPEC_STORE(ptr_, val_) spec_store2<STREAM>(&(ptr_), (val_))
#ifndef SPDY_STREAM_MIN_MB
#define SPDY_STREAM_MIN_MB 16
#endif
constexpr long STREAM_MIN_BYTES = (long)SPDY_STREAM_MIN_MB << 20;   // grid-side bytes of one launch from which it streams
inline bool stream_policy(long grid_bytes) { return grid_bytes >= STREAM_MIN_BYTES; }
bool streams(long grid_bytes) { return stream_policy(grid_bytes); }
// (spdy_kernels.hpp)  Measured on the captured steps: T63 L16 72.0 -> 68.5 us, T63 L8 54.5 -> 52.7 us with the by-chunk inverse
// launch (13-27 MB of grids), the grid tendencies (11-21 MB), the row workspace and the staged contraction's spectra written
// through; the same at T30 L8 (2.7-3.4 MB per launch) costs 0.7 us -- hence a threshold between the two.
bool write_through_policy(const DevPlan &p, long output_bytes)
{
    const long mb = p.lo.wt_min_mb;
    return mb > 0 && output_bytes >= (mb << 20);
}

namespace t30 {
constexpr int TRUNC = 30, MX = 31, NX = 32, IY = 24, IL = 48, IX = 96;
constexpr int BT = 2, TROWS = BT * IL;                      // 96 grid rows per tile
constexpr int NLW = 4, NFW = 3, NTHR = 64 * (NLW + NFW);    // Legendre waves, FFT waves, 448 threads
constexpr int SPEC_C = MX * NX;                             // complex coefficients per field (992)
// inverse: compact Fourier tile, row slot = 62 doubles (496 B = 31*16 B: ds_read_b128 conflict-free)
constexpr int F_ROW = 62, F_TILE = TROWS * F_ROW;           // doubles
constexpr int XROWS = 640, XW = 2 * BT;                     // packed B-operand rows of XW doubles, see xoff()
constexpr int S2G_DUMMY = 8;                                // sink for the one unused (wave 0, slot 7) wavenumber
constexpr int XS_TILE = XROWS * XW;
constexpr int S2G_LDS = (2 * F_TILE + 2 * XS_TILE + S2G_DUMMY) * 8;   // 136,256 B: both images double-buffered
// direct: grid/Fourier row slots, stride 99 (odd: conflict-free row-per-lane FFT access)
constexpr int G_ROW = 99, G_TILE = TROWS * G_ROW;
constexpr int G_TW = 48;                                    // last-stage twiddle pairs, per-lane selectable: [12][column h][re, im]
constexpr int G2S_LDS = (2 * G_TILE + G_TW) * 8;            // 152,448 B: double-buffered row slots + twiddles

__device__ __forceinline__ int mslot(int s, int w) { return (s & 1) ? 4 * s + 3 - w : 4 * s + w; }
// first packed row of zonal wavenumber m in the inverse B-operand image: wavenumbers 8q..8q+7 hold
// 2 parities x (4-q) k-steps x 4 rows each
__device__ __forceinline__ int xoff(int m) { const int q = m >> 3; return 64 * (4 * q - (q * (q - 1)) / 2) + 8 * (m & 7) * (4 - q); }
}  // namespace t30

#ifndef SPDY_G2S_NEARLY
#define SPDY_G2S_NEARLY 3     // row groups (of 8) of the next tile prefetched before the FFT; the rest after it
#endif
#define MFMA4(a, b, c) __builtin_amdgcn_mfma_f64_4x4x4f64((a), (b), (c), 0, 0, 0)


// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains vmcnt(0), i.e. it would
// wait for every global load in flight (next-tile prefetch, bulk A-operand loads) at every phase
// boundary; nothing is exchanged between waves through global memory here, so only lgkmcnt matters.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ------------------------------------------------------------------------------------------
// spec_to_grid, fused (spectral.f90:98-110).  grid[nb][48][96] <- spec[nb][32][31] complex
//   step k: Legendre waves turn spectra image k%2 into Fourier tile k%2 (tile k), then stage the
//           prefetched spectra of tile k+1 into image (k+1)%2; FFT waves transform Fourier tile
//           (k-1)%2 (tile k-1) and stream the grid rows out.
// ------------------------------------------------------------------------------------------
struct S2gMixed {                                           // MODE 3 only
    const double *spec_p; const int *kcos_p; int kcos_all_p; double *grid_p; int npairs, nplain;
    // optional gradient tiles [npairs, npairs + ngrad): psi[i] -> (gx[i], gy[i]) (spectral.f90:124-144 + two spec_to_grid).  A
    // gradient is the uvspec stencil with vor = 0, div = psi and the tables (gradx, gradym, gradyp) in place of (uvdx, uvdym,
    // uvdyp): psdx = i gradx psi, psdy = -gradym psi(n-1) + gradyp psi(n+1); the extra terms are exact zeros.  `zero` is one
    // all-zero spectrum that every gradient tile reads as its vorticity.
    int ngrad, kcos_grad; const double *psi; double *gx, *gy; const double *zero;
    // the plain spectra may come from up to four separate arrays (the reference reads vor, div, t, tr of one time level from
    // four prognostic arrays, tendencies.f90:89-101): plain fields [0, seg_first[0]) are spec_p, [seg_first[i], seg_first[i+1])
    // seg_spec[i]; unused entries have seg_first = INT_MAX.  The grids of all of them are one stack, grid_p.
    const double *seg_spec[3]; int seg_first[3];
};
__device__ __forceinline__ const double *s2g_plain_field(const S2gMixed &m, int f)
{
    const double *base = m.spec_p;
    int first = 0;
    UNROLL for (int i = 0; i < 3; ++i)
        if (f >= m.seg_first[i]) { base = m.seg_spec[i]; first = m.seg_first[i]; }
    return base + (long)(f - first) * (2 * t30::SPEC_C);
}
// MODE 0: the tile's two fields are consecutive fields of `spec`, output to consecutive fields of `grid`.
// MODE 1 = uvspec + 2 x spec_to_grid (spectral.f90:173-196, tendencies.f90:98-100) in one pass: tile i is the pair
//          (vor[i], div[i]) = (spec, spec2); the staging turns it into (U, V) on the fly; outputs ug = grid, vg = grid2.
// MODE 2 = grad + 2 x spec_to_grid (spectral.f90:124-144, tendencies.f90:121-123): tile i is psi[i] = spec, staged
//          as (dpsi/dx, dpsi/dy); outputs grid, grid2.   In MODE 1/2 nb counts tiles and kcos_all applies to both.
// PART: the small-batch form.  A launch with fewer than a third as many tiles as CUs would leave most of the chip idle while
// every workgroup walks through a whole tile's latency chain (operand image, 72 matrix instructions, 32 row FFTs per wave).
// The latitudes of legendre_inv are independent (legendre.f90:84-110), so the work item becomes (tile, third of the
// latitudes): workgroup 3 t + q synthesises latitudes 8 q .. 8 q + 7 of both hemispheres of tile t -- ONE packed matrix
// instruction per k-step (blocks 0, 1: even-n sums, blocks 2, 3: odd-n sums, as for latitudes 16..23 in the whole-tile walk)
// from a third of the operand image -- and its FFT wave 0 transforms those 32 grid rows (FFT waves 1 and 2 only keep the
// barriers).  Every (latitude, column) is the same chain of matrix instructions on the same operands as in the whole-tile
// walk: bit-identical results (tests/test_gpu_determinism.py).  The Fourier tile holds the part's rows compactly:
// local row = 16 field + (south: lat - 8 q | north: 8 + (7 - (lat - 8 q))), i.e. ascending grid rows in both halves.
template <int MODE, bool STREAM, bool PART = false>
__global__ __launch_bounds__(t30::NTHR, 2) void s2g_fused_t30_kernel(DevPlan p, int nb, const double *__restrict__ spec,
                                                                    const double *__restrict__ spec2,
                                                                    const int *__restrict__ d_kcos, int kcos_all,
                                                                    double *__restrict__ grid, double *__restrict__ grid2,
                                                                    S2gMixed mixed)
{
    using namespace t30;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *lds_f = lds, *lds_x = lds + 2 * F_TILE, *sink = lds + 2 * F_TILE + 2 * XS_TILE;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    TL_MARK(0, 0);
    constexpr bool DERIVED = MODE == 1 || MODE == 2, MIXED = MODE == 3, UVSPEC = MODE == 1 || MODE == 3;
    // MODE 3 = one launch for a model step's whole inverse batch: tiles [0, npairs) are (vor, div) pairs handled as in
    // MODE 1 (outputs grid, grid2, kcos_all), the tiles after them plain 2-field tiles of mixed.spec_p -> mixed.grid_p
#define IS_DER(t_) (DERIVED || (MIXED && (int)(t_) < nder))
#define IS_GRAD(t_) (MIXED && (int)(t_) >= mixed.npairs && (int)(t_) < nder)
    const int nder = MIXED ? mixed.npairs + mixed.ngrad : 0;     // derived tiles of a mixed batch: uvspec pairs, then gradients
    const int ntiles = DERIVED ? nb : MIXED ? nder + (mixed.nplain + BT - 1) / BT : (nb + BT - 1) / BT;
    // this workgroup's tiles: wg0, wg0 + wgs, ...  (PART: the one tile blockIdx.x / 3, latitude third `part`)
    const int wg0 = PART ? (int)blockIdx.x / 3 : (int)blockIdx.x, wgs = PART ? (1 << 28) : (int)gridDim.x;
    const int part = PART ? (int)blockIdx.x - 3 * wg0 : 0;
    const int ksteps = PART ? (wg0 < ntiles ? 1 : 0) : (wg0 < ntiles) ? (ntiles - 1 - wg0) / wgs + 1 : 0;   // tiles of this workgroup

    // (the packed-spectra images are zero-filled below, once the first loads are in flight)
    if (w < NLW) {
        // =================================================================== Legendre waves
        // resident MFMA A operands: slot s -> (4 - s/2) k-steps x {even-n lat 0..15, odd-n lat 0..15, packed lat 16..23}
        double areg[60];
        // 30 16-byte loads from the register image (two fragments each) instead of 60 8-byte ones
#define S2G_LOAD_AREG()                                                                                        \
    do {                                                                                                       \
        const double2 *img = PART ? reinterpret_cast<const double2 *>(p.img_s2g3) + (long)(part * NLW + w) * 10 * 64 + lane \
                                  : reinterpret_cast<const double2 *>(p.img_s2g) + (long)w * 30 * 64 + lane;   \
        UNROLL for (int q = 0; q < (PART ? 10 : 30); ++q) {                                                    \
            const double2 v = img[q * 64];                                                                     \
            areg[2 * q] = v.x;                                                                                 \
            areg[2 * q + 1] = v.y;                                                                             \
        }                                                                                                      \
    } while (0)
        if (STREAM) S2G_LOAD_AREG();       // throughput launches: requested first (0.5-1 us of 56 better than behind the first tile)
        // spectra staging: one tile = 2 fields = 64 spectral rows (field b, index n) of 31 complex.
        // Thread (rsub = tid/32, m = tid%32) moves column m of rows rsub + 8k: n = rsub + 8(k&3), b = k>>2,
        // so every global and LDS offset is base + constant.  (named scalars: an array ends up in scratch)
        const int pm = tid & 31, rsub = tid >> 5, pmc = min(pm, MX - 1);
        double2 pre0, pre1, pre2, pre3, pre4, pre5, pre6, pre7;
#define S2G_PREFETCH(tile_)                                                                                    \
    do {                                                                                                       \
        const int tc_ = min((int)(tile_), ntiles - 1); /* past the end: harmless re-read */                   \
        const double2 *src_ = reinterpret_cast<const double2 *>(spec) + (long)tc_ * BT * SPEC_C + rsub * MX + pmc; \
        const int o1_ = (nb - tc_ * BT) > 1 ? SPEC_C : 0; /* second field of the tile, if it exists */        \
        /* only the coefficients the transform reads (m' + n <= trunc+1, about half of the rhomboid): the dead */ \
        /* lanes are masked off, so whole lines of the rows' tails are never fetched (-35 % lines)            */ \
        if (live0) { pre0 = src_[0];        pre4 = src_[o1_]; }                                                \
        if (live1) { pre1 = src_[8 * MX];   pre5 = src_[o1_ + 8 * MX]; }                                       \
        if (live2) { pre2 = src_[16 * MX];  pre6 = src_[o1_ + 16 * MX]; }                                      \
        if (live3) { pre3 = src_[24 * MX];  pre7 = src_[o1_ + 24 * MX]; }                                      \
    } while (0)
#define S2G_STAGE(xd_)                                                                                         \
    do {                                                                                                       \
        if (live0) { *reinterpret_cast<double2 *>((xd_) + 0 * XW) = pre0;  *reinterpret_cast<double2 *>((xd_) + 0 * XW + 2) = pre4; }  \
        if (live1) { *reinterpret_cast<double2 *>((xd_) + 4 * XW) = pre1;  *reinterpret_cast<double2 *>((xd_) + 4 * XW + 2) = pre5; }  \
        if (live2) { *reinterpret_cast<double2 *>((xd_) + 8 * XW) = pre2;  *reinterpret_cast<double2 *>((xd_) + 8 * XW + 2) = pre6; }  \
        if (live3) { *reinterpret_cast<double2 *>((xd_) + 12 * XW) = pre3; *reinterpret_cast<double2 *>((xd_) + 12 * XW + 2) = pre7; } \
    } while (0)
        // LDS destination of (m, n = rsub): packed row xoff(m) + parity block + n/2, XW doubles per row;
        // only m + n <= trunc+1 is ever read by the reference (legendre.f90:93: m <= nsh2(n))
        const int xrow0 = (xoff(pmc) + (rsub & 1) * 4 * (4 - (pmc >> 3)) + (rsub >> 1)) * XW;
        const bool live0 = pm < MX && pmc + rsub <= TRUNC + 1, live1 = pm < MX && pmc + rsub + 8 <= TRUNC + 1;
        const bool live2 = pm < MX && pmc + rsub + 16 <= TRUNC + 1, live3 = pm < MX && pmc + rsub + 24 <= TRUNC + 1;
        // MODE 1/2: thread (pj = tid/32, m = tid%32) owns rows n = 4*pj .. 4*pj+3 of column m and fetches rows
        // 4*pj-1 .. 4*pj+4 of the input spectra, so the three-point stencils in n are thread-local
        const int pj = tid >> 5;
        double2 in0[6], in1[6];
#define S2G_PREFETCH_D(tile_)                                                                                  \
    do {                                                                                                       \
        const int tc_ = min((int)(tile_), ntiles - 1);                                                         \
        const bool gr_ = IS_GRAD(tc_);   /* gradient tile: vorticity = the zero spectrum, divergence = psi */  \
        const double2 *s0_ = reinterpret_cast<const double2 *>(gr_ ? mixed.zero : spec) + (gr_ ? 0L : (long)tc_ * SPEC_C) + pmc; \
        const double2 *s1_ = reinterpret_cast<const double2 *>(gr_ ? mixed.psi : UVSPEC ? spec2 : spec) + (long)(gr_ ? tc_ - mixed.npairs : tc_) * SPEC_C + pmc; \
        UNROLL for (int r = 0; r < 6; ++r) {                                                                   \
            const int nc_ = min(max(4 * pj - 1 + r, 0), NX - 1);                                               \
            in0[r] = make_double2(0.0, 0.0);                                                                   \
            in1[r] = make_double2(0.0, 0.0);                                                                   \
            if (pmc + nc_ <= TRUNC + 2) { /* rows next to a live coefficient only (dead tails are never fetched) */ \
                in0[r] = s0_[nc_ * MX];                                                                        \
                if (UVSPEC) in1[r] = s1_[nc_ * MX];                                                            \
            }                                                                                                  \
        }                                                                                                      \
    } while (0)
        // times_i(c * z): the reference's full (0,1) complex multiply of the scaled value
#define S2G_TI(c_, z_) make_double2(((c_) * (z_).x) * 0.0 - (c_) * (z_).y, (c_) * (z_).x + ((c_) * (z_).y) * 0.0)
#define S2G_STAGE_D(xd_, tile_)                                                                                \
    do {                                                                                                       \
        const bool sg_ = IS_GRAD(min((int)(tile_), ntiles - 1));                                               \
        const double *tdx_ = sg_ ? p.gradx_e : p.uvdx, *tym_ = sg_ ? p.gradym : p.uvdym, *typ_ = sg_ ? p.gradyp : p.uvdyp; \
        UNROLL for (int i = 0; i < 4; ++i) {                                                                   \
            const int n_ = 4 * pj + i, e_ = n_ * MX + pmc;                                                     \
            const double2 lo0 = in0[i], mi0 = in0[i + 1], hi0 = in0[i + 2];                                    \
            double2 f0_, f1_;                                                                                  \
            if (UVSPEC) { /* uvspec: in0 = vor, in1 = div; f0 = U, f1 = V (operation order of uvspec_kernel) */   \
                const double2 lo1 = in1[i], mi1 = in1[i + 1], hi1 = in1[i + 2];                                \
                const double dx_ = tdx_[e_], ym_ = tym_[e_], yp_ = typ_[e_];                                   \
                const double2 zp_ = S2G_TI(dx_, mi0), zc_ = S2G_TI(dx_, mi1);                                  \
                if (n_ == 0) {                                                                                 \
                    f0_ = make_double2(zc_.x - yp_ * hi0.x, zc_.y - yp_ * hi0.y);                              \
                    f1_ = make_double2(zp_.x + yp_ * hi1.x, zp_.y + yp_ * hi1.y);                              \
                } else if (n_ == NX - 1) {                                                                     \
                    f0_ = make_double2(ym_ * lo0.x, ym_ * lo0.y);                                              \
                    f1_ = make_double2((-ym_) * lo1.x, (-ym_) * lo1.y);                                        \
                } else {                                                                                       \
                    f0_ = make_double2((ym_ * lo0.x - yp_ * hi0.x) + zc_.x, (ym_ * lo0.y - yp_ * hi0.y) + zc_.y); \
                    f1_ = make_double2(((-ym_) * lo1.x + yp_ * hi1.x) + zp_.x, ((-ym_) * lo1.y + yp_ * hi1.y) + zp_.y); \
                }                                                                                              \
            } else {        /* grad: f0 = i*gradx*psi, f1 = -gradym*psi(n-1) + gradyp*psi(n+1) (grad_kernel) */ \
                const double gx_ = p.gradx[pmc], ym_ = p.gradym[e_], yp_ = p.gradyp[e_];                       \
                f0_ = S2G_TI(gx_, mi0);                                                                        \
                if (n_ == 0) f1_ = make_double2(yp_ * hi0.x, yp_ * hi0.y);                                     \
                else if (n_ == NX - 1) f1_ = make_double2((-ym_) * lo0.x, (-ym_) * lo0.y);                     \
                else f1_ = make_double2((-ym_) * lo0.x + yp_ * hi0.x, (-ym_) * lo0.y + yp_ * hi0.y);           \
            }                                                                                                  \
            if (pm < MX && pmc + n_ <= TRUNC + 1) {                                                            \
                double *d_ = (xd_) + (xoff(pmc) + (i & 1) * 4 * (4 - (pmc >> 3)) + 2 * pj + (i >> 1)) * XW;    \
                *reinterpret_cast<double2 *>(d_) = f0_;                                                        \
                *reinterpret_cast<double2 *>(d_ + 2) = f1_;                                                    \
            }                                                                                                  \
        }                                                                                                      \
    } while (0)
        // MODE 3, plain tiles: the same moves as S2G_PREFETCH / S2G_STAGE with in0[k] = rows rsub + 8k of field 0 and
        // in1[k] of field 1 (sharing the registers of the derived tiles), read from mixed.spec_p
#define S2G_PREFETCH_A(tile_)                                                                                  \
    do {                                                                                                       \
        const int tp_ = (int)(tile_) - nder;                                                                   \
        const int f0_ = tp_ * BT, f1_ = min(f0_ + 1, mixed.nplain - 1);   /* (an absent second field reads the first again) */ \
        const double2 *src_ = reinterpret_cast<const double2 *>(s2g_plain_field(mixed, f0_)) + rsub * MX + pmc; \
        const double2 *sr1_ = reinterpret_cast<const double2 *>(s2g_plain_field(mixed, f1_)) + rsub * MX + pmc; \
        if (live0) { in0[0] = src_[0];        in1[0] = sr1_[0]; }                                              \
        if (live1) { in0[1] = src_[8 * MX];   in1[1] = sr1_[8 * MX]; }                                         \
        if (live2) { in0[2] = src_[16 * MX];  in1[2] = sr1_[16 * MX]; }                                        \
        if (live3) { in0[3] = src_[24 * MX];  in1[3] = sr1_[24 * MX]; }                                        \
    } while (0)
#define S2G_STAGE_A(xd_)                                                                                       \
    do {                                                                                                       \
        if (live0) { *reinterpret_cast<double2 *>((xd_) + 0 * XW) = in0[0];  *reinterpret_cast<double2 *>((xd_) + 0 * XW + 2) = in1[0]; }  \
        if (live1) { *reinterpret_cast<double2 *>((xd_) + 4 * XW) = in0[1];  *reinterpret_cast<double2 *>((xd_) + 4 * XW + 2) = in1[1]; }  \
        if (live2) { *reinterpret_cast<double2 *>((xd_) + 8 * XW) = in0[2];  *reinterpret_cast<double2 *>((xd_) + 8 * XW + 2) = in1[2]; }  \
        if (live3) { *reinterpret_cast<double2 *>((xd_) + 12 * XW) = in0[3]; *reinterpret_cast<double2 *>((xd_) + 12 * XW + 2) = in1[3]; } \
    } while (0)
#define S2G_FETCH_ANY(tile_)                                                                                   \
    do {                                                                                                       \
        if (MIXED) {                                                                                           \
            const int tm_ = min((int)(tile_), ntiles - 1);                                                     \
            if (tm_ < nder) S2G_PREFETCH_D(tm_); else S2G_PREFETCH_A(tm_);                                     \
        } else if (DERIVED) S2G_PREFETCH_D(tile_);                                                             \
        else S2G_PREFETCH(tile_);                                                                              \
    } while (0)
#define S2G_STAGE_ANY(img_, tile_)                                                                             \
    do {                                                                                                       \
        if (MIXED) {                                                                                           \
            if (min((int)(tile_), ntiles - 1) < nder) S2G_STAGE_D(img_, tile_); else S2G_STAGE_A((img_) + xrow0); \
        } else if (DERIVED) S2G_STAGE_D(img_, tile_);                                                          \
        else S2G_STAGE((img_) + xrow0);                                                                        \
    } while (0)
        S2G_FETCH_ANY(wg0);
        // small (latency-bound) launches: the resident operands are requested BEHIND the first tile's spectra -- loads return
        // in order, so the staging below waits for eight loads instead of thirty-eight, and the image (first needed by the
        // first matrix instruction, two barriers later) arrives under the zero fill and the staging: 12.9 -> 12.0 us at 91 fields
        if (!STREAM) S2G_LOAD_AREG();
#undef S2G_LOAD_AREG
        TL_MARK(0, 27);
        // (PART: one tile per workgroup -- only image 0 is ever used, and there is no next tile to prefetch or stage)
        for (int e = tid; e < (PART ? 1 : 2) * XS_TILE; e += NTHR) lds_x[e] = 0.0;   // padded / inactive rows stay 0 forever
        lds_barrier();                                            // (Z) zero fill complete before anything is staged
        TL_MARK(0, 26);
        S2G_STAGE_ANY(lds_x, wg0);                                // tile 0 -> image 0
        TL_MARK(0, 28);
        if (!PART) S2G_FETCH_ANY(wg0 + wgs);
        lds_barrier();                                            // (A) image 0 complete

        const int blk = (lane >> 2) & 3, col = lane & 3, drow = lane >> 4;
        for (int k = 0; k <= ksteps; ++k) {
            const int titer = SPDY_TRACE_STEP(k, ksteps);
            (void)titer;
            PHASE_MARK(0, 0);
            if (k < 25) TL_MARK(0, 1 + k);
            if (k < ksteps) {
                // ---- Legendre synthesis (legendre.f90:74-111) on 4x4x4 blocks:
                //   type 1 (per parity): blocks = latitude groups 0..3 (lat = lane & 15 for A, = 4*blk + (lane>>4) for D)
                //   type 2: blocks 0,1 = latitude groups 4,5 of the even-n sum, blocks 2,3 = the same of the odd-n sum
                const double *xs = lds_x + (k & 1) * XS_TILE;
                double *ft = lds_f + (k & 1) * F_TILE;
                int ai = 0;
                UNROLL for (int s = 0; s < 8; ++s) {
                    const int m = mslot(s, w), mc = min(m, MX - 1);
                    const int nk = 4 - (s >> 1);
                    const double *bsrc = xs + (xoff(mc) + (lane >> 4)) * XW + col;
                    double acc1e = 0.0, acc1o = 0.0, acc2 = 0.0;
                    UNROLL for (int ks = 0; ks < 4; ++ks) {
                        if (ks < nk) {
                            const double be = bsrc[(4 * ks) * XW], bo = bsrc[(4 * nk + 4 * ks) * XW];
                            if (PART) {                          // the part's eight latitudes, both parities packed
                                acc2 = MFMA4(areg[ai], (blk >> 1) ? bo : be, acc2);
                                ai += 1;
                            } else {
                                acc1e = MFMA4(areg[ai], be, acc1e);
                                acc1o = MFMA4(areg[ai + 1], bo, acc1o);
                                acc2 = MFMA4(areg[ai + 2], (blk >> 1) ? bo : be, acc2);
                                ai += 3;
                            }
                        }
                    }
                    // rows: south = lat, north = 47 - lat; out(north) = even + odd, out(south) = even - odd
                    const double other = __shfl_xor(acc2, 8);    // lane ^ 8 flips the parity half of type 2
                    const bool real = m < MX;                    // the single unused slot writes into a spare cell
                    if (PART) {
                        double *fb = ft + (col >> 1) * (16 * F_ROW) + 2 * mc + (col & 1);
                        const int q = 4 * (blk & 1) + drow;      // latitude 8 part + q
                        *(real ? fb + (blk < 2 ? 15 - q : q) * F_ROW : sink) = blk < 2 ? acc2 + other : other - acc2;
                    } else {
                        double *fb = ft + (col >> 1) * (IL * F_ROW) + 2 * mc + (col & 1);
                        const int lat1 = 4 * blk + drow, lat2 = 16 + 4 * (blk & 1) + drow;
                        *(real ? fb + (IL - 1 - lat1) * F_ROW : sink) = acc1e + acc1o;
                        *(real ? fb + lat1 * F_ROW : sink) = acc1e - acc1o;
                        *(real ? fb + (blk < 2 ? (IL - 1 - lat2) : lat2) * F_ROW : sink) = blk < 2 ? acc2 + other : other - acc2;
                    }
                }
                PHASE_MARK(0, 1);
                // stage tile k+1 (prefetched a step ago) into the other image, prefetch tile k+2
                if (!PART) {
                    S2G_STAGE_ANY(lds_x + ((k + 1) & 1) * XS_TILE, wg0 + (k + 1) * wgs);
                    S2G_FETCH_ANY(wg0 + (k + 2) * wgs);
                }
            }
            PHASE_MARK(0, 2);
            lds_barrier();
        }
        TL_MARK(0, 31);
#undef S2G_PREFETCH
#undef S2G_STAGE
#undef S2G_PREFETCH_D
#undef S2G_STAGE_D
#undef S2G_TI
#undef S2G_FETCH_ANY
#undef S2G_STAGE_ANY
#undef S2G_PREFETCH_A
#undef S2G_STAGE_A
    } else {
        // =================================================================== FFT waves
        const int fw = w - NLW;                                   // 0..2: rows 32*fw .. 32*fw+31 of the tile
        // the FFT waves are the longer role of a step here and share three of the four SIMDs with a Legendre wave each: with a
        // raised priority their instructions win the arbitration on those SIMDs (57.5 -> 55 us at B = 6144; the same in the
        // direct kernel, whose roles are balanced, costs 3 us, and in the derived modes, where the Legendre waves also apply the
        // uvspec / grad stencils while staging, 11 us: uvspec->grid 63 -> 75 us)
        if (MODE == 0) __builtin_amdgcn_s_setprio(2);
        for (int e = tid; e < (PART ? 1 : 2) * XS_TILE; e += NTHR) lds_x[e] = 0.0;   // this wave's share of the zero fill
        lds_barrier();                                            // (Z)
        lds_barrier();                                            // (A)
        for (int k = 0; k <= ksteps; ++k) {
            const int titer = SPDY_TRACE_STEP(k, ksteps);
            (void)titer;
            PHASE_MARK(0, 3);
            if (k < 25) TL_MARK(0, 1 + k);
            if (k >= 1 && (!PART || fw == 0)) {
                const int tile = wg0 + (k - 1) * wgs;
                // ---- 32 row FFTs (fourier.f90:23-53), wave-local: lanes l and l+32 own the two 48-point
                // columns of row 32*fw + l.  Opaque per-step offset: keeps the constant loads in the loop.
                int coff = 0, h = lane >> 5;
                asm volatile("" : "+s"(coff), "+v"(h));
                const FftConstants &c = *reinterpret_cast<const FftConstants *>(reinterpret_cast<const char *>(&c_fft96) + coff);
                const int rowidx = 32 * fw + (lane & 31);
                // (PART: local rows, see the kernel's head -- field = row / 16, grid row = 8 part + l | 32 - 8 part + l)
                const int fld = PART ? rowidx >> 4 : rowidx / IL;
                const int j = PART ? ((rowidx & 15) < 8 ? 8 * part + (rowidx & 15) : 32 - 8 * part + (rowidx & 15)) : rowidx - fld * IL;
                double *ft = lds_f + ((k - 1) & 1) * F_TILE;
                double *rowp = ft + rowidx * F_ROW;
                double x[48], y[48];
                {
                    // ido=48 radix-2 stage (fftpack radb2), column h of this lane; inputs beyond 2*mx-2 are zero
                    // coefficient i of the row sits at rowp[i + 1] (i >= 1): the pairs (pp, pp + 1) and (48 + q, 48 + q + 1) start at
                    // even slots, i.e. on 16-byte boundaries (a row is 31 x 16 bytes) -- one ds_read_b128 each, and with rows
                    // 124 dwords apart the four 16-lane groups of a b128 read fall on 16 different slots of the bank row
                    // (the 8-byte reads were two instructions per pair and 2-way conflicted between rows r and r + 16)
                    auto fv = [&](int i) -> double { return i == 0 ? rowp[0] : (i <= 2 * MX - 2 ? rowp[i + 1] : 0.0); };
                    auto fv2 = [&](int i) -> double2 { return *reinterpret_cast<const double2 *>(rowp + i + 1); };   // (fv(i), fv(i+1)), i odd
                    static_assert((2 * MX - 2) % 2 == 0 && F_ROW % 2 == 0, "pairs of Fourier slots are 16-byte aligned");
                    x[0] = fv(0);                                          // fv(95) == 0 for both columns
                    if (h == 0) {
                        UNROLL for (int pp = 1; pp < 47; pp += 2) {
                            const int q = 46 - pp;
                            const double2 a = fv2(pp);
                            if (48 + q + 1 <= 2 * MX - 2) {
                                const double2 b = fv2(48 + q);
                                x[pp] = a.x + b.x;
                                x[pp + 1] = a.y - b.y;
                            } else {
                                x[pp] = a.x;
                                x[pp + 1] = a.y;
                            }
                        }
                        x[47] = fv(47) + fv(47);
                    } else {
                        UNROLL for (int pp = 1; pp < 47; pp += 2) {
                            const int q = 46 - pp;
                            const double2 a = fv2(pp);
                            double tr2 = a.x, ti2 = a.y;
                            if (48 + q + 1 <= 2 * MX - 2) {
                                const double2 b = fv2(48 + q);
                                tr2 = a.x - b.x;
                                ti2 = a.y + b.y;
                            }
                            x[pp] = c.first[pp - 1] * tr2 - c.first[pp] * ti2;
                            x[pp + 1] = c.first[pp - 1] * ti2 + c.first[pp] * tr2;
                        }
                        x[47] = -(fv(48) + fv(48));
                    }
                }
                sub48_backward_c(c, x, y);
                PHASE_MARK(0, 4);
                const bool der = IS_DER(tile);
                const int tp = MIXED ? tile - nder : tile;                   // index among the plain tiles
                const int gfld = tp * BT + fld;
                const bool dgr = IS_GRAD(tile);
                int kc = der ? (dgr ? mixed.kcos_grad : kcos_all) : 1;
                if (!der && !MIXED && gfld < nb) kc = d_kcos ? d_kcos[gfld] : kcos_all;
                if (!der && MIXED && gfld < mixed.nplain) kc = mixed.kcos_p ? mixed.kcos_p[gfld] : mixed.kcos_all_p;
                if (__any(kc != 1)) {
                    const double sc = kc == 1 ? 1.0 : p.cosgr[j];
                    UNROLL for (int t = 0; t < 48; ++t) y[t] *= sc;
                }
                // copy-out through this row's own (now dead) 62-double slot, half a row at a time:
                // permlane32_swap pairs the columns so each lane holds 16-byte pieces of the row
                UNROLL for (int half = 0; half < 2; ++half) {
                    UNROLL for (int kk2 = 0; kk2 < 12; ++kk2) {
                        const int kk = 12 * half + kk2;
                        const unsigned long long a64 = __double_as_longlong(y[2 * kk]), b64 = __double_as_longlong(y[2 * kk + 1]);
                        const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)a64, (unsigned)b64, false, false);
                        const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(a64 >> 32), (unsigned)(b64 >> 32), false, false);
                        double2 piece;
                        piece.x = __longlong_as_double(((unsigned long long)hi[0] << 32) | lo[0]);
                        piece.y = __longlong_as_double(((unsigned long long)hi[1] << 32) | lo[1]);
                        *reinterpret_cast<double2 *>(rowp + 2 * (2 * kk2 + h)) = piece;
                    }
                    // read back row-contiguous: lane (rl, pl) takes pieces pl + 8c of rows rl + 8a -> every
                    // store instruction writes 8 full 128-byte lines; all offsets are base + constant
                    {
                        // line group g = lane/8 takes row rl + 2a of the wave's 32 in round a, rl = {0,16,8,24}[g%4] + g/4: ds_read_b128
                        // is served in the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... and a row is 124 dwords (= -4
                        // mod 64), so the 16-byte slot of (row, piece) is (piece - row) mod 16; this row order makes the four half
                        // lines of every group land on four different quarters of the 256-byte bank row (rows g + 8a: 2-3-way)
                        const int g8 = lane >> 3, pl = lane & 7;
                        const int rl = ((0x18081000 >> (8 * (g8 & 3))) & 0xff) + (g8 >> 2);
                        const double *cb = ft + (32 * fw + rl) * F_ROW + 2 * pl;
                        // tile row of local row rl (the rows rl + 2a of one lane stay inside one group of eight)
                        const int trow = PART ? (rl >> 4) * IL + (((rl >> 3) & 1) ? 40 - 8 * part : 8 * part) + (rl & 7) : 32 * fw + rl;
                        const long grow = (long)tp * TROWS + trow;
                        double *gb = (MIXED ? mixed.grid_p : grid) + grow * IX + 48 * half + 2 * pl;
                        const long glimit = (long)(MIXED ? mixed.nplain : nb) * IL;
                        // MODE 1/2: rows 0..47 -> grid[tile], rows 48..95 -> grid2[tile] (row group a of this wave: uniform)
                        const long dt_ = dgr ? tile - mixed.npairs : tile;          // (gradient tiles write gx, gy)
                        double *gb0 = (dgr ? mixed.gx : grid) + (dt_ * IL + trow) * IX + 48 * half + 2 * pl;
                        double *gb1 = (dgr ? mixed.gy : grid2) + (dt_ * IL + trow - IL) * IX + 48 * half + 2 * pl;
                        UNROLL for (int a = 0; a < 4; ++a) {
                            UNROLL for (int cc = 0; cc < 3; ++cc) {
                                const double2 v = *reinterpret_cast<const double2 *>(cb + a * 2 * F_ROW + 16 * cc);
                                if (der)
                                    grid_store2<STREAM>(reinterpret_cast<double2 *>((trow + 2 * a >= IL ? gb1 : gb0) + a * 2 * IX + 16 * cc), v);
                                else if (grow + 2 * a < glimit)
                                    grid_store2<STREAM>(reinterpret_cast<double2 *>(gb + a * 2 * IX + 16 * cc), v);
                            }
                        }
                    }
                }
                PHASE_MARK(0, 5);
            }
            lds_barrier();
        }
        TL_MARK(0, 31);
    }
}
#undef IS_DER
#undef IS_GRAD

// ------------------------------------------------------------------------------------------
// grid_to_spec, fused (spectral.f90:112-122).  spec[nb][32][31] complex <- grid[nb][48][96]
// gscale: optional per-latitude factor applied on load (vdspec: cosgr / cosgr2)
//   step k: FFT waves stage + transform tile k into row buffer k%2 and prefetch tile k+1; Legendre waves
//           contract row buffer (k-1)%2 (tile k-1), leaving the spectra in place of the columns they consumed,
//           and write the spectra of tile k-2 (picked up from row buffer k%2 before barrier B1 hands that buffer
//           to the FFT waves) as contiguous 16-byte-per-lane stores.  Two barriers per step.
// ------------------------------------------------------------------------------------------
struct G2sMixed { const double *grid_p; double *spec_p; int npairs, nplain; };   // MODE 3 only (see the kernel)
// MODE 0: plain.  MODE 1: every grid row is multiplied by gscale[latitude] on the way in.
// MODE 2 = vdspec (spectral.f90:198-227) in one pass: a tile is the pair (ug[i], vg[i]) = (grid, grid2), scaled as in
//          MODE 1; both spectra stay in LDS and the copy-out applies vds (spectral.f90:146-171) to them, writing
//          vorticity to `spec` and divergence to `spec2`.  nb counts pairs.
//          NSPLIT = 3 (small batches: at most a third as many tiles as CUs): three workgroups per tile; all three run the
//          tile's row FFTs, each contracts and stores a third of the zonal wavenumbers -- slots {0,1}, {2,3}, {4..7} of every
//          Legendre wave (m' 0-7, 8-15, 16-30): 24 of the 72 matrix instructions each, and a 128-byte line of spectra (8
//          wavenumbers) has ONE writer wherever the 31-coefficient rows allow.  The same instructions on the same values for
//          every (m', n): bit-identical to the whole-tile walk (SPDY_T30_NOSPLIT selects that).
template <int MODE, bool STREAM, int NSPLIT = 1>
__global__ __launch_bounds__(t30::NTHR, 2) void g2s_fused_t30_kernel(DevPlan p, int nb, const double *__restrict__ grid,
                                                                    const double *__restrict__ grid2,
                                                                    const double *__restrict__ gscale,
                                                                    double *__restrict__ spec, double *__restrict__ spec2,
                                                                    G2sMixed mixed)
{
    using namespace t30;
    constexpr bool SCALED = MODE != 0, PAIR = MODE == 2, MIXED = MODE == 3;
    // MODE 3 = one launch for a model step's whole direct batch: tiles [0, npairs) are (u, v) pairs handled as in
    // MODE 2, the tiles after them are plain 2-field tiles of mixed.grid_p -> mixed.spec_p (nplain fields, unscaled)
#define IS_PAIR(t_) (PAIR || (MIXED && (int)(t_) < mixed.npairs))
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    TL_MARK(1, 0);
    const int ntiles = PAIR ? nb : MIXED ? mixed.npairs + (mixed.nplain + BT - 1) / BT : (nb + BT - 1) / BT;
    constexpr bool SPLIT = NSPLIT > 1;
    // first tile, tile stride and (SPLIT) which third of the zonal wavenumbers this workgroup contracts
    const int wg0 = SPLIT ? (int)blockIdx.x / NSPLIT : (int)blockIdx.x, wgs = SPLIT ? (int)gridDim.x / NSPLIT : (int)gridDim.x;
    const int qpart = SPLIT ? (int)blockIdx.x % NSPLIT : 0;
#define G2S_SLOT_PART(s_) ((s_) < 2 ? 0 : (s_) < 4 ? 1 : 2)           /* slots {0,1}, {2,3}, {4..7}: 24 matrix instructions each */
    const int ksteps = (wg0 < ntiles) ? (ntiles - 1 - wg0) / wgs + 1 : 0;
    // twiddles of the last (ido = 48) FFT stage where a lane can pick its own pair with one LDS read:
    // butterfly pb = 4*it + 1 + 2*h uses (first[pb-1], first[pb]); pb = 47 does not exist (entry unused)
    double *lds_tw = lds + 2 * G_TILE;                              // every FFT wave writes (and then reads) the same 48 values

    if (w >= NLW) {
        // =================================================================== FFT waves
        // wave fw owns rows 32*fw..32*fw+31 of the tile: lane (rl = lane/16, l16 = lane%16) moves pieces
        // l16 + 16q (q < 3) of rows rl + 4a (a < 8): 24 16-byte pieces, all offsets base + constant.
        const int fw = w - NLW, l16 = lane & 15, rl = lane >> 4;
        constexpr int NPRE = 24, NEARLY = SPDY_G2S_NEARLY;          // pieces per lane; how many are issued before the FFT
        double2 pre[NPRE];
        // row groups [A0, A1) of the tile (3 pieces per row group); a macro with compile-time bounds, not a
        // lambda: the by-reference capture keeps `pre` in scratch memory
#define G2S_EXP_TILE(t_) (t_)
#define G2S_PREFETCH(tile_, A0, A1)                                                                        \
    do {                                                                                                   \
        const int tc_ = min((int)(tile_), ntiles - 1);                                                     \
        if (IS_PAIR(tc_)) { /* rows 0..47 = ug[pair], rows 48..95 = vg[pair]; row group a >= 4 of wave 1 crosses over */ \
            const double2 *s0_ = reinterpret_cast<const double2 *>(grid) + (long)tc_ * (IL * IX / 2) + l16; \
            const double2 *s1_ = reinterpret_cast<const double2 *>(grid2) + (long)tc_ * (IL * IX / 2) + l16; \
            UNROLL for (int a = (A0); a < (A1); ++a) {                                                     \
                const bool second_ = 32 * fw + 4 * a >= IL;                                                \
                const int row_ = 32 * fw + rl + 4 * a - (second_ ? IL : 0);                                \
                const double2 *src_ = second_ ? s1_ : s0_;                                                 \
                UNROLL for (int q = 0; q < 3; ++q) pre[3 * a + q] = grid_load2<STREAM>(&src_[row_ * 48 + 16 * q]); \
            }                                                                                              \
        } else {                                                                                           \
            const int tq_ = MIXED ? tc_ - mixed.npairs : tc_; /* index among the plain tiles */           \
            const int tp_ = G2S_EXP_TILE(tq_);                                                             \
            const int nrow_ = min(BT, (MIXED ? mixed.nplain : nb) - tq_ * BT) * IL; /* valid rows in this tile */ \
            const double2 *src_ = reinterpret_cast<const double2 *>(MIXED ? mixed.grid_p : grid) + (long)tp_ * (TROWS * IX / 2) + l16; \
            UNROLL for (int a = (A0); a < (A1); ++a) {                                                     \
                const int row_ = 32 * fw + rl + 4 * a, rowc_ = row_ < nrow_ ? row_ : 0;                    \
                UNROLL for (int q = 0; q < 3; ++q) pre[3 * a + q] = grid_load2<STREAM>(&src_[rowc_ * 48 + 16 * q]); \
            }                                                                                              \
        }                                                                                                  \
    } while (0)
        TL_MARK(1, 26);
        G2S_PREFETCH(wg0, 0, 8);
        TL_MARK(1, 27);
        {   // The twiddle pairs of the ido = 48 stage: entry e of the table is first[pb - 1 + (e & 1)], pb = 4 (e / 4) + 1 +
            // 2 ((e / 2) & 1).  Each FFT wave fetches all 48 behind its own first-tile loads and stores them itself -- the
            // three waves write the same values to the same cells, and a wave reads them back behind its own write -- so no
            // wave waits at a start-up barrier for another wave's constant-memory round trip (it cost every launch the ~4 k
            // ticks between its last row request and the first step).
            const int e = min(lane, G_TW - 1), pb = 4 * (e >> 2) + 1 + 2 * ((e >> 1) & 1);
            const double twv = pb <= 45 ? c_fft96.first[pb - 1 + (e & 1)] : 0.0;
            if (lane < G_TW) lds_tw[lane] = twv;
        }
        for (int k = 0; k <= ksteps + 1; ++k) {
            const int titer = SPDY_TRACE_STEP(k, ksteps);
            (void)titer;
            // MODE 2/3 (two source arrays, row groups that cross from one to the other): per-step opaque lane indices, so the
            // prefetch addresses are recomputed each step instead of being hoisted into ~15 registers that spill -- a
            // scratch reload inside the FFT waits (vmcnt) for the whole HBM prefetch
            int lane_o = lane;
            if (MODE != 0) asm volatile("" : "+v"(lane_o));
            const int l16 = lane_o & 15, rl = lane_o >> 4;
            PHASE_MARK(1, 0);
            if (k < 25) TL_MARK(1, 1 + k);
            lds_barrier();                                          // B1: the spectra of tile k-2 have left row buffer k%2
            if (k < ksteps) {
                double *buf = lds + (k & 1) * G_TILE;
                // ---- own grid rows into their LDS slots (stride 99)
                {
                    double *gdst = buf + (32 * fw + rl) * G_ROW + 2 * l16;
                    UNROLL for (int a = 0; a < 8; ++a) {
                        double sc = 1.0;
                        if (SCALED) sc = (!MIXED || IS_PAIR(wg0 + k * wgs)) ? gscale[(32 * fw + rl + 4 * a) % IL] : 1.0;
                        UNROLL for (int q = 0; q < 3; ++q) {
                            double2 v = pre[3 * a + q];
                            if (SCALED) { v.x *= sc; v.y *= sc; }
                            double *d = gdst + 4 * a * G_ROW + 32 * q;
                            d[0] = v.x;
                            d[1] = v.y;
                        }
                    }
                }
                G2S_PREFETCH(wg0 + (k + 1) * wgs, 0, NEARLY);   // in flight during the FFT below
                PHASE_MARK(1, 1);
                // ---- 32 row FFTs (fourier.f90:56-82), wave-local: lanes l and l+32 own the two decimated
                // 48-point sub-transforms of row 32*fw + l, then share its ido=48 stage
                int coff = 0;                                 // opaque per step: keeps the constant loads in the loop
                asm volatile("" : "+s"(coff));                // (an offset, not the pointer: scalar loads survive)
                const FftConstants &c = *reinterpret_cast<const FftConstants *>(reinterpret_cast<const char *>(&c_fft96) + coff);
                const int h = lane >> 5;
                double *rowp = buf + (32 * fw + (lane & 31)) * G_ROW;
                double x[48], y[48];
                UNROLL for (int t = 0; t < 48; ++t) x[t] = rowp[2 * t + h];
                sub48_forward_c(c, x, y);
                PHASE_MARK(1, 2);
                // ido = 48 radix-2 stage (fftpack radf2) in registers.  Lane l holds z0[] (column 0), lane l+32
                // holds z1[]; one permlane32_swap of (y[p], y[p+2]) leaves (z0[p], z1[p]) in the low lane and
                // (z0[p+2], z1[p+2]) in the high lane, so the low lane does butterfly p and the high lane
                // butterfly p+2 completely, and only results are written: Fourier coefficient slot k of this
                // row (k <= 2*mx-2 = 60 are needed; slots 61.. are never read).
                auto swap2 = [&](double a, double b, double &o0, double &o1) {
                    const unsigned long long a64 = __double_as_longlong(a), b64 = __double_as_longlong(b);
                    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)a64, (unsigned)b64, false, false);
                    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(a64 >> 32), (unsigned)(b64 >> 32), false, false);
                    o0 = __longlong_as_double(((unsigned long long)hi[0] << 32) | lo[0]);
                    o1 = __longlong_as_double(((unsigned long long)hi[1] << 32) | lo[1]);
                };
                {   // i = 0 / i = 47 specials: low lane gets (z0[0], z1[0]), high lane (z0[47], z1[47])
                    double u0, u1;
                    swap2(y[0], y[47], u0, u1);
                    if (h == 0) rowp[0] = u0 + u1;                               // ch(0,0)
                    else { rowp[47] = u0; rowp[48] = -u1; }                      // ch(47,0), ch(0,1)
                }
                double *zlo = rowp + 2 * h, *zhi = rowp - 2 * h;                 // own slots p+2h ; mirrored 94-p-2h
                // all twelve twiddle pairs of this lane's butterflies in one go (scalar loads inside the loop would
                // put a load latency + lgkmcnt(0) drain of the LDS writes in front of every butterfly)
                double2 tw[12];
                UNROLL for (int it = 0; it < 12; ++it) tw[it] = *reinterpret_cast<const double2 *>(lds_tw + 4 * it + 2 * h);
                UNROLL for (int pp = 1; pp <= 45; pp += 4) {
                    double a0r, a1r, a0i, a1i;                                   // this lane's butterfly pb = pp + 2h
                    swap2(y[pp], y[pp + 2 <= 46 ? pp + 2 : pp], a0r, a1r);
                    swap2(y[pp + 1], y[pp + 3 <= 47 ? pp + 3 : pp + 1], a0i, a1i);
                    const bool mine = pp + 2 <= 45 || h == 0;                    // last group: only butterfly 45 exists
                    const double wr = tw[pp >> 2].x, wi = tw[pp >> 2].y;
                    const double tr2 = wr * a1r + wi * a1i, ti2 = wr * a1i - wi * a1r;
                    if (mine) {
                        zlo[pp] = a0r + tr2;                                     // ch(pb,0)
                        zlo[pp + 1] = a0i + ti2;                                 // ch(pb+1,0)
                        if (pp + 2 * h >= 35) {                                  // mirrored pair q = 46-pb <= 11 -> slots 48+q(+1) <= 60
                            zhi[94 - pp] = a0r - tr2;                            // ch(q,1)
                            zhi[95 - pp] = ti2 - a0i;                            // ch(q+1,1)
                        }
                    }
                }
                G2S_PREFETCH(wg0 + (k + 1) * wgs, NEARLY, 8);   // the rest, once the FFT registers are dead
                PHASE_MARK(1, 3);
            }
            lds_barrier();
        }
        TL_MARK(1, 31);
#undef G2S_PREFETCH
    } else {
        // =================================================================== Legendre waves
        // resident MFMA A operands: slots 0..3 (m' < 16): 2 parities x 6 latitude k-steps; slots 4..7: 6 packed
        double areg[SPLIT ? 24 : 72];
        {   // 16-byte loads from the register image (two fragments each); first used a whole step after the first rows.
            // SPLIT: only this workgroup's slots -- twelve consecutive entries from q = 0 (slots 0, 1), 12 (slots 2, 3) or 24 (slots 4..7)
            const double2 *img = reinterpret_cast<const double2 *>(p.img_g2s) + (long)w * 36 * 64 + lane;
            if (SPLIT) {
                UNROLL for (int q = 0; q < 12; ++q) {
                    const double2 v = img[(12 * qpart + q) * 64];
                    areg[2 * q] = v.x;
                    areg[2 * q + 1] = v.y;
                }
            } else {
                UNROLL for (int q = 0; q < 36; ++q) {
                    const double2 v = img[q * 64];
                    areg[2 * q] = v.x;
                    areg[2 * q + 1] = v.y;
                }
            }
        }
        const double fscale = c_fft96.scale;
        const int blk = (lane >> 2) & 3, col = lane & 3, drow = lane >> 4, part = col & 1;
        // Copy-out map.  The contraction leaves its results in LDS, in place of the Fourier columns it consumed
        // (coefficient (field f, n, m', re/im) at row f*48 + n, column 2m'-1+part; (m'=0, re) at column 0), and the
        // tile's 1984 complex coefficients -- one contiguous 31,744-byte range of `spec` -- leave a step later as
        // full 16-byte-per-lane stores: element c = 256*i + tid.  (8-byte stores straight from the MFMA layout
        // reach 16 contiguous bytes per (n, m') only; the memory system runs those at about a third of the rate.)
        int co_off[8];
        unsigned co_m0 = 0, co_f1 = 0;                             // bit i: element i has m' = 0 / belongs to field 1
        unsigned co_mine = 0xffu;                                  // (SPLIT) bit i: element i's zonal wavenumber is in this workgroup's quarter
#define G2S_COMAP(tid_)                                                                                    \
    do {                                                                                                   \
        co_m0 = 0; co_f1 = 0;                                                                              \
        if (SPLIT) co_mine = 0;                                                                            \
        UNROLL for (int i = 0; i < 8; ++i) {                                                               \
            const int c = min(256 * i + (tid_), BT * SPEC_C - 1);                                          \
            const int f = c / SPEC_C, r = c - f * SPEC_C, n = r / MX, m = r - n * MX;                      \
            co_off[i] = (f * IL + n) * G_ROW + (m == 0 ? 0 : 2 * m - 1);                                   \
            co_m0 |= (m == 0 ? 1u : 0u) << i;                                                              \
            co_f1 |= (unsigned)f << i;                                                                     \
            if (SPLIT) co_mine |= (G2S_SLOT_PART(m >> 2) == qpart ? 1u : 0u) << i;                         \
        }                                                                                                  \
    } while (0)
        if (!MIXED) G2S_COMAP(tid);
        double2 co[8];
        // vds factors gradx(m'), vddym(m',n), vddyp(m',n) of this lane's 4 copy-out positions.  They are the same every step,
        // but 24 registers held across the contraction spill; so they are re-read (L2) at the END of every step, after the
        // contraction's registers have died, and consumed at the top of the next one -- the load latency sits behind the
        // step barrier instead of in front of B1, where the FFT waves wait for this copy-out to leave the row buffer
        // (MODE 2; the mixed-batch kernel, out of registers, reads them where it uses them).
        double vgx[4] = {0.0, 0.0, 0.0, 0.0}, vym[4] = {0.0, 0.0, 0.0, 0.0}, vyp[4] = {0.0, 0.0, 0.0, 0.0};
#define G2S_VDS_FACTORS()                                                                                  \
    do {                                                                                                   \
        int tf_ = tid;                                                                                     \
        asm volatile("" : "+v"(tf_));                                                                      \
        const int m = min(tf_ & 31, MX - 1), pj = tf_ >> 5;   /* this lane's column and block of four rows */  \
        UNROLL for (int i = 0; i < 4; ++i) {                                                               \
            const int c = (4 * pj + i) * MX + m;                                                           \
            vgx[i] = p.gradx[m];                                                                           \
            vym[i] = p.vddym[c];                                                                           \
            vyp[i] = p.vddyp[c];                                                                           \
        }                                                                                                  \
    } while (0)
        if (PAIR) G2S_VDS_FACTORS();
        for (int k = 0; k <= ksteps + 1; ++k) {
            const int titer = SPDY_TRACE_STEP(k, ksteps);
            (void)titer;
            if (MIXED) {                                            // the mixed-batch kernel carries both copy-out paths: recompute
                int tid_o = tid;                                    // the map per step (a few dozen integer ops) rather than hold it
                asm volatile("" : "+v"(tid_o));                     // in 10 registers that spill
                G2S_COMAP(tid_o);
            }
            PHASE_MARK(1, 4);
            if (k < 25) TL_MARK(1, 1 + k);
            const long ctile = wg0 + (k - 2) * wgs;                                              // the tile that leaves now
            const bool cpair = IS_PAIR(ctile);
            if (k >= 2 && !cpair) {                                 // spectra of tile k-2 (contracted a step ago) -> registers
                const double *rb = lds + (k & 1) * G_TILE;
                UNROLL for (int i = 0; i < 8; ++i) {
                    co[i].x = rb[co_off[i]];
                    co[i].y = rb[co_off[i] + 1];
                }
            }
            if (k >= 2 && cpair) {
                // vds on the pair's spectra U (rows 0..31) and V (rows 48..79) of row buffer k%2: co[i] = vorticity,
                // co[4+i] = divergence at position i.  Operation order as in vds_kernel (spdy_kernels.hip).
                const double *rb = lds + (k & 1) * G_TILE;
                int tv = tid;
                asm volatile("" : "+v"(tv));
                if (MIXED) G2S_VDS_FACTORS();                       // (the mixed-batch kernel has no registers to carry them: read here)
                // Lane (pj = tid/32, m = tid%32) owns rows n = 4 pj .. 4 pj + 3 of column m and reads rows 4 pj - 1 .. 4 pj + 4 of both
                // spectra once (24 LDS reads for four positions; one position per lane and step needed 12 each)
                const int m = min(tv & 31, MX - 1), pj = tv >> 5, cc = m == 0 ? 0 : 2 * m - 1;
                double2 uc[6], vc[6];
                UNROLL for (int r = 0; r < 6; ++r) {
                    const int nn = min(max(4 * pj - 1 + r, 0), NX - 1);
                    const double *qu = rb + nn * G_ROW + cc, *qv = qu + IL * G_ROW;          // coefficient (n = nn, m'); Im(m'=0) is 0
                    uc[r] = make_double2(qu[0], m == 0 ? 0.0 : qu[1]);
                    vc[r] = make_double2(qv[0], m == 0 ? 0.0 : qv[1]);
                }
                UNROLL for (int i = 0; i < 4; ++i) {
                    const int n = 4 * pj + i;
                    const double2 u0 = uc[i + 1], v0 = vc[i + 1], ulo = uc[i], vlo = vc[i], uhi = uc[i + 2], vhi = vc[i + 2];
                    // times_i(gradx * z) = (re*0 - im, re + im*0) of the scaled value
                    const double2 gu = make_double2(vgx[i] * u0.x, vgx[i] * u0.y), gv = make_double2(vgx[i] * v0.x, vgx[i] * v0.y);
                    const double2 zp = make_double2(gu.x * 0.0 - gu.y, gu.x + gu.y * 0.0), zc = make_double2(gv.x * 0.0 - gv.y, gv.x + gv.y * 0.0);
                    double2 vo, dv;
                    if (n == 0) {
                        vo = make_double2(zc.x - vyp[i] * uhi.x, zc.y - vyp[i] * uhi.y);
                        dv = make_double2(zp.x + vyp[i] * vhi.x, zp.y + vyp[i] * vhi.y);
                    } else if (n == NX - 1) {
                        vo = make_double2(vym[i] * ulo.x, vym[i] * ulo.y);
                        dv = make_double2((-vym[i]) * vlo.x, (-vym[i]) * vlo.y);
                    } else {
                        vo = make_double2((vym[i] * ulo.x - vyp[i] * uhi.x) + zc.x, (vym[i] * ulo.y - vyp[i] * uhi.y) + zc.y);
                        dv = make_double2(((-vym[i]) * vlo.x + vyp[i] * vhi.x) + zp.x, ((-vym[i]) * vlo.y + vyp[i] * vhi.y) + zp.y);
                    }
                    co[i] = vo;
                    co[4 + i] = dv;
                }
            }
            lds_barrier();                                          // B1: row buffer k%2 may be refilled with grid rows
            PHASE_MARK(1, 6);
            const long cplain = MIXED ? ctile - mixed.npairs : ctile;                             // its index among the plain tiles
            const int pcol = tid & 31, pbase = 4 * (tid >> 5) * MX + min(pcol, MX - 1);           // pairs: (row block, column) of this lane
            double2 *cdst = cpair ? reinterpret_cast<double2 *>(spec) + ctile * SPEC_C + pbase
                                  : reinterpret_cast<double2 *>(MIXED ? mixed.spec_p : spec) + cplain * (BT * SPEC_C) + tid;
            double2 *cdst2 = reinterpret_cast<double2 *>(spec2) + ctile * SPEC_C + pbase;         // pairs: divergence
            const int cfields = k >= 2 ? (MIXED ? mixed.nplain : nb) - (int)cplain * BT : 0;      // plain: fields of that tile that exist
#define G2S_COPYOUT(i_)                                                                                    \
    do {                                                                                                   \
        if (cpair) {                                                                                       \
            if (pcol < MX && (!SPLIT || G2S_SLOT_PART(pcol >> 2) == qpart))                                \
                G2S_SPEC_STORE(((i_) < 4 ? cdst : cdst2)[MX * ((i_) & 3)], co[i_]);                        \
        } else if (256 * (i_) + tid < BT * SPEC_C && (int)((co_f1 >> (i_)) & 1u) < cfields && (!SPLIT || ((co_mine >> (i_)) & 1u))) \
            G2S_SPEC_STORE(cdst[256 * (i_)], make_double2(co[i_].x, ((co_m0 >> (i_)) & 1u) ? 0.0 : co[i_].y)); \
    } while (0)
            if (k >= 1 && k <= ksteps) {
                // ---- Legendre analysis (legendre.f90:114-155) on 4x4x4 blocks: D[n, col] += (P*wt)[n, lat] * E[lat, col]
                //   m' < 16 : one instruction per parity, blocks = n groups 0..3 of that parity (n = 2*(4*blk+i)+par)
                //   m' >= 16: <= 2 n groups per parity, both parities packed: blocks 0,1 even n, blocks 2,3 odd n
                // Fourier coefficient k of a row lives at z[k-1] (k >= 2), z[0] for k = 0, and Im(m'=0) = 0;
                // the float32(1/ix) scale of fourier.f90:72 is applied to E here.
                double *fbase = lds + ((k - 1) & 1) * G_TILE + (col >> 1) * (IL * G_ROW);
                // one slot = one zonal wavenumber of this wave: s_ its slot index (a runtime value in the SPLIT form), T1_ its
                // instruction form (compile-time: two parities x 6 k-steps, or 6 packed k-steps), AI_ its first operand register
#define G2S_SLOT(s_, T1_, AI_)                                                                             \
    do {                                                                                                   \
        const int m = mslot((s_), w), mc = min(m, MX - 1);                                                 \
        const int zi = mc == 0 ? 0 : 2 * mc + part - 1;                                                    \
        const double live = (mc == 0 && part == 1) ? 0.0 : fscale;                                         \
        double be[6], bo[6];                                                                               \
        UNROLL for (int ks = 0; ks < 6; ++ks) {                                                            \
            const int lat = 4 * ks + drow;                                                                 \
            const double south = fbase[(IL - 1 - lat) * G_ROW + zi], north = fbase[lat * G_ROW + zi];      \
            be[ks] = (south + north) * live;                                                               \
            bo[ks] = (south - north) * live;                                                               \
        }                                                                                                  \
        /* results go back into this wave's own (now consumed) columns; Im(m'=0) has no cell (it is 0) */  \
        const bool keep = m < MX && !(mc == 0 && part == 1);                                               \
        double *ob = fbase + zi;                                                                           \
        if (T1_) {                                                                                         \
            double acc0 = 0.0, acc1 = 0.0;                                                                 \
            G2S_SLOT_MFMA1(AI_);                                                                           \
            if (keep) {                                                                                    \
                const int n0 = 2 * (4 * blk + drow);                                                       \
                ob[n0 * G_ROW] = acc0;                                                                     \
                ob[(n0 + 1) * G_ROW] = acc1;                                                               \
            }                                                                                              \
        } else {                                                                                           \
            double acc = 0.0;                                                                              \
            G2S_SLOT_MFMA2(AI_);                                                                           \
            if (keep) {                                                                                    \
                const int n = 2 * (4 * (blk & 1) + drow) + (blk >> 1);           /* 0..15 */               \
                ob[n * G_ROW] = acc;                                                                       \
                ob[(n + 16) * G_ROW] = 0.0;                                      /* l > trunc+1: exactly 0 */ \
            }                                                                                              \
        }                                                                                                  \
    } while (0)
#define G2S_SLOT_MFMA1(AI_)                                                                                \
    UNROLL for (int ks = 0; ks < 6; ++ks) {                                                                \
        acc0 = MFMA4(areg[(AI_) + ks], be[ks], acc0);                                                      \
        acc1 = MFMA4(areg[(AI_) + 6 + ks], bo[ks], acc1);                                                  \
    }
#define G2S_SLOT_MFMA2(AI_) UNROLL for (int ks = 0; ks < 6; ++ks) acc = MFMA4(areg[(AI_) + ks], (blk >> 1) ? bo[ks] : be[ks], acc)
                if (SPLIT) {                                        // this workgroup's third
                    if (qpart < 2) {
                        G2S_SLOT(2 * qpart, true, 0);
                        G2S_SLOT(2 * qpart + 1, true, 12);
                    } else {
                        G2S_SLOT(4, false, 0);
                        G2S_SLOT(5, false, 6);
                        G2S_SLOT(6, false, 12);
                        G2S_SLOT(7, false, 18);
                    }
                    if (k >= 2) UNROLL for (int i = 0; i < 8; ++i) G2S_COPYOUT(i);
                } else {
                    int ai = 0;
                    UNROLL for (int s = 0; s < 8; ++s) {
                        G2S_SLOT(s, s < 4, ai);
                        ai += s < 4 ? 12 : 6;
                        if (k >= 2) G2S_COPYOUT(s);                 // one 1 KB store of tile k-2 per slot
                    }
                }
#undef G2S_SLOT
#undef G2S_SLOT_MFMA1
#undef G2S_SLOT_MFMA2
                PHASE_MARK(1, 5);
            } else if (k >= 2) {
                UNROLL for (int i = 0; i < 8; ++i) G2S_COPYOUT(i);  // drain: the last tile's spectra
            }
#undef G2S_COPYOUT
            if (PAIR && k >= 1) G2S_VDS_FACTORS();                   // for the next step's vds
            lds_barrier();                                          // B0
        }
#undef G2S_COMAP
#undef G2S_VDS_FACTORS
        TL_MARK(1, 31);
    }
}
#undef IS_PAIR
#undef G2S_SLOT_PART

#if defined(SPDY_WG_SPAN) && !defined(SPDY_PHASE_TRACE)
extern "C" __attribute__((visibility("default"))) int spdy_debug_wg_span(long long *out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wg_span), sizeof(long long) * 2 * 512 * 2);
}
#endif
#ifdef SPDY_PHASE_TRACE
extern "C" __attribute__((visibility("default"))) int spdy_debug_phase_trace(long long *out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_trace), sizeof(long long) * 2 * 8 * 8 * 8);
}
extern "C" __attribute__((visibility("default"))) int spdy_debug_wg_span(long long *out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wg_span), sizeof(long long) * 2 * 512 * 2);
}
extern "C" __attribute__((visibility("default"))) int spdy_debug_timeline(long long *out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_timeline), sizeof(long long) * 2 * 2 * 8 * 32);
}
#endif

hipError_t launch_s2g_fused(const DevPlan &p, const S2gFused &r, int max_wg, hipStream_t s)
{
    const int mode = r.mode, nb = r.nb, ngrad = r.ngrad;
    const int nplain = r.nplain[0] + r.nplain[1] + r.nplain[2] + r.nplain[3];
    if (nb <= 0 && nplain <= 0) return hipSuccess;
    // (mode 3 with nb = 0: plain segments only, one launch -- no pair tile reads spec / spec2 or writes grid / grid2)
    const bool pairs = mode == 1 || mode == 2 || (mode == 3 && nb > 0);
    if (mode < 0 || mode > 3 || (pairs && !r.grid2) || ((mode == 1 || (mode == 3 && nb > 0)) && !r.spec2)) return hipErrorInvalidValue;
    if (mode == 3 && (nb < 0 || nplain <= 0 || !r.plain[0] || !r.grid_p)) return hipErrorInvalidValue;
    if (ngrad < 0 || (ngrad > 0 && (mode != 3 || !r.psi || !r.gx || !r.gy || !r.zero || !p.gradx_e))) return hipErrorInvalidValue;
    S2gMixed mx{r.plain[0], r.kcos_p, r.kcos_all_p, r.grid_p, mode == 3 ? nb : 0, mode == 3 ? nplain : 0, ngrad, r.kcos_grad, r.psi, r.gx,
                r.gy, r.zero, {nullptr, nullptr, nullptr}, {0x7fffffff, 0x7fffffff, 0x7fffffff}};
    for (int i = 1, first = r.nplain[0]; i < 4; first += r.nplain[i++])
        if (r.nplain[i] > 0) { mx.seg_spec[i - 1] = r.plain[i]; mx.seg_first[i - 1] = first; }
    const int ntiles = mode == 3 ? nb + ngrad + (nplain + t30::BT - 1) / t30::BT : mode ? nb : (nb + t30::BT - 1) / t30::BT, nwg = max_wg;
    const dim3 grd(ntiles < nwg ? ntiles : nwg), blk(t30::NTHR);
    // grid-side bytes of this launch: pairs write two grids each
    const bool stream = stream_policy((long)(mode ? 2L * (nb + ngrad) : nb) * t30::IL * t30::IX * 8 + (mode == 3 ? (long)nplain * t30::IL * t30::IX * 8 : 0));
    // small batches (model-shaped launches, lone fields): work items = (tile, third of the latitudes), one per workgroup
    const bool no_part = p.lo.t30_nopart != 0;
    const bool by_part = 3 * ntiles <= nwg && p.img_s2g3 && !no_part && !stream;
    const dim3 grd3(3 * ntiles);
#define SPDY_S2G_LAUNCH(M)                                                                                                        \
    do {                                                                                                                          \
        if (by_part) hipLaunchKernelGGL((s2g_fused_t30_kernel<M, false, true>), grd3, blk, t30::S2G_LDS, s, p, nb, r.spec, r.spec2, r.d_kcos, r.kcos_all, r.grid, r.grid2, mx); \
        else if (stream) hipLaunchKernelGGL((s2g_fused_t30_kernel<M, true>), grd, blk, t30::S2G_LDS, s, p, nb, r.spec, r.spec2, r.d_kcos, r.kcos_all, r.grid, r.grid2, mx); \
        else hipLaunchKernelGGL((s2g_fused_t30_kernel<M, false>), grd, blk, t30::S2G_LDS, s, p, nb, r.spec, r.spec2, r.d_kcos, r.kcos_all, r.grid, r.grid2, mx);       \
    } while (0)
    if (mode == 1) SPDY_S2G_LAUNCH(1);
    else if (mode == 2) SPDY_S2G_LAUNCH(2);
    else if (mode == 3) SPDY_S2G_LAUNCH(3);
    else SPDY_S2G_LAUNCH(0);
#undef SPDY_S2G_LAUNCH
    return hipGetLastError();
}

hipError_t launch_g2s_fused(const DevPlan &p, const G2sFused &r, int max_wg, hipStream_t s)
{
    const int nb = r.nb, nplain = r.nplain;
    const bool mixed = nplain > 0;                            // pairs (grid, grid2 -> spec, spec2) + plain fields (grid_p -> spec_p)
    if (nb <= 0 && !mixed) return hipSuccess;
    if (p.trunc != t30::TRUNC || p.ix != t30::IX || p.il != t30::IL || !p.pa_dir2) return hipErrorInvalidValue;
    const bool pair = r.grid2 != nullptr;                     // vdspec in one pass: (grid, grid2) -> (spec, spec2)
    if (pair && (!r.gscale || !r.spec2)) return hipErrorInvalidValue;
    if (mixed && (!r.grid_p || !r.spec_p || (nb > 0 && !pair))) return hipErrorInvalidValue;
    const G2sMixed mx{r.grid_p, r.spec_p, mixed ? nb : 0, nplain};
    const int ntiles = mixed ? nb + (nplain + t30::BT - 1) / t30::BT : pair ? nb : (nb + t30::BT - 1) / t30::BT, nwg = max_wg > 0 ? max_wg : 256;
    const dim3 grd(ntiles < nwg ? ntiles : nwg), blk(t30::NTHR);
    const bool stream = stream_policy((long)((pair || mixed) ? 2L * nb : nb) * t30::IL * t30::IX * 8 + (mixed ? (long)nplain * t30::IL * t30::IX * 8 : 0));
    // small batches: three workgroups per tile, a third of the zonal wavenumbers each.  Measured (tools/t30_small_direct.py,
    // graph replays): plain 1-73 fields 8.9-9.3 -> 7.1-7.7 us per launch, a step's mixed 73-field launch 11.2 -> 9.8 us on its
    // own and 11.2 -> 10.15 us inside the captured T30 L8 step (34.5 -> 34.2 us: the launch in front of it gives 0.3 us back).
    // (Four workgroups per tile, slots {s, 7 - s} each, were 0.2 us faster alone and 0.2 us SLOWER in the step: there every
    // 128-byte line of spectra was written by two workgroups.)
    const bool no_split = p.lo.t30_nosplit != 0;
    // (up to a sixth as many tiles as CUs: at twice the T30 L8 step's 37 tiles -- T30 L16, 73 tiles, 219 workgroups -- the
    // captured step is 2 us SLOWER with the split form, 41.8 vs 39.7 us, although the launch on its own still gains)
    const bool by_split = r.allow_split && 6 * ntiles <= nwg && !no_split && !stream;
    const dim3 grd3(3 * ntiles);
#define SPDY_G2S_LAUNCH(M)                                                                                                        \
    do {                                                                                                                          \
        if (by_split) hipLaunchKernelGGL((g2s_fused_t30_kernel<M, false, 3>), grd3, blk, t30::G2S_LDS, s, p, nb, r.grid, r.grid2, r.gscale, r.spec, r.spec2, mx); \
        else if (stream) hipLaunchKernelGGL((g2s_fused_t30_kernel<M, true>), grd, blk, t30::G2S_LDS, s, p, nb, r.grid, r.grid2, r.gscale, r.spec, r.spec2, mx); \
        else hipLaunchKernelGGL((g2s_fused_t30_kernel<M, false>), grd, blk, t30::G2S_LDS, s, p, nb, r.grid, r.grid2, r.gscale, r.spec, r.spec2, mx);       \
    } while (0)
    if (mixed) SPDY_G2S_LAUNCH(3);
    else if (pair) SPDY_G2S_LAUNCH(2);
    else if (r.gscale) SPDY_G2S_LAUNCH(1);
    else SPDY_G2S_LAUNCH(0);
#undef SPDY_G2S_LAUNCH
    return hipGetLastError();
}
