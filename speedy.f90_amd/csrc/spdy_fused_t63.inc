// Fused, persistent, wave-specialised T63 kernels (included by spdy_kernels.hip after spdy_fused_t30.inc; shares its
// radix templates, MFMA4, lds_barrier).  A whole transform happens inside one workgroup, so HBM sees the algorithmic
// bytes only (the four-kernel path moves the 98 KB/field Fourier intermediate out and back in: 1.9x).
//
// A T63 field does not fit the LDS the way two T30 fields do (Fourier image 98 KB, grid 147 KB per field), and the
// Legendre table (0.9 MB of live P(m,n,lat)) cannot stay in registers.  So the work is cut differently:
//   * a tile is a PAIR of fields (4 real columns = 2 fields x re/im: a full v_mfma_f64_4x4x4_4b N dimension);
//   * the pair is walked in NCH = 6 latitude chunks of CP = 8 north/south latitude pairs (32 grid rows, 49 KB);
//     the Legendre sum over latitudes (direct transform) is ACCUMULATED across the six chunks in the matrix-core
//     accumulators, which stay in VGPRs (38 doubles per lane); for the inverse transform the pair's spectra are the
//     MFMA B operands and stay in VGPRs the same way while the six chunks of Fourier rows are produced;
//   * the four blocks of one MFMA are four consecutive zonal wavenumbers m' = 4q .. 4q+3 (a "quad") with the same
//     four total-wavenumber rows n -- so a 16-lane group of the D (resp. B) layout is 4 m' x (2 fields x re/im):
//     64 contiguous bytes of each field's spectrum, and spectra move between registers and HBM without an LDS pass;
//   * the A operands (P * weight, one 1 KB double2 fragment pair per (slot, chunk)) stream from L2: every workgroup
//     reads the same 0.9 MB image, once per field pair instead of once per field.
// Roles (8 waves, by SIMD): 4 Legendre waves (quads {w, 15-w, 4+w, 11-w}: 37-38 slots each, balanced) and 4 FFT waves in two
// groups of two (wave = one field of the pair: 16 rows x 4 lanes, 48-point register sub-transforms, the ido = 48 radix-4
// stage after lane transposes); a group spends two steps on a chunk (phases A and B), the groups alternate.  Three 32-row
// chunk buffers, ONE workgroup barrier (LDS only) per chunk step.
// Round-3 findings that shaped the code (DESIGN.md 4.3): no memory access under a lane-dependent condition (a guarded
// LDS read is a branch plus a dependent round trip; a guarded vector load makes the compiler wait vmcnt(0)); buffer
// addressing (scalar base + one lane offset + immediates) for every global stream; the stage's twiddle factors by the
// column-owner lane; far loads and the L2-hit A ring do not share a wave's in-order vmcnt stream gracefully.
#ifdef SPDY_T63_TRACE
// Debug-only s_memtime marks of workgroup 0: [kernel 0 = g2s, 1 = s2g][wave < 8][step < 24][mark < 8]
__device__ long long g_t63_trace[2 * 8 * 24 * 8];
#define T63_MARK(kern, step, mark)                                                                      \
    do {                                                                                                \
        if (blockIdx.x == 0 && lane == 0 && (step) < 24)                                                \
            g_t63_trace[(((kern) * 8 + w) * 24 + (step)) * 8 + (mark)] = __builtin_amdgcn_s_memtime();  \
    } while (0)
extern "C" __attribute__((visibility("default"))) int spdy_debug_t63_trace(long long *out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_t63_trace), sizeof(long long) * 2 * 8 * 24 * 8);
}
#else
#define T63_MARK(kern, step, mark) do { } while (0)
#endif
#ifndef T63_NEARLY
#define T63_NEARLY 2
#endif
#ifndef T63_RA               /* lane-transpose rounds (of 12) of the direct transform's FFT waves done in phase A */
#define T63_RA 6
#endif
// The wave index stays a VECTOR value to the compiler: as a scalar (readfirstlane) the role branches become real control flow
// and ROCm 7.2's allocator spills the FFT waves' register arrays (direct kernel 93 -> 282 us, round 3).
// Wave roles and SIMDs (hardware waves w and w + 4 of a workgroup share a SIMD: spdy_wave_placement checks it): waves 0-3 are
// the Legendre waves, 4-7 the FFT waves -- one of each per SIMD, the FFT wave at raised priority (T63_IS_FFT_D /
// T63_ROLE_INDEX_D; both kernels, every launch form, since the end of round 3: direct 83-84 -> 81-82 us at B = 1536, same bits).
// Until then the roles sat on separate SIMDs; the mixed placement first returned timing-dependent wrong grid values from the
// inverse kernel (a 128-bit buffer store's data registers rewritten one wait state behind it: DESIGN 4.3, t63_bstore2_safe,
// tools/store_valu_hazard.hip, tools/scan_store_hazard.py).  The placement and priority experiments of rounds 2-4 (roles by SIMD,
// younger-half priorities, ...) and the "(wrong results)" timing ablations live in tools/experiments/, not here.
#define T63_WAVE_ID(tid_) ((tid_) >> 6)
#define T63_IS_FFT_D(w_) (((w_) & 4) != 0)
#define T63_ROLE_INDEX_D(w_) ((w_) & 3)
// T63_SU(x): a wave-uniform value the compiler only knows as a vector (it derives from the wave index) as a SCALAR, for the
// chunk / pair walk: the segment-table lookups then are scalar loads from the kernel arguments instead of vector loads, each
// followed by s_waitcnt vmcnt(0) in the middle of the row prefetch stream.  (The wave index itself stays a vector value:
// as a scalar it turns the role / phase branches into real control flow and the register arrays spill, see above.)
#define T63_SU(x_) __builtin_amdgcn_readfirstlane(x_)
#ifndef T63_ZERO_AUX        /* ... and of its zero fill (the structurally zero half of every spectrum, which no later kernel reads) */
#define T63_ZERO_AUX T63_SPEC_AUX
#endif
#ifndef T63_STAGED_WT       /* staged direct form (model-sized launches): row workspace and spectra written through (sc0 sc1) */
#define T63_STAGED_WT 1
#endif
#ifndef T63_SPEC_AUX        /* cache policy of the direct transform's spectra stores: 0 default, 2 nt, 16 sc1, 17 sc0 sc1 */
#define T63_SPEC_AUX 0
#endif
namespace t63 {
// first zonal wavenumber of row n that no direct slot writes (the rest of the row is structurally zero)
__device__ __forceinline__ int first_unwritten_m(int n)
{
    int q = 0;
    while (q < NQ && (n >> 1) < 4 * ngrp(true, q, n & 1)) ++q;
    return 4 * q;
}
}  // namespace t63

// One launch may carry up to six independent sub-batches ("segments": own source and destination arrays, own scale / kcos
// policy) -- a model step's whole inverse or direct batch (U spectra -> ug, V spectra -> vg, plain spectra -> grids; scaled
// ug, vg -> spectra for vds, plain grids -> spectra) is ONE launch and one pipeline fill instead of three.  Field pairs are
// formed inside a segment; global pair index P = blockIdx.x + k * gridDim.x walks the segments in order.
struct T63PairRef {
    const double *src;      // segment source array
    double *dst;            // segment destination array
    const double *scale;    // direct: per-latitude factor on load (nullptr: none)
    const int *kcos;        // inverse: per-field kcos (nullptr: kcos_all)
    int kcos_all, nb;       // nb = fields of the segment
    long fld0;              // first field of the pair within the segment
    int op;                 // inverse: T63_OP_* (derived spectra: src / scale are the operator's inputs); direct: T63_OP_VDS -- the
                            // pair is (src[fld0], b.vds_src2[fld0]) -> vds -> (dst[fld0], b.vds_dst2[fld0])
};
// Fields per pair index of a segment: two consecutive fields of one array, or (T63_OP_VDS) one field of each of two arrays
#define T63_FLD0(g_, P_) ((g_).op == T63_OP_VDS ? (long)((P_) - (g_).pair0) : 2L * ((P_) - (g_).pair0))
__device__ __forceinline__ T63PairRef t63_pair(const T63Batch &b, long P)
{
    int s = 0;
    UNROLL for (int i = 1; i < T63_MAX_SEG; ++i)
        if (i < b.nseg && P >= b.seg[i].pair0) s = i;
    const T63Seg &g = b.seg[s];
    return T63PairRef{g.src, g.dst, g.scale, g.kcos, g.kcos_all, g.nb, T63_FLD0(g, P), g.op};
}

// t63_pair for a SCALAR pair index, by scalar loads straight from the kernel-argument segment.  The generic t63_pair compares
// 64-bit values (vector ALU: there is no scalar 64-bit signed compare), so the segment index is a vector value to the compiler;
// and a by-value argument is an SSA aggregate, which a dynamic index sends to a private (scratch) copy -- with the
// three-pair kernel's fifteen lookups per step that is what the compiler chose (424 scratch loads per variant); in the FFT waves of
// the pair kernels the generic lookup is ~100 scalar and vector instructions per chunk.  Reading the argument where the
// dispatcher put it keeps every lookup on the scalar unit: seven 32-bit compares and one s_load of the selected segment.
// CONTRACT: valid only inside a __global__ whose parameter list is EXACTLY (DevPlan p, T63Batch b) -- the batch is read from
// where the dispatcher put the second argument.  T63_KARG_CONTRACT(b) at the top of every such kernel states it in the code and,
// in the trace build, checks it on the device (a kernel with another signature would silently read the wrong bytes).
#ifdef SPDY_T63_TRACE
#define T63_KARG_CONTRACT(b_)                                                                                          \
    do {                                                                                                               \
        if (t63_batch_karg()->nseg != (b_).nseg || t63_batch_karg()->npairs != (b_).npairs || t63_batch_karg()->seg[0].src != (b_).seg[0].src) \
            __builtin_trap();                                                                                          \
    } while (0)
#else
#define T63_KARG_CONTRACT(b_) do { } while (0)
#endif
typedef const T63Batch __attribute__((address_space(4))) *T63BatchKarg;
__device__ __forceinline__ T63BatchKarg t63_batch_karg();
__device__ __forceinline__ T63BatchKarg t63_batch_karg()
{
    static_assert(sizeof(DevPlan) % 8 == 0 && alignof(T63Batch) <= 8, "second kernel argument follows the first without padding");
    const char __attribute__((address_space(4))) *ka = (const char __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
    return reinterpret_cast<T63BatchKarg>(ka + sizeof(DevPlan));
}
__device__ __forceinline__ T63PairRef t63_pair_s(T63BatchKarg b, int P)
{
    int s = 0;                                   // segments start in ascending order: the index is the number of starts <= P
    UNROLL for (int i = 1; i < T63_MAX_SEG; ++i) s += (int)(i < b->nseg) & (int)(P >= b->seg[i].pair0);
    s = T63_SU(s);
    return T63PairRef{b->seg[s].src, b->seg[s].dst, b->seg[s].scale, b->seg[s].kcos, b->seg[s].kcos_all, b->seg[s].nb, T63_FLD0(b->seg[s], P), b->seg[s].op};
}
// (the FFT waves' lookups; against the generic form: ~100 instructions fewer per chunk, the same launch times -- round 5 A/B)
#define T63_PAIR_FFT(P_) t63_pair_s(t63_batch_karg(), T63_SU(P_))
// How a workgroup walks the batch.  Throughput form: it owns whole pairs (P = blockIdx.x + k gridDim.x) and runs their six
// chunks in order, so a pair's operands are loaded once.  Inverse transform, small batches (by_chunk): the chunks of a pair
// are independent there, so the work items are (pair, chunk) = (I / NCH, I % NCH), I = blockIdx.x + u gridDim.x -- a 50-pair
// model-step batch then fills the chip with 300 one-chunk workgroups (3-4 pipeline steps) instead of 50 six-chunk ones (8).
// The by-chunk items of a workgroup are CONSECUTIVE (round 4): items I = blockIdx.x * ipw + u, i.e. neighbouring chunks of one
// pair, so the pair's spectra -- 38 far loads per lane, ~4 k ticks in front of a synthesis -- are fetched once per pair and not
// once per item (strided items: a model step's 546-item launch spent 9-11 k ticks per item in its Legendre waves, 4-6 k where no
// operands had to come: tools/phase_trace_t63.py 182).
// By-chunk launches with DERIVED segments (T63_OP_*, round 6): those segments come first in the launch and their b.nop_items
// items are walked ONE per workgroup (workgroup w = item w), the plain items behind them b.ipw per workgroup -- a derived pair's
// operands cost two memory round trips more than a plain pair's (t63_inv_load_b_op), a second item costs about as much, and a
// model step's launch leaves a third of the CUs idle anyway; so a workgroup never meets a derived pair in the middle of its
// walk (the in-loop operand load stays the plain one).  nop_items = 0: the walk of round 4.
template <bool BYCHUNK>
struct T63Walk {
    int T, ipw, base;
    __device__ __forceinline__ int item(int u) const { return BYCHUNK ? base + u : (int)blockIdx.x + u * (int)gridDim.x; }
    __device__ __forceinline__ long pair(int u) const { return BYCHUNK ? item(u) / t63::NCH : (long)blockIdx.x + (long)(u / t63::NCH) * gridDim.x; }
    __device__ __forceinline__ int chunk(int u) const { return BYCHUNK ? item(u) % t63::NCH : u % t63::NCH; }
};
template <bool BYCHUNK>
__device__ __forceinline__ T63Walk<BYCHUNK> t63_walk(const T63Batch &b)
{
    T63Walk<BYCHUNK> w;
    const int units = BYCHUNK ? b.npairs * t63::NCH : b.npairs;
    const int mine = ((int)blockIdx.x < units) ? (units - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
    const int nop = BYCHUNK ? b.nop_items : 0, bid = (int)blockIdx.x;
    w.ipw = BYCHUNK ? b.ipw : 1;
    w.base = bid < nop ? bid : nop + (bid - nop) * w.ipw;
    w.T = BYCHUNK ? (bid < nop ? 1 : max(0, min(w.ipw, units - w.base))) : mine * t63::NCH;
    return w;
}

// ------------------------------------------------------------------------------------------
// grid_to_spec, fused, T63 (spectral.f90:112-122).  spec[nb][65][64] complex <- grid[nb][96][192]
//   step t (chunk t of this workgroup's pair sequence): FFT waves put chunk t into row buffer t%2 (grid rows ->
//   Fourier coefficients in place) and prefetch chunk t+1; Legendre waves accumulate chunk t-1 from buffer (t-1)%2
//   and, after a pair's last chunk, write its spectra.
// MODE 0 plain; MODE 1: every grid row is multiplied by gscale[latitude] on the way in (vdspec's cosgr / cosgr2).
// ------------------------------------------------------------------------------------------
// A-operand ring: T63_PF fragment pairs (1 KB each per wave) in flight per Legendre wave, running ACROSS chunk steps -- the
// stream is L2-latency bound (a 6-deep ring measured 15.8k ticks per step: 38 KB per wave at 6 KB per round trip), and the
// loads of the next chunk do not depend on its rows, so they are issued before the step barrier.
#ifndef T63_PF
#define T63_PF 12
#endif
#ifndef T63_PF_D            /* ring depth of the direct / of the inverse kernel */
#define T63_PF_D T63_PF
#endif
#ifndef T63_PF_I
#define T63_PF_I T63_PF
#endif
// Buffer-addressed global access (scalar base in a resource descriptor + 32-bit lane offset + scalar offset): the 64-bit
// per-lane address arithmetic of flat/global instructions (6-8 vector integer ops per access) disappears, and the cache policy
// is an immediate.  aux: 0 default, 2 nt (streaming), 16 sc1, 17 sc0 sc1.  The base must be wave-uniform (T63_SU).
typedef unsigned int spdy_u4 __attribute__((ext_vector_type(4)));
typedef unsigned int spdy_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t t63_rsrc(const void *base)
{
    // the base IS wave-uniform (kernel arguments, the segment table, scalar indices), but where the compiler cannot prove it
    // (a pointer selected by a runtime value) it wraps every buffer access in a waterfall loop: say so explicitly
    const unsigned long long a = reinterpret_cast<unsigned long long>(base);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((unsigned long long)hi << 32) | lo), 0, 0x7fffffff, 0x00020000);
}
template <int AUX>
__device__ __forceinline__ void t63_bstore2(__amdgpu_buffer_rsrc_t r, int voff, int soff, double2 v)
{
    const unsigned long long a = __double_as_longlong(v.x), b = __double_as_longlong(v.y);
    spdy_u4 w;
    w.x = (unsigned)a; w.y = (unsigned)(a >> 32); w.z = (unsigned)b; w.w = (unsigned)(b >> 32);
    __builtin_amdgcn_raw_buffer_store_b128(w, r, voff, soff, AUX);
}
template <int AUX>
__device__ __forceinline__ void t63_bstore1(__amdgpu_buffer_rsrc_t r, int voff, int soff, double v)
{
    const unsigned long long a = __double_as_longlong(v);
    spdy_u2 w;
    w.x = (unsigned)a; w.y = (unsigned)(a >> 32);
    __builtin_amdgcn_raw_buffer_store_b64(w, r, voff, soff, AUX);
}
// the same descriptor as four scalar words (operand of the inline-assembly store below)
__device__ __forceinline__ spdy_u4 t63_rsrc_u4(const void *base)
{
    const unsigned long long a = reinterpret_cast<unsigned long long>(base);
    spdy_u4 r;
    r.x = __builtin_amdgcn_readfirstlane((unsigned)a);
    r.y = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32)) & 0xffffu;
    r.z = 0x7fffffffu;
    r.w = 0x00020000u;
    return r;
}
// 128-bit buffer store whose data registers cannot be rewritten before two wait states have passed (see the inverse
// kernel's copy-out)
template <bool NT, bool WT = false>     // NT: streaming; WT: write-through (sc0 sc1)
__device__ __forceinline__ void t63_bstore2_safe(spdy_u4 r, int voff, int soff, double2 v)
{
    const unsigned long long a = __double_as_longlong(v.x), b = __double_as_longlong(v.y);
    spdy_u4 w;
    w.x = (unsigned)a; w.y = (unsigned)(a >> 32); w.z = (unsigned)b; w.w = (unsigned)(b >> 32);
    if (NT) asm volatile("buffer_store_dwordx4 %0, %1, %2, %3 offen nt\n\ts_nop 1" :: "v"(w), "v"(voff), "s"(r), "s"(soff) : "memory");
    else if (WT) asm volatile("buffer_store_dwordx4 %0, %1, %2, %3 offen sc0 sc1\n\ts_nop 1" :: "v"(w), "v"(voff), "s"(r), "s"(soff) : "memory");
    else asm volatile("buffer_store_dwordx4 %0, %1, %2, %3 offen\n\ts_nop 1" :: "v"(w), "v"(voff), "s"(r), "s"(soff) : "memory");
}
template <int AUX>
__device__ __forceinline__ double2 t63_bload2(__amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    const spdy_u4 w = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, AUX);
    return make_double2(__longlong_as_double(((unsigned long long)w.y << 32) | w.x), __longlong_as_double(((unsigned long long)w.w << 32) | w.z));
}
template <int AUX>
__device__ __forceinline__ double t63_bload1(__amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    const spdy_u2 w = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, AUX);
    return __longlong_as_double(((unsigned long long)w.y << 32) | w.x);
}

// One A-operand fragment pair (1 KB per wave).  (A buffer-addressed form -- scalar descriptor, one lane-offset register -- and
// sc0 / sc1 / nt policies on these loads were measured neutral or worse in rounds 3-4: tools/experiments/.)
#define T63_AFRAG(aimg_, f0_, s_, lane_) (aimg_)[((f0_) + (s_) * AFRAG_SLOT_STRIDE) * 64 + (lane_)]
#define T63_AFRAG_FLAT T63_AFRAG
#define T63_AFRAG_D T63_AFRAG
#define T63_AFRAG_I T63_AFRAG
// (Round 6 re-measured two cheaper address forms of these loads with the roles sharing SIMDs -- buffer loads off one descriptor and
// one lane offset: inverse +5 us, direct neutral; a 64-bit base pointer per chunk with the slot in the load's immediate offset,
// 85 vector instructions fewer per synthesis: neutral in both kernels.  The Legendre wave's instruction count is not what the
// step waits for.  DESIGN 4.3; the knobs are in the git history at commit "T63: buffer-addressed operand ring re-measured".)
template <bool DIR, int W, int PF, int S0 = 0>
__device__ __forceinline__ void t63_ring_init(const double2 *__restrict__ aimg, int c, int lane, double2 (&ring)[PF])
{
    using namespace t63;
    UNROLL for (int s = 0; s < PF; ++s) ring[s] = T63_AFRAG(aimg, afrag(W, S0, c), s, lane);
}

// lane ^ 1 of a double through the DPP crossbar (quad_perm [1,0,3,2]): no LDS round trip
__device__ __forceinline__ double t63_quad_xor1(double x)
{
    const unsigned long long a = __double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)a, 0xB1, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(a >> 32), 0xB1, 0xF, 0xF, true);
    return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

// [IB, IE): the wave's quad positions this workgroup contracts -- all four, or one half of them in the split launch of
// small batches (g2s_fused_t63_kernel<.., SPLIT>); the operand ring then runs over that half's slots only.
template <int W, int IB = 0, int IE = 4>
__device__ __forceinline__ void t63_dir_contract(const double *buf, int c, int cnext, const double2 *__restrict__ aimg, double fscale,
                                                 int lane, double (&acc)[t63::MAXS], double2 (&ring)[T63_PF_D])
{
    using namespace t63;
    asm volatile("" : "+v"(lane));      // opaque per call: LDS / image offsets of the four wave variants are recomputed each
                                        // step (a few integer ops) instead of living in ~20 registers across the loop
    const int blk = (lane >> 2) & 3, col = lane & 3, drow = lane >> 4, part = col & 1, f = col >> 1;
    // uniform (scalar) bases, the lane enters as a 32-bit offset: one address register for the whole stream instead of
    // one 64-bit pair per slot (the offsets exceed the instruction's immediate range)
    constexpr int S0 = slot_of(true, W, IB, 0, 0);                  // first slot of the range; ring positions count from it
    const int fc = afrag(W, S0, c), fn = afrag(W, S0, cnext);
    constexpr int NS = slot_of(true, W, IE, 0, 0) - S0, PF = T63_PF_D, NSP = (NS + PF - 1) / PF * PF;
    UNROLL for (int i = IB; i < IE; ++i) {
        const int q = wave_quad(W, i), m = 4 * q + blk;
        const int zi = m == 0 ? 0 : 2 * m + part - 1;
        const double live = (m == 0 && part == 1) ? 0.0 : fscale;
        double be[2], bo[2];
        UNROLL for (int ks = 0; ks < 2; ++ks) {
            const int il = 4 * ks + drow;                                   // latitude within the chunk
            const double lo = buf[(f * 16 + il) * RS + zi], hi = buf[(f * 16 + 8 + il) * RS + zi];   // rows lat, IL-1-lat
            be[ks] = (hi + lo) * live;
            bo[ks] = (hi - lo) * live;
        }
        UNROLL for (int par = 0; par < 2; ++par) {
            UNROLL for (int g = 0; g < 9; ++g) {
                if (g < ngrp(true, q, par)) {
                    const int s = slot_of(true, W, i, par, g), r = s - S0;
                    const double2 a = ring[r % PF];
                    if (r + PF < NS) ring[r % PF] = T63_AFRAG_D(aimg, fc, r + PF, lane);
                    else if (r + PF >= NSP) ring[r % PF] = T63_AFRAG_D(aimg, fn, r + PF - NSP, lane);   // first slots of the next chunk
                    acc[s] = MFMA4(a.x, par ? bo[0] : be[0], acc[s]);
                    acc[s] = MFMA4(a.y, par ? bo[1] : be[1], acc[s]);
                }
            }
        }
    }
    // ring positions whose turn falls on a virtual slot NS <= s < NSP
    UNROLL for (int r = NS; r < NSP; ++r)
        if (r + PF >= NSP) ring[r % PF] = T63_AFRAG_D(aimg, fn, r + PF - NSP, lane);
}

// spectra of one field pair out of the accumulators: 16-byte stores, 64 contiguous bytes per 16-lane group and field
template <int W, int IB = 0, int IE = 4, int AUX = T63_SPEC_AUX>
__device__ __forceinline__ void t63_dir_writeout(double *__restrict__ spec, long fld0, int nfld, int lane, double (&acc)[t63::MAXS])
{
    using namespace t63;
    asm volatile("" : "+v"(lane));      // opaque per call: the ~40 store addresses are computed here, not hoisted out of the
                                        // step loop into registers that then spill next to the accumulators
    const int blk = (lane >> 2) & 3, col = lane & 3, drow = lane >> 4, part = col & 1, f = col >> 1;
    UNROLL for (int i = IB; i < IE; ++i) {
        const int q = wave_quad(W, i), m = 4 * q + blk;
        UNROLL for (int par = 0; par < 2; ++par) {
            UNROLL for (int g = 0; g < 9; ++g) {
                if (g < ngrp(true, q, par)) {
                    const int s = slot_of(true, W, i, par, g);
                    const double re = acc[s], im = __shfl_xor(re, 1);
                    acc[s] = 0.0;
                    const int n = 2 * (4 * g + drow) + par;
                    {
                        const __amdgpu_buffer_rsrc_t rw = t63_rsrc(spec + fld0 * (long)(2 * NX * MX));
                        const bool wr = part == 0 && n < NX && f < nfld;
                        t63_bstore2<AUX>(rw, wr ? ((f * NX + n) * MX + m) * 16 : (int)0x80000000, 0, make_double2(re, im));
                    }
                }
            }
        }
    }
}

// ... the same for a wave that holds all four of its quads (the whole-pair walk): the quads of positions (0, 2) and of (3, 1)
// are neighbours -- an even quad qe and qe + 1 (spdy_t63_sched.hpp) -- so ONE store carries a slot of each: the lanes with
// part = 0 store the even quad's coefficient (re their own value, im their neighbour lane's), the lanes with part = 1 -- idle in
// the form above -- the odd quad's (re the neighbour's, im their own).  Per (n, field) that is 8 zonal wavenumbers x 16 bytes
// = one whole 128-byte line, and 19-20 store instructions per wave instead of 37-38 with half their lanes off.  (The even quad
// has at most one n-group more than the odd one: that slot leaves as a half-line store, as above.)
template <int W, int AUX = T63_SPEC_AUX>
__device__ __forceinline__ void t63_dir_writeout_pairs(double *__restrict__ spec, long fld0, int nfld, int lane, double (&acc)[t63::MAXS])
{
    using namespace t63;
    asm volatile("" : "+v"(lane));      // (opaque per call, as above)
    const int blk = (lane >> 2) & 3, col = lane & 3, drow = lane >> 4, part = col & 1, f = col >> 1;
    const __amdgpu_buffer_rsrc_t rw = t63_rsrc(spec + fld0 * (long)(2 * NX * MX));
    UNROLL for (int pp = 0; pp < 2; ++pp) {
        const int ie = pp == 0 ? 0 : 3, io = pp == 0 ? 2 : 1;            // positions of the even quad and of its odd neighbour
        const int qe = wave_quad(W, ie), qo = wave_quad(W, io);
        static_assert(wave_quad(W, 2) == wave_quad(W, 0) + 1 && wave_quad(W, 1) == wave_quad(W, 3) + 1 && wave_quad(W, 0) % 2 == 0 && wave_quad(W, 3) % 2 == 0,
                      "neighbouring quads at positions (0, 2) and (3, 1)");
        const int m = 4 * (part == 0 ? qe : qo) + blk;
        UNROLL for (int par = 0; par < 2; ++par) {
            UNROLL for (int g = 0; g < 9; ++g) {
                const bool he = g < ngrp(true, qe, par), ho = g < ngrp(true, qo, par);
                if (he || ho) {
                    const int se = he ? slot_of(true, W, ie, par, g) : 0, so = ho ? slot_of(true, W, io, par, g) : 0;
                    const double xe = he ? acc[se] : 0.0, xo = ho ? acc[so] : 0.0;
                    const double xe_n = __shfl_xor(xe, 1), xo_n = __shfl_xor(xo, 1);
                    if (he) acc[se] = 0.0;
                    if (ho) acc[so] = 0.0;
                    const double re = part == 0 ? xe : xo_n, im = part == 0 ? xe_n : xo;
                    const int n = 2 * (4 * g + drow) + par;
                    const bool wr = n < NX && f < nfld && (part == 0 ? he : ho);
                    t63_bstore2<AUX>(rw, wr ? ((f * NX + n) * MX + m) * 16 : (int)0x80000000, 0, make_double2(re, im));
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// The ido = 48 radix-4 stage of the N = 192 transforms, in registers.  The four lanes l, l+16, l+32, l+48 of a row hold
// the four 48-point sub-transforms y_h[0..47].  A butterfly needs the same positions of all four, so the 48 values are
// redistributed first: twelve 4x4 lane transposes (v_permlane32_swap + v_permlane16_swap, two stages each) leave lane h
// with all four columns of the 12 positions of ITS butterflies -- items h, h+4, h+8 of fftpack's 13 (item it = the
// butterfly pair p = 2 it - 1 and 46 - p; lane 0 also takes the i = 0 / i = 47 specials and the self-paired p = 23).
// No LDS round trip between the sub-transforms and the last stage; only final coefficients are written.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void t63_swap32(double &x, double &y)     // x[hi 32 lanes] <-> y[lo 32 lanes]
{
    const unsigned long long a = __double_as_longlong(x), b = __double_as_longlong(y);
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)a, (unsigned)b, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(a >> 32), (unsigned)(b >> 32), false, false);
    x = __longlong_as_double(((unsigned long long)hi[0] << 32) | lo[0]);
    y = __longlong_as_double(((unsigned long long)hi[1] << 32) | lo[1]);
}
__device__ __forceinline__ void t63_swap16(double &x, double &y)     // x[odd rows of 16] <-> y[even rows of 16]
{
    const unsigned long long a = __double_as_longlong(x), b = __double_as_longlong(y);
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)a, (unsigned)b, false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(a >> 32), (unsigned)(b >> 32), false, false);
    x = __longlong_as_double(((unsigned long long)hi[0] << 32) | lo[0]);
    y = __longlong_as_double(((unsigned long long)hi[1] << 32) | lo[1]);
}
// position (0..47) that register slot k of transpose round rho carries: it ends up in lane k
constexpr int t63_pos(int k, int rho)
{
    const int g = rho / 4, e = rho % 4;
    if (k == 0 && g == 0) return e == 0 ? 0 : e == 1 ? 47 : e == 2 ? 23 : 24;
    const int it = k + 4 * g, p = 2 * it - 1, q = 46 - p;
    return e == 0 ? p : e == 1 ? p + 1 : e == 2 ? q : q + 1;
}
// The lane transposes, IN PLACE, rounds [R0, R1): in y = this lane's 48-point sub-transform (lane h = lane >> 4); round rho
// leaves column j of this lane's position rho in y[t63_pos(j, rho)]
// (the register the value of lane j's sub-transform at that position came from), so there is no second 48-double array and
// the twelve rounds can be split between the two phases of a chunk.
template <int R0, int R1>
__device__ __forceinline__ void t63_redistribute_inplace(double (&y)[48])
{
    UNROLL for (int rho = R0; rho < R1; ++rho) {
        double r0 = y[t63_pos(0, rho)], r1 = y[t63_pos(1, rho)], r2 = y[t63_pos(2, rho)], r3 = y[t63_pos(3, rho)];
        t63_swap32(r0, r2);
        t63_swap32(r1, r3);
        t63_swap16(r0, r1);
        t63_swap16(r2, r3);
        y[t63_pos(0, rho)] = r0; y[t63_pos(1, rho)] = r1; y[t63_pos(2, rho)] = r2; y[t63_pos(3, rho)] = r3;
    }
}

// fftpack radf4 (ido = 48, l1 = 1), the butterflies: on values whose twiddle factors have already been applied by the lanes that own the columns
// (t63_twiddle_column_fwd, before the lane transposes): v[4 rho + j] = (cr_j, ci_j) of this lane's position rho; additions only,
// no LDS reads in front of the butterflies.
// The values sit where t63_redistribute_inplace left them: column j of round rho in v[t63_pos(j, rho)].
__device__ __forceinline__ void t63_radf4_last_raw(const double (&v)[48], double *z, double hsqt2, int h)
{
#define T63F_V(R_, j_) v[t63_pos(j_, R_)]
#define T63F_RAW(p_, q_, R0, R1)                                                                                   \
    do {                                                                                                          \
        const double a0 = T63F_V(R0, 0), cr2 = T63F_V(R0, 1), cr3 = T63F_V(R0, 2), cr4 = T63F_V(R0, 3);            \
        const double a1 = T63F_V(R1, 0), ci2 = T63F_V(R1, 1), ci3 = T63F_V(R1, 2), ci4 = T63F_V(R1, 3);            \
        const double sr1 = cr2 + cr4, sr4 = cr4 - cr2, si1 = ci2 + ci4, si4 = ci2 - ci4;                           \
        const double si2 = a1 + ci3, si3 = a1 - ci3, sr2 = a0 + cr3, sr3 = a0 - cr3;                               \
        z[p_] = sr1 + sr2;                                                                                         \
        z[(p_) + 1] = si1 + si2;                                                                                   \
        z[48 + (q_)] = sr3 - si4;                                                                                  \
        z[48 + (q_) + 1] = sr4 - si3;                                                                              \
        if (96 + (p_) + 1 < 2 * t63::MX) {                                                                         \
            z[96 + (p_)] = si4 + sr3;                                                                              \
            z[96 + (p_) + 1] = sr4 + si3;                                                                          \
        }                                                                                                          \
    } while (0)
    if (h == 0) {
        const double a0 = T63F_V(0, 0), a1 = T63F_V(0, 1), a2 = T63F_V(0, 2), a3 = T63F_V(0, 3);
        const double e0 = T63F_V(1, 0), e1 = T63F_V(1, 1), e2 = T63F_V(1, 2), e3 = T63F_V(1, 3);
        const double tr1 = a1 + a3, tr2 = a0 + a2;
        const double ti1 = -hsqt2 * (e1 + e3), ur1 = hsqt2 * (e1 - e3);
        z[0] = tr1 + tr2;
        z[48 + 47] = a0 - a2;
        z[96] = a3 - a1;
        z[47] = ur1 + e0;
        z[48] = ti1 - e2;
        T63F_RAW(23, 23, 2, 3);
    } else {
        const int p = 2 * h - 1, q = 46 - p;
        T63F_RAW(p, q, 0, 1);
        T63F_RAW(q, p, 2, 3);
    }
    UNROLL for (int g = 1; g < 3; ++g) {
        const int p = 2 * (h + 4 * g) - 1, q = 46 - p;
        T63F_RAW(p, q, 4 * g, 4 * g + 1);
        T63F_RAW(q, p, 4 * g + 2, 4 * g + 3);
    }
#undef T63F_RAW
#undef T63F_V
}
// forward (radf4, fftpack.f90:905-910): cr = wr y[p] + wi y[p+1], ci = wr y[p+1] - wi y[p]; factor pairs as t63_load_column_twiddles
__device__ __forceinline__ void t63_twiddle_column_fwd(double (&y)[48], const double *twc)
{
    UNROLL for (int j = 0; j < 23; ++j) {
        const double2 wq = *reinterpret_cast<const double2 *>(twc + 2 * j);
        const double yr = y[2 * j + 1], yi = y[2 * j + 2];
        y[2 * j + 1] = wq.x * yr + wq.y * yi;
        y[2 * j + 2] = wq.x * yi - wq.y * yr;
    }
}

template <int W, int IB = 0, int IE = 4>
__device__ __forceinline__ void t63_dir_legendre_wave(const DevPlan &p, const T63Batch &b, double *lds, int bid, int gdim, int T, int lane)
{
    using namespace t63;
    const int w = T63_WAVE_ID(threadIdx.x);                   // (trace builds: T63_MARK)
    (void)w;
    double acc[MAXS];
    UNROLL for (int s = 0; s < MAXS; ++s) acc[s] = 0.0;
    const double fscale = c_fft192.scale;
    const double2 *aimg = reinterpret_cast<const double2 *>(p.img_g2s63);
    double2 ring[T63_PF_D];
    t63_ring_init<true, W, T63_PF_D, slot_of(true, W, IB, 0, 0)>(aimg, 0, lane, ring);
    lds_barrier();                                             // (T)
    for (int t = 0; t <= T + 1; ++t) {
        T63_MARK(0, t, 0);
        if (t >= 2) {
            const int tc = t - 2, k = tc / NCH, c = tc - k * NCH, cn = c + 1 == NCH ? 0 : c + 1;
            const double *buf = lds + (tc % NBUF) * BUF;
            // (every pair's spectra leave in one burst behind the barrier of its last chunk's step; the form that stored them inside
            // the next pair's first contraction measured 88 against 85 us in round 3: tools/experiments/)
            t63_dir_contract<W, IB, IE>(buf, c, cn, aimg, fscale, lane, acc, ring);
            T63_MARK(0, t, 1);
        }
        T63_MARK(0, t, 4);
        lds_barrier();
        // The write-out reads registers only: BEHIND the step barrier it runs beside the FFT waves' next step instead of holding
        // them at the barrier (the last chunk's step of a pair was 13-16 k ticks against 7.7 k; round 5: 81.3-82.7 -> 80.4-80.6 us at
        // B = 1536, same bits).
        if (t >= 2 && (t - 2) % NCH == NCH - 1) {              // the pair is complete: spectra out, accumulators reset
            const T63PairRef pr = t63_pair(b, bid + (long)((t - 2) / NCH) * gdim);
            if (IB == 0 && IE == 4) t63_dir_writeout_pairs<W>(pr.dst, pr.fld0, (int)min(2L, (long)pr.nb - pr.fld0), lane, acc);
            else
            t63_dir_writeout<W, IB, IE>(pr.dst, pr.fld0, (int)min(2L, (long)pr.nb - pr.fld0), lane, acc);
        }
    }
}

// vdspec pairs (T63_OP_VDS, row f1 at T63 -- staged form): the pair's two fields are (u, v); quad position I of wave W holds, per
// lane (zonal wavenumber m = 4 q + blk, column = (field, re | im), row drow of the slot's four), the coefficients of its slots, and
// vds (spectral.f90:146-171)
//     vor(m, n) =  vddym u(m, n-1) - vddyp u(m, n+1) + (0, 1) gradx v(m, n)       div(m, n) = -vddym v(m, n-1) + vddyp v(m, n+1) + (0, 1) gradx u(m, n)
// is evaluated on them in registers: the n +- 1 neighbours are the other parity's slot of the same quad, in the same lane or one
// 16-lane row away (n = 2 (4 g + drow) + par); the other field's value for the (0, 1) term is two lanes away (DPP); what lies
// outside the wave's slots is structurally zero (the transform writes nothing there).  vds reaches ONE row beyond the transform's
// triangle (row nmax + 1 of every column, incl. row nx): one halo group per parity.  vorticity -> dst, divergence -> dst2, 16-byte
// stores of the (re, im) pairs; everything else of the two spectra is the rows launch's zero fill.
__device__ __forceinline__ double t63_quad_perm(double x, int ctrl)     // DPP quad_perm: 0x4E = lane ^ 2, 0x1B = lane ^ 3, 0xB1 = lane ^ 1
{
    const unsigned long long a = __double_as_longlong(x);
    unsigned lo, hi;
    if (ctrl == 0x4E) { lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)a, 0x4E, 0xF, 0xF, true); hi = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(a >> 32), 0x4E, 0xF, 0xF, true); }
    else if (ctrl == 0x1B) { lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)a, 0x1B, 0xF, 0xF, true); hi = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(a >> 32), 0x1B, 0xF, 0xF, true); }
    else { lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)a, 0xB1, 0xF, 0xF, true); hi = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(a >> 32), 0xB1, 0xF, 0xF, true); }
    return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}
template <int W, int I>
__device__ __forceinline__ void t63_dir_writeout_vds(const DevPlan &p, const T63PairRef &pr, double *dst2, int lane, const double (&acc)[t63::MAXS])
{
    using namespace t63;
    constexpr int q = wave_quad(W, I), G0 = ngrp(true, q, 0), G1 = ngrp(true, q, 1);
    const int blk = (lane >> 2) & 3, col = lane & 3, drow = lane >> 4, part = col & 1, f = col >> 1, m = 4 * q + blk;
    const int lane_dn = (lane + 48) & 63, lane_up = (lane + 16) & 63;      // the lanes that hold drow - 1 / drow + 1 of this (m, column)
    // own field's coefficients by (parity, group); groups the wave has no slot for are structurally zero
    double x0[10], x1[10];
    UNROLL for (int g = 0; g < 10; ++g) {
        x0[g] = g < G0 ? acc[slot_of(true, W, I, 0, g)] : 0.0;
        x1[g] = g < G1 ? acc[slot_of(true, W, I, 1, g)] : 0.0;
    }
    const double sg = f ? -1.0 : 1.0, gx = p.gradx[m];
    double *const out = (f ? dst2 : pr.dst) + pr.fld0 * (long)(2 * NX * MX);
    UNROLL for (int par = 0; par < 2; ++par) {
        UNROLL for (int g = 0; g < 10; ++g) {
            if (g <= (par ? G1 : G0) && 8 * g + par <= NX - 1) {               // the parity's slots and its halo group
                const int n = 2 * (4 * g + drow) + par, nc = min(n, NX - 1), e = nc * MX + m;
                double xm, xp;                                                 // own field at n - 1, n + 1
                if (par == 0) {
                    const double a = __shfl(x1[g], lane_dn), b = g > 0 ? __shfl(x1[g - 1], lane_dn) : 0.0;
                    xm = drow == 0 ? b : a;
                    xp = x1[g];
                } else {
                    const double a = __shfl(x0[g], lane_up), b = g + 1 < 10 ? __shfl(x0[g + 1], lane_up) : 0.0;
                    xm = x0[g];
                    xp = drow == 3 ? b : a;
                }
                const double xs = par ? x1[g] : x0[g];
                const double ysame = t63_quad_perm(xs, 0x4E), ycross = t63_quad_perm(xs, 0x1B);     // other field: same part, other part
                const double dm = sg * p.vddym[e], dp = -sg * p.vddyp[e];
                const double gs = gx * ysame, gc = gx * ycross;                 // real x complex, then the full (0, 1) multiply
                double zi = part ? gc + gs * 0.0 : gs * 0.0 - gc;
                if (n >= NX - 1) zi = 0.0;                                      // row nx: vddym u(n-1) only
                const double v = (dm * xm + dp * xp) + zi;
                const double vn = t63_quad_perm(v, 0xB1);                       // the (re, im) partner
                if (part == 0 && n < NX) store2_wt(reinterpret_cast<double2 *>(out) + e, make_double2(v, vn));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// STAGED form of small direct batches (at most a third as many pairs as CUs: every model-sized T63 batch).  In the fused walk a
// lone pair is a chain of eight steps whose length is ONE FFT wave's phase (5.9 k ticks of 48-point sub-transforms on one SIMD;
// tools/phase_trace_t63.py 146: steps of 6.3-6.6 k ticks, the Legendre waves busy for 1.7-2.4 k of each) -- yet the row FFTs of
// different chunks do not depend on each other; only the contraction accumulates over the chunks, in chunk order.  And a
// workgroup that contracts a whole pair (or half of one, SPLIT below) pulls 0.45-0.9 MB of operand image and 196 KB of rows
// through ONE CU.  So the two halves run as two launches of many small work items:
//   g2s_rows_t63_kernel      work item = (pair, chunk, field) per WAVE, four waves per workgroup, no barrier behind the table
//                            set-up: grid rows -> the chunk's Fourier rows, by exactly the code of the fused kernel's FFT waves
//                            (phases A and B back to back), into the plan's row workspace [pair][chunk][field][16 rows][128]
//                            (98 KB per field: cache-resident at these sizes); also the structurally zero part of the spectra;
//   g2s_contract_t63_kernel  work item = (pair, quad position i of the slot schedule) per workgroup, wave w = Legendre wave w of
//                            the fused kernel restricted to its quad wave_quad(w, i): no LDS, no barrier -- each lane fetches the
//                            24 Fourier coefficients it multiplies (six chunks) straight from the workspace into registers and
//                            streams its 9-17 slots' operand fragments, one chunk ahead.
// Every Fourier row is computed, and every coefficient accumulated over the chunks, by the same instructions on the same values
// in the same order as in the fused walk: bit-identical (tests/test_gpu_determinism.py::test_t63_small_direct_forms_agree).
// ------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void g2s_rows_t63_kernel(DevPlan p, T63Batch b)
{
    using namespace t63;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int WROWS = 16 * RS;                                 // one wave's 16 row slots
    double *tw = lds + 4 * WROWS;
    int *zfirst = reinterpret_cast<int *>(tw + TW);                // [NX] first structurally-zero m' of every spectral row
    const int tid = threadIdx.x, lane = tid & 63, wi = tid >> 6;
    for (int e = tid; e < TW; e += 256) tw[e] = e < 48 ? (double)((e & 1) ^ 1) : c_fft192.first[e - 48];
    for (int e = tid; e < NX; e += 256) zfirst[e] = first_unwritten_m(e);
    lds_barrier();                                                 // tables ready; from here on every wave is on its own
    const int item = T63_SU(4 * (int)blockIdx.x + wi);             // ((pair, chunk), field of the pair)
    if (item >= 2 * NCH * b.npairs) return;
    const int fw = item & 1, c = (item >> 1) % NCH;
    const long P = (item >> 1) / NCH;
    const T63PairRef pr = t63_pair(b, P);
    const int l16 = lane & 15, rl = lane >> 4;
    double2 pre[24];
    {   // the wave's 16 grid rows (as T63_PREFETCH of the fused kernel): 8 of latitudes 8c.., 8 of their mirror images
        // (T63_OP_VDS: the pair's two fields are field fld0 of TWO arrays -- fw is wave-uniform, the base is a scalar select)
        const bool vds = T63_SU(pr.op) == T63_OP_VDS;
        const __amdgpu_buffer_rsrc_t rs = t63_rsrc((vds && fw ? b.vds_src2 : pr.src) + pr.fld0 * (long)(IL * IX));
        const int vl = (vds ? 0 : min(fw, (int)(pr.nb - 1 - pr.fld0))) * (IL * IX * 8) + 16 * l16;
        UNROLL for (int a = 0; a < 4; ++a) {
            const int i_ = rl + 4 * (a & 1);
            const int vo = vl + ((a >> 1) ? (CP - 1 - i_) : i_) * (IX * 8);
            const int so = ((a >> 1) ? IL - CP - CP * c : CP * c) * (IX * 8);
            UNROLL for (int qq = 0; qq < 6; ++qq) pre[6 * a + qq] = t63_bload2<0>(rs, vo + 256 * qq, so);
        }
    }
    {   // what no Legendre slot writes is structurally zero (l > trunc+1, row nx): this wave's field, rows n = c, c + 6, ... (lane =
        // m'), as the fused walk's FFT waves do it in their phase B
        constexpr int NZ = (NX + NCH - 1) / NCH;
        int zf[NZ];
        UNROLL for (int j = 0; j < NZ; ++j) zf[j] = zfirst[min(c + NCH * j, NX - 1)];
        // (hazard-safe stores: here the compiler had put the next address computation into a data register of the last
        // store, one wait state behind it -- tools/scan_store_hazard.py, DESIGN 4.3)
        const bool vds = T63_SU(pr.op) == T63_OP_VDS;
        const spdy_u4 rz = t63_rsrc_u4((vds && fw ? b.vds_dst2 : pr.dst) + pr.fld0 * (long)(2 * NX * MX));
        const int vz = (vds ? 0 : fw) * (NX * MX * 16) + 16 * lane;
        const bool have = vds || pr.fld0 + fw < pr.nb;
        UNROLL for (int j = 0; j < NZ; ++j) {
            const bool wr = have && c + NCH * j < NX && lane >= zf[j];
            t63_bstore2_safe<false, T63_STAGED_WT != 0>(rz, wr ? vz + j * (NCH * MX * 16) : (int)0x80000000, c * (MX * 16), make_double2(0.0, 0.0));
        }
    }
    double *wbuf = lds + wi * WROWS;
    {   // own grid rows into their LDS slots
        double *gdst = wbuf + rl * RS + 2 * l16;
        UNROLL for (int a = 0; a < 4; ++a) {
            double sc = 1.0;
            if (MODE == 1 && pr.scale) {
                const int i_ = rl + 4 * (a & 1);
                sc = pr.scale[(a >> 1) ? IL - 1 - CP * c - i_ : CP * c + i_];
            }
            UNROLL for (int qq = 0; qq < 6; ++qq) {
                double2 v = pre[6 * a + qq];
                if (MODE == 1) { v.x *= sc; v.y *= sc; }
                double *d = gdst + 4 * a * RS + 32 * qq;
                d[0] = v.x;
                d[1] = v.y;
            }
        }
    }
    const int r = lane & 15, h = lane >> 4;
    double *z = wbuf + r * RS;
    double y[48];
    {
        double x[48];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the wave's own row writes have landed
        UNROLL for (int i = 0; i < 48; ++i) x[i] = z[4 * i + h];
        sub48_forward_c(c_fft192, x, y);
    }
    t63_twiddle_column_fwd(y, tw + 48 * h);
    t63_redistribute_inplace<0, 12>(y);
    t63_radf4_last_raw(y, z, c_fft192.hsqt2, h);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              // the rows are complete (four lanes wrote each)
    // Fourier rows out: slots z[0 .. 2 mx) of every row (what the contraction reads), 1 KB per row and store
    double2 *dst = reinterpret_cast<double2 *>(p.rows_ws) + ((((long)P * NCH + c) * 2 + fw) * 16) * MX + lane;
    UNROLL for (int rr = 0; rr < 16; ++rr) {
        const double *zr = wbuf + rr * RS + 2 * lane;
        if (T63_STAGED_WT) store2_wt(&dst[rr * MX], make_double2(zr[0], zr[1]));
        else dst[rr * MX] = make_double2(zr[0], zr[1]);
    }
}

// Legendre wave W of the fused walk, restricted to quad position I of its schedule, with its B operands from the row workspace.
// NP pairs per workgroup (P0 .. P0 + NP - 1; a pair index past the batch's end repeats the last pair: same values to the same
// addresses): every operand fragment then feeds NP pairs' matrix instructions -- above ~40 pairs the launch is bound by the
// operand image streaming out of L2 (0.9 MB per pair), not by latency.  PF: fragments in flight (the position's slots of one
// chunk, or half of them when two pairs' accumulators and coefficients need the registers).
template <int W, int I, int NP, bool VDS = false>
__device__ __forceinline__ void t63_dir_contract_rows(const DevPlan &p, const T63Batch &b, long P0, int lane)
{
    using namespace t63;
    constexpr int q = wave_quad(W, I);
    constexpr int S0 = slot_of(true, W, I, 0, 0), NS = slot_of(true, W, I + 1, 0, 0) - S0;     // this position's slots
    constexpr int PF = NP == 1 ? NS : (NS + 1) / 2, NSP = (NS + PF - 1) / PF * PF;
    const int blk = (lane >> 2) & 3, col = lane & 3, drow = lane >> 4, part = col & 1, f = col >> 1;
    const int m = 4 * q + blk, zi = m == 0 ? 0 : 2 * m + part - 1;
    const double live = (m == 0 && part == 1) ? 0.0 : c_fft192.scale;
    // the lane's Fourier coefficients of all six chunks (rows lat and IL-1-lat of field f, latitudes 4 ks + drow of the chunk)
    double lo[NP][NCH][2], hi[NP][NCH][2];
    UNROLL for (int np = 0; np < NP; ++np) {
        const long P = min(P0 + np, (long)b.npairs - 1);
        const double *rows = p.rows_ws + (P * NCH * 32 + f * 16) * (long)(2 * MX) + zi;
        UNROLL for (int c = 0; c < NCH; ++c)
            UNROLL for (int ks = 0; ks < 2; ++ks) {
                lo[np][c][ks] = rows[(c * 32 + 4 * ks + drow) * (2 * MX)];
                hi[np][c][ks] = rows[(c * 32 + 8 + 4 * ks + drow) * (2 * MX)];
            }
    }
    const double2 *aimg = reinterpret_cast<const double2 *>(p.img_g2s63);
    double2 ring[PF];
    UNROLL for (int s = 0; s < PF; ++s) ring[s] = T63_AFRAG_FLAT(aimg, afrag(W, S0, 0), s, lane);
    double acc[NP][MAXS];
    UNROLL for (int np = 0; np < NP; ++np)
        UNROLL for (int s = 0; s < MAXS; ++s) acc[np][s] = 0.0;
    UNROLL for (int c = 0; c < NCH; ++c) {
        double be[NP][2], bo[NP][2];
        UNROLL for (int np = 0; np < NP; ++np)
            UNROLL for (int ks = 0; ks < 2; ++ks) {
                be[np][ks] = (hi[np][c][ks] + lo[np][c][ks]) * live;
                bo[np][ks] = (hi[np][c][ks] - lo[np][c][ks]) * live;
            }
        UNROLL for (int par = 0; par < 2; ++par) {
            UNROLL for (int g = 0; g < 9; ++g) {
                if (g < ngrp(true, q, par)) {
                    const int s = slot_of(true, W, I, par, g), r = s - S0;
                    const double2 a = ring[r % PF];
                    // the fragment PF slots on: of this chunk, or (ring positions counted over NSP = NS rounded up to a multiple of
                    // PF, as in t63_dir_contract) of the next one
                    if (r + PF < NS) ring[r % PF] = T63_AFRAG_FLAT(aimg, afrag(W, S0, c), r + PF, lane);
                    else if (r + PF >= NSP && c + 1 < NCH) ring[r % PF] = T63_AFRAG_FLAT(aimg, afrag(W, S0, c + 1), r + PF - NSP, lane);
                    UNROLL for (int np = 0; np < NP; ++np) {
                        acc[np][s] = MFMA4(a.x, par ? bo[np][0] : be[np][0], acc[np][s]);
                        acc[np][s] = MFMA4(a.y, par ? bo[np][1] : be[np][1], acc[np][s]);
                    }
                }
            }
        }
        // ring positions whose turn falls on a virtual slot NS <= r < NSP
        UNROLL for (int r = NS; r < NSP; ++r)
            if (r + PF >= NSP && c + 1 < NCH) ring[r % PF] = T63_AFRAG_FLAT(aimg, afrag(W, S0, c + 1), r + PF - NSP, lane);
    }
    UNROLL for (int np = 0; np < NP; ++np) {
        const T63PairRef pr = t63_pair(b, min(P0 + np, (long)b.npairs - 1));
        // (the staged form writes its spectra through: T63_STAGED_WT)
        if (VDS && T63_SU(pr.op) == T63_OP_VDS) t63_dir_writeout_vds<W, I>(p, pr, b.vds_dst2, lane, acc[np]);
        else t63_dir_writeout<W, I, I + 1, T63_STAGED_WT ? 17 : 0>(pr.dst, pr.fld0, (int)min(2L, (long)pr.nb - pr.fld0), lane, acc[np]);
    }
}

// VDS: the launch carries vdspec pairs (T63_OP_VDS segments); launches without them run the VDS = false instantiation, whose code is
// what it was before the fold
template <int NP, bool VDS = false>
__global__ __launch_bounds__(256) void g2s_contract_t63_kernel(DevPlan p, T63Batch b)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = (int)blockIdx.x & 3;
    const long P = (long)(blockIdx.x >> 2) * NP;
#define T63_CR(W_, I_) if (w == W_ && i == I_) t63_dir_contract_rows<W_, I_, NP, VDS>(p, b, P, lane)
    T63_CR(0, 0); T63_CR(0, 1); T63_CR(0, 2); T63_CR(0, 3);
    T63_CR(1, 0); T63_CR(1, 1); T63_CR(1, 2); T63_CR(1, 3);
    T63_CR(2, 0); T63_CR(2, 1); T63_CR(2, 2); T63_CR(2, 3);
    T63_CR(3, 0); T63_CR(3, 1); T63_CR(3, 2); T63_CR(3, 3);
#undef T63_CR
}

// SPLIT (batches of at most half as many pairs as CUs): two workgroups per pair.  Both run the pair's FFTs; workgroup 2v
// contracts the zonal-wavenumber quads at positions 0, 1 of every Legendre wave's schedule, workgroup 2v+1 those at 2, 3
// (quads q and 15-q are one balanced position pair), so each streams half of the operand image -- the stream through ONE
// CU is what a lone pair's 37 us are made of.  Every coefficient is still summed by the same instructions in the same order:
// bit-identical to the unsplit launch.
template <int MODE, bool STREAM, bool SPLIT = false>
__global__ __launch_bounds__(t63::NTHR) void g2s_fused_t63_kernel(DevPlan p, T63Batch b)
{
    using namespace t63;
    T63_KARG_CONTRACT(b);                                          // (T63_PAIR_FFT below reads `b` from the kernel-argument segment)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *tw = lds + NBUF * BUF;
    int *zfirst = reinterpret_cast<int *>(tw + TW + IL);           // [NX] first structurally-zero m' of every spectral row
    const int tid = threadIdx.x, lane = tid & 63, w = T63_WAVE_ID(tid);
    const int npairs = b.npairs;
    const int bid = SPLIT ? (int)blockIdx.x >> 1 : (int)blockIdx.x, gdim = SPLIT ? (int)gridDim.x >> 1 : (int)gridDim.x;
    const int half = SPLIT ? (int)blockIdx.x & 1 : 0;
    const int kp = (bid < npairs) ? (npairs - 1 - bid) / gdim + 1 : 0;                                       // pairs of this workgroup
    const int T = kp * NCH;                                                                                  // chunk steps

    // A workgroup's waves w and w+4 share a SIMD.  Since the end of round 3 every SIMD hosts one Legendre wave (hardware waves
    // 0-3) and one FFT wave (4-7): T63_IS_FFT_D above.  (Until then the Legendre waves had the SIMDs of waves {0,4}, {1,5} and the
    // FFT waves those of {2,6}, {3,7}.)
    const bool is_fft = T63_IS_FFT_D(w);
    const int wi = T63_ROLE_INDEX_D(w);                            // index within the role, 0..3
    if (is_fft) {
        // one Legendre and one FFT wave per SIMD: the FFT wave -- a dependent chain of vector instructions -- wins the issue
        // arbitration against the Legendre wave, which waits on its operand stream most of the time anyway (B = 1536: 81.7-82.4 ->
        // 80.7-81.0 us; priority 3 the same, 1 nothing; with it the mixed placement also pays in the split form of model-sized
        // batches: captured T63 L8 step 66.3 -> 65.4 us, L16 81.1 -> 80.9 us -- without it the split form lost 0.8 us mixed)
        __builtin_amdgcn_s_setprio(2);
        // =================================================================== FFT waves: two groups of two (wave = one field
        // of the pair); group gp takes the chunks t = gp, gp+2, ... and spends TWO steps on each, so that one group's phase A
        // runs beside the other's phase B.  What each phase holds is balanced by measured length (a phase is a latency
        // chain of one wave, not a throughput: at 146 fields on an idle chip phase A took 8.4 k ticks and phase B 3.1 k, and
        // the step is the longer of the two):
        //   A: rows of chunk t registers -> LDS -> registers (transposition), first part of the prefetch of chunk t+2,
        //      48-point sub-transforms, twiddle factors of the ido = 48 stage (by column), lane transposes rounds [0, RA)
        //   B: zero fill of the chunk's share of the spectra, transposes [RA, 12), rest of the prefetch, the stage's butterflies
        const int fw = wi & 1, gp = wi >> 1;
        const int l16 = lane & 15, rl = lane >> 4;
        for (int e = 64 * wi + lane; e < TW; e += 64 * NFW) tw[e] = e < 48 ? (double)((e & 1) ^ 1) : c_fft192.first[e - 48];
        constexpr int NEARLY = T63_NEARLY;                         // row groups (of 4 x 4 rows) fetched in phase A, two steps ahead
        constexpr int RA = T63_RA;                                 // transpose rounds done in phase A
        double2 pre[24];
        double y[48];                                              // the sub-transforms live across the step barrier
        // lane (rl, l16) moves pieces l16 + 16 qq (qq < 6) of rows r16 = rl + 4a (a < 4) of its 16 rows:
        // r16 < 8: latitude 8c + r16; r16 >= 8: latitude IL-1 - 8c - (r16-8).  Buffer form: base = the pair's first field
        // (scalar); lane offset = field within the pair (the absent second field of an odd segment reads the first again), row
        // within the chunk half, 16-byte piece; scalar offset = the chunk's first row of that half
#define T63_PREFETCH(t_, A0, A1)                                                                              \
    do {                                                                                                      \
        const int tc_ = T63_SU(min((int)(t_), T - 1)), k_ = tc_ / NCH, c_ = tc_ - k_ * NCH;                   \
        const T63PairRef pr_ = T63_PAIR_FFT(bid + k_ * gdim);                                     \
        const __amdgpu_buffer_rsrc_t rs_ = t63_rsrc(pr_.src + pr_.fld0 * (long)(IL * IX));                    \
        const int vl_ = min(fw, (int)(pr_.nb - 1 - pr_.fld0)) * (IL * IX * 8) + 16 * l16;                     \
        UNROLL for (int a = (A0); a < (A1); ++a) {                                                            \
            const int i_ = rl + 4 * (a & 1);                                                                  \
            const int vo_ = vl_ + ((a >> 1) ? (CP - 1 - i_) : i_) * (IX * 8);                                 \
            const int so_ = ((a >> 1) ? IL - CP - CP * c_ : CP * c_) * (IX * 8);                              \
            UNROLL for (int qq = 0; qq < 6; ++qq) pre[6 * a + qq] = t63_bload2<STREAM ? 2 : 0>(rs_, vo_ + 256 * qq, so_); \
        }                                                                                                     \
    } while (0)
        T63_PREFETCH(gp, 0, 4);
        lds_barrier();                                             // (T) twiddles ready (and pairs the Legendre waves' first barrier)
        for (int u = 0; u <= T + 1; ++u) {
            T63_MARK(0, u, 0);
            const int t = ((u & 1) == gp) ? u : u - 1;             // the chunk this group works on in step u
            const bool phase_a = (u & 1) == gp;
            double *buf = lds + (t % NBUF) * BUF;
            int lane_s = lane;
            asm volatile("" : "+v"(lane_s));                       // opaque per step: LDS addresses are recomputed, not kept in
                                                                   // registers that spill (a scratch reload waits for the HBM prefetch)
            const int r = lane_s & 15, h = lane_s >> 4;
            double *z = buf + (fw * 16 + r) * RS;
            if (phase_a && t < T) {
                const int ts = T63_SU(t), c = ts % NCH;
                {   // own grid rows into their LDS slots
                    double *gdst = buf + (fw * 16 + rl) * RS + 2 * l16;
                    const double *scale = nullptr;
                    if (MODE == 1) scale = T63_PAIR_FFT(bid + (ts / NCH) * gdim).scale;
                    UNROLL for (int a = 0; a < 4; ++a) {
                        double sc = 1.0;
                        if (MODE == 1 && scale) {
                            const int i_ = rl + 4 * (a & 1);
                            sc = scale[(a >> 1) ? IL - 1 - CP * c - i_ : CP * c + i_];
                        }
                        UNROLL for (int qq = 0; qq < 6; ++qq) {
                            double2 v = pre[6 * a + qq];
                            if (MODE == 1) { v.x *= sc; v.y *= sc; }
                            double *d = gdst + 4 * a * RS + 32 * qq;
                            d[0] = v.x;
                            d[1] = v.y;
                        }
                    }
                }
                T63_MARK(0, u, 1);
                T63_PREFETCH(t + 2, 0, NEARLY);                    // this group's next chunk, two steps ahead
                // ---- 16 row FFTs (fourier.f90:56-82): lanes r, r+16, r+32, r+48 own the four decimated 48-point
                // sub-transforms of row r
                int coff = 0;
                asm volatile("" : "+s"(coff));                     // opaque per step: keeps the constant loads in the loop
                const FftConstants &cc = *reinterpret_cast<const FftConstants *>(reinterpret_cast<const char *>(&c_fft192) + coff);
                {
                    double x[48];
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the wave's own row writes have landed
                    UNROLL for (int i = 0; i < 48; ++i) x[i] = z[4 * i + h];
                    sub48_forward_c(cc, x, y);
                }
                T63_MARK(0, u, 2);
                t63_twiddle_column_fwd(y, tw + 48 * h);            // this lane's column: factors at constant offsets, one batch
                t63_redistribute_inplace<0, RA>(y);
                T63_MARK(0, u, 6);
            } else if (!phase_a && t >= 0 && t < T) {
                const int ts = T63_SU(t), c = ts % NCH;
                const T63PairRef pr = T63_PAIR_FFT(bid + (ts / NCH) * gdim);
                int coff = 0;
                asm volatile("" : "+s"(coff));
                const FftConstants &cc = *reinterpret_cast<const FftConstants *>(reinterpret_cast<const char *>(&c_fft192) + coff);
                T63_MARK(0, u, 1);
                {   // what no Legendre slot writes is structurally zero (l > trunc+1, row nx): this wave's field, rows
                    // n = c, c + 6, ... of it per chunk c (lane = m'), so the stores ride along with the six steps of the pair.
                    // Branch-free: a lane that has nothing to write gets an offset beyond the descriptor's range and the
                    // hardware drops its store.
                    constexpr int NZ = (NX + NCH - 1) / NCH;
                    int zf[NZ];
                    UNROLL for (int j = 0; j < NZ; ++j) zf[j] = zfirst[min(c + NCH * j, NX - 1)];
                    const __amdgpu_buffer_rsrc_t rz = t63_rsrc(pr.dst + pr.fld0 * (long)(2 * NX * MX));
                    const int vz = fw * (NX * MX * 16) + 16 * lane_s;
                    const bool have = pr.fld0 + fw < pr.nb && half == 0;        // (split launch: the first workgroup of the pair)
                    UNROLL for (int j = 0; j < NZ; ++j) {
                        const bool wr = have && c + NCH * j < NX && lane_s >= zf[j];
                        t63_bstore2<T63_ZERO_AUX>(rz, wr ? vz + j * (NCH * MX * 16) : (int)0x80000000, c * (MX * 16), make_double2(0.0, 0.0));
                    }
                }
                t63_redistribute_inplace<RA, 12>(y);
                T63_PREFETCH(t + 2, NEARLY, 4);                    // the rest of the next chunk (after the transposes: registers)
                T63_MARK(0, u, 5);
                t63_radf4_last_raw(y, z, cc.hsqt2, h);
                T63_MARK(0, u, 3);
            }
            T63_MARK(0, u, 4);
            lds_barrier();
        }
#undef T63_PREFETCH
    } else {
        // =================================================================== Legendre waves: one straight-line loop per wave
        // variant (the slot schedule is compile-time per wave; dispatching once here instead of at every call keeps the
        // register arrays out of four-way merges)
        for (int e = 64 * wi + lane; e < NX; e += 64 * NLW) zfirst[e] = first_unwritten_m(e);
        if (!SPLIT) {
            if (wi == 0) t63_dir_legendre_wave<0>(p, b, lds, bid, gdim, T, lane);
            else if (wi == 1) t63_dir_legendre_wave<1>(p, b, lds, bid, gdim, T, lane);
            else if (wi == 2) t63_dir_legendre_wave<2>(p, b, lds, bid, gdim, T, lane);
            else t63_dir_legendre_wave<3>(p, b, lds, bid, gdim, T, lane);
        } else if (half == 0) {
            if (wi == 0) t63_dir_legendre_wave<0, 0, 2>(p, b, lds, bid, gdim, T, lane);
            else if (wi == 1) t63_dir_legendre_wave<1, 0, 2>(p, b, lds, bid, gdim, T, lane);
            else if (wi == 2) t63_dir_legendre_wave<2, 0, 2>(p, b, lds, bid, gdim, T, lane);
            else t63_dir_legendre_wave<3, 0, 2>(p, b, lds, bid, gdim, T, lane);
        } else {
            if (wi == 0) t63_dir_legendre_wave<0, 2, 4>(p, b, lds, bid, gdim, T, lane);
            else if (wi == 1) t63_dir_legendre_wave<1, 2, 4>(p, b, lds, bid, gdim, T, lane);
            else if (wi == 2) t63_dir_legendre_wave<2, 2, 4>(p, b, lds, bid, gdim, T, lane);
            else t63_dir_legendre_wave<3, 2, 4>(p, b, lds, bid, gdim, T, lane);
        }
    }
}

// ------------------------------------------------------------------------------------------
// spec_to_grid, fused, T63 (spectral.f90:98-110).  grid[nb][96][192] <- spec[nb][65][64] complex
//   The pair's spectra are the MFMA B operands: 38 doubles per lane, loaded once per pair straight from HBM (64-byte
//   runs: 4 m' x (re, im) per 16-lane group and field) and kept in VGPRs for the pair's six chunks.
//   step u: Legendre waves synthesise chunk u (32 Fourier rows) into buffer u%3; FFT group (u-1)%2 starts chunk u-1
//   (A: ido = 48 radix-4 stage straight from the LDS rows, redistribution), the other group finishes chunk u-2
//   (B: 48-point sub-transforms, transposition through the rows' own LDS slots, coalesced grid stores).
// ------------------------------------------------------------------------------------------
template <int W>
__device__ __forceinline__ void t63_inv_load_b(const double *__restrict__ spec, long fld0, int nfld, int lane, double (&bop)[t63::MAXS])
{
    using namespace t63;
    asm volatile("" : "+v"(lane));
    const int blk = (lane >> 2) & 3, col = lane & 3, kk = lane >> 4, part = col & 1, f = col >> 1;
    UNROLL for (int i = 0; i < 4; ++i) {
        const int q = wave_quad(W, i), m = 4 * q + blk;
        UNROLL for (int par = 0; par < 2; ++par) {
            UNROLL for (int g = 0; g < 9; ++g) {
                if (g < ngrp(false, q, par)) {
                    const int s = slot_of(false, W, i, par, g);
                    const int n = 2 * (4 * g + kk) + par;
                    double v = 0.0;
                    if (n < NX && m + n <= TRUNC + 1 && f < nfld) v = spec[2 * (((fld0 + f) * NX + n) * MX + m) + part];
                    bop[s] = v;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// DERIVED pairs (row f1 at T63, round 6): the segment's spectra are uvspec's U or V (spectral.f90:173-196) or grad's d/dlambda
// or d/dmu (spectral.f90:124-144) of the arrays the segment names -- evaluated by the workgroup that transforms them, in front
// of its first synthesis: no operator launch in front of the transform, no U / V spectra in HBM.  One form for the four
// operators (segment src = A, scale = Z):
//     x(m, n) = (cm A(m, n-1) + cp A(m, n+1)) + (0, 1) cx Z(m, n)
//   U : A = vor, Z = div, cm =  uvdym, cp = -uvdyp, cx = uvdx        V : A = div, Z = vor, cm = -uvdym, cp = uvdyp, cx = uvdx
//   d/dmu : A = psi, cm = -gradym, cp = gradyp, no Z term            d/dlambda : Z = psi, cx = gradx, no A terms
// with the reference's edge rows: no n-1 term in row 1, and in row nx neither the n+1 nor (uvspec) the Z term.
// Two forms were built and measured first (tools/experiments/README.md): round 3's, seven scattered loads per coefficient in
// the Legendre waves' operand loader (500 registers in flight: shelved), and round 6's first, the stencil's neighbours by lane
// exchange inside the Legendre waves (correct, spill-free, three loads per coefficient -- and 8 us per derived workgroup: four
// copies of a 20 KB straight-line loader that runs once is an instruction-cache miss per line, tools/phase_trace_t63_derive.py).
// This form:
//   * ALL EIGHT waves of the workgroup take part (the FFT waves have nothing to do before the first synthesis), with ONE copy
//     of the code: waves 0-3 the pair's first field, 4-7 its second; a wave's work items are "packed rows" -- row n of the live
//     triangle has 65 - n coefficients, so rows r and 66 - r share the 64 lanes (rows 0, 1 and 33 stand alone): 34 items per
//     field, at most nine per wave, every lane of every item a live coefficient (m, n) in storage order -- whole-line loads;
//   * per item six buffer loads (A(n-1), A(n+1), Z(n): 16 bytes; the three table entries: 8) off two lane offsets and
//     immediates, all nine items in flight together: ONE memory round trip.  The descriptors of A and Z span exactly one
//     field, so rows -1 and nx read as zero (the hardware's range check) where the reference has no such term;
//   * the results go to LDS in B-OPERAND order (chunk buffers 1 and 2 are idle until the second step; slot stride 68 doubles)
//     with one 16-byte write per coefficient; behind the workgroup's first barrier the Legendre waves pick their 38 operands
//     up with compile-time offsets.
// ------------------------------------------------------------------------------------------
namespace t63 {
constexpr int STAGE_STRIDE = 68;                               // doubles per staged slot (64 lanes + 4: spreads the scatter over the banks)
static_assert(NLW * MAXS * STAGE_STRIDE <= 2 * BUF, "the staged operands fit chunk buffers 1 and 2");
// first staged slot (wave * MAXS + slot) of (quad q, parity): what the lane that computed (m, n) needs to find its B-operand cell
constexpr int stage_slot0(int q, int par)
{
    const int w = q < 8 ? q / 2 : (15 - q) % 2 == 0 ? (15 - q) / 2 : (14 - q) / 2;
    const int i = q < 8 ? (q % 2 == 0 ? 0 : 2) : (15 - q) % 2 == 0 ? 1 : 3;
    return w * MAXS + slot_of(false, w, i, par, 0);
}
static_assert(wave_quad(1, 0) == 2 && stage_slot0(2, 0) == MAXS && stage_slot0(15, 1) == slot_of(false, 0, 1, 1, 0) && stage_slot0(5, 0) == 2 * MAXS + slot_of(false, 2, 2, 0, 0)
              && stage_slot0(8, 0) == 3 * MAXS + slot_of(false, 3, 3, 0, 0), "inverse of wave_quad");
}  // namespace t63
__device__ __forceinline__ __amdgpu_buffer_rsrc_t t63_rsrc_n(const void *base, unsigned bytes)    // (wave-uniform base, as t63_rsrc)
{
    const unsigned long long a = reinterpret_cast<unsigned long long>(base);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((unsigned long long)hi << 32) | lo), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ void t63_derive_to_lds(const DevPlan &p, const T63PairRef &pr, int op, double *stage, int w, int lane)
{
    using namespace t63;
    const int f = T63_SU(w >> 2), wj = T63_SU(w & 3);
    if (pr.fld0 + f >= pr.nb) return;                                       // (the absent second field of an odd segment)
    const bool gr = op >= T63_OP_GX, vform = op == T63_OP_V || op == T63_OP_GY;
    const bool use_a = op != T63_OP_GX, use_z = op != T63_OP_GY;
    const double sg = vform ? -1.0 : 1.0;
    constexpr unsigned FB = NX * MX * 16;                                   // bytes of one field's spectrum
    const __amdgpu_buffer_rsrc_t rA = t63_rsrc_n(pr.src + (pr.fld0 + f) * (long)(2 * NX * MX), FB);
    const __amdgpu_buffer_rsrc_t rZ = t63_rsrc_n(pr.scale + (pr.fld0 + f) * (long)(2 * NX * MX), FB);
    const __amdgpu_buffer_rsrc_t rTm = t63_rsrc_n(gr ? p.gradym : p.uvdym, FB / 2), rTp = t63_rsrc_n(gr ? p.gradyp : p.uvdyp, FB / 2);
    const __amdgpu_buffer_rsrc_t rTx = t63_rsrc_n(gr ? p.gradx_e : p.uvdx, FB / 2);
    // lanes 0 .. 31 hold the slot table entry of (quad lane >> 1, parity lane & 1); looked up per item with one ds_bpermute
    const int slot_entry = stage_slot0((lane >> 1) & 15, lane & 1);
    constexpr int NIT = 9, NPACK = 34;                                      // items per wave, packed rows per field
    double2 a1[NIT], a2[NIT], zz[NIT];
    double tm[NIT], tp[NIT], tx[NIT];
    UNROLL for (int j = 0; j < NIT; ++j) {
        const int r = min(NIT * wj + j, NPACK - 1);                         // (wave 3's last two items repeat row 33: same values, same cells)
        const int thr = r < 2 ? 64 : 65 - r, in_a = lane < thr;
        const int n = in_a ? r : 66 - r, m = in_a ? lane : lane - thr;
        const int vc = (n * MX + m) * 16;
        a1[j] = t63_bload2<0>(rA, vc - MX * 16, 0);                         // row -1: out of range, reads as zero
        a2[j] = t63_bload2<0>(rA, vc + MX * 16, 0);                         // row nx: out of range, reads as zero
        zz[j] = t63_bload2<0>(rZ, vc, 0);
        tm[j] = t63_bload1<0>(rTm, vc >> 1, 0);
        tp[j] = t63_bload1<0>(rTp, vc >> 1, 0);
        tx[j] = t63_bload1<0>(rTx, vc >> 1, 0);
    }
    UNROLL for (int j = 0; j < NIT; ++j) {
        const int r = min(NIT * wj + j, NPACK - 1);
        const int thr = r < 2 ? 64 : 65 - r, in_a = lane < thr;
        const int n = in_a ? r : 66 - r, m = in_a ? lane : lane - thr;
        const double cm = sg * tm[j], cp = -sg * tp[j];
        double cx = tx[j];
        if (!gr && n == NX - 1) cx = 0.0;                                   // uvspec's row nx has no Z term
        const double zr = cx * zz[j].x, zim = cx * zz[j].y;                 // real x complex ...
        double ire = zr * 0.0 - zim, iim = zr + zim * 0.0;                  // ... then the full (0, 1) multiply
        double nre = cm * a1[j].x + cp * a2[j].x, nim = cm * a1[j].y + cp * a2[j].y;
        if (!use_a) { nre = 0.0; nim = 0.0; }
        if (!use_z) { ire = 0.0; iim = 0.0; }
        const int q = m >> 2, blk = m & 3, par = n & 1, g = n >> 3, kk = (n >> 1) & 3;
        const int slot = __shfl(slot_entry, 2 * q + par) + g;
        *reinterpret_cast<double2 *>(stage + slot * STAGE_STRIDE + kk * 16 + blk * 4 + f * 2) = make_double2(nre + ire, nim + iim);
    }
}
// the Legendre wave's 38 operands out of the staged image (behind the barrier that follows t63_derive_to_lds)
template <int W>
__device__ __forceinline__ void t63_inv_load_b_staged(const double *stage, int nfld, int lane, double (&bop)[t63::MAXS])
{
    using namespace t63;
    asm volatile("" : "+v"(lane));
    const int blk = (lane >> 2) & 3, col = lane & 3, kk = lane >> 4, f = col >> 1;
    UNROLL for (int i = 0; i < 4; ++i) {
        const int q = wave_quad(W, i), m = 4 * q + blk;
        UNROLL for (int par = 0; par < 2; ++par)
            UNROLL for (int g = 0; g < 9; ++g)
                if (g < ngrp(false, q, par)) {
                    const int s = slot_of(false, W, i, par, g);
                    const int n = 2 * (4 * g + kk) + par;
                    const double v = stage[(W * MAXS + s) * STAGE_STRIDE + lane];
                    bop[s] = (n < NX && m + n <= TRUNC + 1 && f < nfld) ? v : 0.0;      // (cells no item wrote hold old rows)
                }
    }
}

template <int W>
__device__ __forceinline__ void t63_inv_load_b_any(const DevPlan &p, const T63PairRef &pr, int lane, double (&bop)[t63::MAXS])
{
    const int nfld = (int)max(0L, min(2L, (long)pr.nb - pr.fld0));
    (void)p;
    t63_inv_load_b<W>(pr.src, pr.fld0, nfld, lane, bop);
}

template <int W>
__device__ __forceinline__ void t63_inv_synth(double *buf, int c, int cnext, const double2 *__restrict__ aimg, int lane,
                                              double (&bop)[t63::MAXS], double2 (&ring)[T63_PF_I])
{
    using namespace t63;
    asm volatile("" : "+v"(lane));
    const int blk = (lane >> 2) & 3, col = lane & 3, drow = lane >> 4, part = col & 1, f = col >> 1;
    const int fc = afrag(W, 0, c), fn = afrag(W, 0, cnext);
    constexpr int NS = nslots(false, W), PF = T63_PF_I, NSP = (NS + PF - 1) / PF * PF;
    UNROLL for (int i = 0; i < 4; ++i) {
        const int q = wave_quad(W, i), m = 4 * q + blk;
        double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};                       // [parity][latitude group of 4]
        UNROLL for (int par = 0; par < 2; ++par) {
            UNROLL for (int g = 0; g < 9; ++g) {
                if (g < ngrp(false, q, par)) {
                    const int s = slot_of(false, W, i, par, g);
                    const double2 a = ring[s % PF];
                    if (s + PF < NS) ring[s % PF] = T63_AFRAG_I(aimg, fc, s + PF, lane);
                    else if (s + PF >= NSP) ring[s % PF] = T63_AFRAG_I(aimg, fn, s + PF - NSP, lane);
                    acc[par][0] = MFMA4(a.x, bop[s], acc[par][0]);
                    acc[par][1] = MFMA4(a.y, bop[s], acc[par][1]);
                }
            }
        }
        // rows: lat -> even - odd, IL-1-lat -> even + odd (legendre.f90:106-109); column 2m'+part of the Fourier row
        double *fb = buf + f * 16 * RS + 2 * m + part;
        UNROLL for (int lg = 0; lg < 2; ++lg) {
            const int il = 4 * lg + drow;
            fb[il * RS] = acc[0][lg] - acc[1][lg];
            fb[(8 + il) * RS] = acc[0][lg] + acc[1][lg];
        }
    }
    UNROLL for (int s = NS; s < NSP; ++s)
        if (s + PF >= NSP) ring[s % PF] = T63_AFRAG_I(aimg, fn, s + PF - NSP, lane);
}

// fftpack radb4 (ido = 48, l1 = 1) for this lane's positions, straight from the Fourier row in LDS, WITHOUT its twiddle
// factors: v[4 rho + j] = column j's (cr, ci) sums at this lane's position rho.  The factors
// multiply one column's values only (fftpack.f90:394-400), so they are applied after the lane transposes, by the lane that owns
// the column (t63_twiddle_column): its 23 factor pairs sit at constant offsets from one per-lane base and are fetched in one
// batch -- in the position-owner form above every butterfly waited for its own three LDS reads (21 dependent round trips).
__device__ __forceinline__ void t63_radb4_first_raw(const double *rowp, double sqrt2, int h, double (&v)[48])
{
    constexpr int LASTF = 2 * t63::MX - 2;
    // fvar[i] = F[i+1] for 1 <= i <= LASTF, zero beyond (fourier.f90:34-41).  Every read is UNCONDITIONAL (the row slot has 193
    // doubles, so any index is inside it) and the zero is a select afterwards: a read guarded by a lane-dependent condition is a
    // branch around a load, i.e. one dependent LDS round trip per value.
    auto fv = [&](int i) -> double { return rowp[i + 1]; };                      /* 1 <= i <= LASTF by construction */
    auto fz = [&](int i) -> double { const double x_ = rowp[i + 1]; return i <= LASTF ? x_ : 0.0; };
#define T63B_RAW(p_, q_, R0, R1)                                                                                  \
    do {                                                                                                          \
        const double c00 = fv(p_), c01 = fv((p_) + 1), c20 = fz(96 + (p_)), c21 = fz(96 + (p_) + 1);               \
        const double c10 = fv(48 + (q_)), c11 = fv(48 + (q_) + 1), c30 = 0.0, c31 = 0.0;  /* 144 + q > LASTF */     \
        const double ti1 = c01 + c31, ti2 = c01 - c31, ti3 = c21 - c11, tr4 = c21 + c11;                           \
        const double tr1 = c00 - c30, tr2 = c00 + c30, ti4 = c20 - c10, tr3 = c20 + c10;                           \
        v[4 * (R0)] = tr2 + tr3;                                                                                   \
        v[4 * (R1)] = ti2 + ti3;                                                                                   \
        v[4 * (R0) + 1] = tr1 - tr4; v[4 * (R1) + 1] = ti1 + ti4;                                                  \
        v[4 * (R0) + 2] = tr2 - tr3; v[4 * (R1) + 2] = ti2 - ti3;                                                  \
        v[4 * (R0) + 3] = tr1 + tr4; v[4 * (R1) + 3] = ti1 - ti4;                                                  \
    } while (0)
    if (h == 0) {
        {   // i = 0
            const double a00 = rowp[0], a473 = 0.0, a471 = fv(47 + 48), a02 = fv(96);
            const double tr1 = a00 - a473, tr2 = a00 + a473, tr3 = a471 + a471, tr4 = a02 + a02;
            v[0] = tr2 + tr3; v[1] = tr1 - tr4; v[2] = tr2 - tr3; v[3] = tr1 + tr4;
        }
        {   // i = 47
            const double b01 = fv(48), b03 = 0.0, b470 = fv(47), b472 = 0.0;
            const double ti1 = b01 + b03, ti2 = b03 - b01, tr1 = b470 - b472, tr2 = b470 + b472;
            v[4] = tr2 + tr2; v[5] = sqrt2 * (tr1 - ti1); v[6] = ti2 + ti2; v[7] = -sqrt2 * (tr1 + ti1);
        }
        T63B_RAW(23, 23, 2, 3);
    } else {
        const int p = 2 * h - 1, q = 46 - p;
        T63B_RAW(p, q, 0, 1);
        T63B_RAW(q, p, 2, 3);
    }
    UNROLL for (int g = 1; g < 3; ++g) {
        const int p = 2 * (h + 4 * g) - 1, q = 46 - p;
        T63B_RAW(p, q, 4 * g, 4 * g + 1);
        T63B_RAW(q, p, 4 * g + 2, 4 * g + 3);
    }
#undef T63B_RAW
}
// the factor pairs (wa(p-1), wa(p)), p = 1, 3, .., 45, of column h: twc = tw4 + 48 h (column 0: (1, 0) pairs)
__device__ __forceinline__ void t63_load_column_twiddles(const double *twc, double2 (&wq)[23])
{
    UNROLL for (int j = 0; j < 23; ++j) wq[j] = *reinterpret_cast<const double2 *>(twc + 2 * j);
}
// backward (radb4): x[p] = wr cr - wi ci, x[p+1] = wr ci + wi cr
__device__ __forceinline__ void t63_twiddle_column_bwd(double (&x)[48], const double2 (&wq)[23])
{
    UNROLL for (int j = 0; j < 23; ++j) {
        const double cr = x[2 * j + 1], ci = x[2 * j + 2];
        x[2 * j + 1] = wq[j].x * cr - wq[j].y * ci;
        x[2 * j + 2] = wq[j].x * ci + wq[j].y * cr;
    }
}

// inverse of t63_redistribute: in v[4 rho + j] = column j at this lane's position rho; out x[pos] = this lane's column
__device__ __forceinline__ void t63_gather_column(const double (&v)[48], double (&x)[48])
{
    UNROLL for (int rho = 0; rho < 12; ++rho) {
        double r0 = v[4 * rho], r1 = v[4 * rho + 1], r2 = v[4 * rho + 2], r3 = v[4 * rho + 3];
        t63_swap32(r0, r2);
        t63_swap32(r1, r3);
        t63_swap16(r0, r1);
        t63_swap16(r2, r3);
        x[t63_pos(0, rho)] = r0; x[t63_pos(1, rho)] = r1; x[t63_pos(2, rho)] = r2; x[t63_pos(3, rho)] = r3;
    }
}

template <int W, bool BYCHUNK, bool OPS>
__device__ __forceinline__ void t63_inv_legendre_wave(const DevPlan &p, const T63Batch &b, double *lds, const T63Walk<BYCHUNK> &wk, int lane, int w)
{
    using namespace t63;
    (void)w;
    const int T = wk.T;
    double bop[MAXS];
    const double2 *aimg = reinterpret_cast<const double2 *>(p.img_s2g63);
    double2 ring[T63_PF_I];
    T63_MARK(1, 23, 0);
    bool staged = false;
    int nfld0 = 0;
    if (T > 0) {
        const T63PairRef pr = t63_pair(b, wk.pair(0));
        nfld0 = (int)max(0L, min(2L, (long)pr.nb - pr.fld0));
        staged = OPS && T63_SU(pr.op) != T63_OP_NONE;          // (wave-uniform: a scalar branch)
        // (the operand ring requested in FRONT of the derivation: measured neutral -- 64.7 vs 64.5 us per T63 L16 step -- at 244
        // instead of 178 registers)
        if (staged) t63_derive_to_lds(p, pr, T63_SU(pr.op), lds + BUF, w, lane);
        else t63_inv_load_b_any<W>(p, pr, lane, bop);
    }
    T63_MARK(1, 23, 1);
    t63_ring_init<false, W, T63_PF_I>(aimg, T > 0 ? wk.chunk(0) : 0, lane, ring);
    lds_barrier();                                             // (T)
    if (OPS && staged) t63_inv_load_b_staged<W>(lds + BUF, nfld0, lane, bop);   // all eight waves' results are in place
    T63_MARK(1, 23, 2);
    for (int u = 0; u <= T + 2; ++u) {
        T63_MARK(1, u, 0);
        if (u < T) {
            // (throughput walk: the plain index arithmetic the compiler schedules without spills; by-chunk walk: items)
            const int c = BYCHUNK ? wk.chunk(u) : u % NCH;
            const int cn = BYCHUNK ? (u + 1 < T ? wk.chunk(u + 1) : 0) : (c + 1 == NCH ? 0 : c + 1);
            double *buf = lds + (u % NBUF) * BUF;
            // ONE synthesis body and ONE operand-load site per wave variant (every further copy of either inside this loop --
            // a refetch-inside-the-synthesis form, a second loader call -- made the register allocator spill thousands of
            // values around the 38 operands and the A ring).  The next pair's (item's) operands are loaded as one batch
            // behind the synthesis: they are younger than the ring entries the next step opens with, so only that step's
            // first matrix instruction waits for them.
            t63_inv_synth<W>(buf, c, cn, aimg, lane, bop, ring);
            if (u + 1 < T && (BYCHUNK ? wk.pair(u + 1) != wk.pair(u) : c == NCH - 1)) {     // (by-chunk: the next item may be of this pair)
                const T63PairRef pn = t63_pair(b, wk.pair(u + 1));
                t63_inv_load_b_any<W>(p, pn, lane, bop);                   // (derived pairs are never met mid-walk: T63Walk)
            }
            T63_MARK(1, u, 1);
        }
        T63_MARK(1, u, 4);
        lds_barrier();
    }
}

// OPS: some segment's spectra are derived on load (T63_OP_*); launches without such a segment run the OPS = false instantiation,
// whose code is what it was before the fold.
template <bool STREAM, bool BYCHUNK, bool OPS = false>
__global__ __launch_bounds__(t63::NTHR) void s2g_fused_t63_kernel(DevPlan p, T63Batch b)
{
    using namespace t63;
    T63_KARG_CONTRACT(b);                                          // (T63_PAIR_FFT below reads `b` from the kernel-argument segment)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *tw = lds + NBUF * BUF;
    const int tid = threadIdx.x, lane = tid & 63, w = T63_WAVE_ID(tid);
    const T63Walk<BYCHUNK> wk = t63_walk<BYCHUNK>(b);
    const int T = wk.T;
    // One Legendre and one FFT wave per SIMD with the FFT wave at priority 3, like the direct kernel (end of round 3, B = 1536:
    // 70.5-70.7 by SIMD -> 69.6 us; mixed without the priority 72.6-73.3, with priority 2 70.5; the by-chunk form of model-sized
    // batches gains with it inside the captured steps, see the direct kernel).  (T63_ROLE_BY_SIMD_I: the roles on separate SIMDs.)
    const bool is_fft = T63_IS_FFT_D(w);
    const int wi = T63_ROLE_INDEX_D(w);
    if (is_fft) {
        __builtin_amdgcn_s_setprio(3);
        // =================================================================== FFT waves
        const int fw = wi & 1, gp = wi >> 1;
        for (int e = 64 * wi + lane; e < TW; e += 64 * NFW) tw[e] = e < 48 ? (double)((e & 1) ^ 1) : c_fft192.first[e - 48];
        double *cg = tw + TW;                                      // 1 / cos(latitude) of every grid row (fourier.f90:47-51)
        for (int e = 64 * wi + lane; e < IL; e += 64 * NFW) cg[e] = p.cosgr[e];
        if (OPS && T > 0) {                                        // a derived pair: its spectra are computed by all eight waves
            const T63PairRef pr0 = T63_PAIR_FFT((int)wk.pair(0));
            if (pr0.op != T63_OP_NONE) t63_derive_to_lds(p, pr0, pr0.op, lds + BUF, w, lane);
        }
        double x[48];                                              // lives across the step barrier between phases A and B
        lds_barrier();                                             // (T)
        for (int u = 0; u <= T + 2; ++u) {
            const bool phase_a = ((u - 1) & 1) == gp;
            const int t = phase_a ? u - 1 : u - 2;
            int lane_s = lane;
            asm volatile("" : "+v"(lane_s));
            const int r = lane_s & 15, h = lane_s >> 4;
            double *buf = lds + ((t + NBUF) % NBUF) * BUF;
            double *z = buf + (fw * 16 + r) * RS;
            T63_MARK(1, u, 0);
            if (t >= 0 && t < T) {
                int coff = 0;
                asm volatile("" : "+s"(coff));
                const FftConstants &cc = *reinterpret_cast<const FftConstants *>(reinterpret_cast<const char *>(&c_fft192) + coff);
                if (phase_a) {
                    double v[48], xx[48];
                    double2 wq[23];
                    t63_radb4_first_raw(z, cc.sqrt2, h, v);
                    t63_load_column_twiddles(tw + 48 * h, wq);      // in flight during the lane transposes
                    T63_MARK(1, u, 1);
                    t63_gather_column(v, xx);
                    t63_twiddle_column_bwd(xx, wq);
                    T63_MARK(1, u, 2);
                    sub48_backward_c(cc, xx, x);
                    T63_MARK(1, u, 5);
                } else {
                    double (&y)[48] = x;
                    T63_MARK(1, u, 1);
                    // element tt of column h is grid point 4 tt + h: through the row's own (now dead) LDS slot, then coalesced
                    UNROLL for (int tt = 0; tt < 48; ++tt) z[4 * tt + h] = y[tt];
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    T63_MARK(1, u, 3);
                    const int ts = T63_SU(t), c = wk.chunk(ts);
                    const T63PairRef pr = T63_PAIR_FFT((int)wk.pair(ts));
                    const long fld = pr.fld0 + fw;
                    if (fld < pr.nb) {
                        // (the per-field kcos is a scalar load, the latitude factor an unconditional LDS read + select: a vector
                        // load under a lane-dependent condition makes the compiler wait vmcnt(0) -- i.e. for the previous row
                        // group's stores -- in front of every group of stores)
                        const int kc = pr.kcos ? pr.kcos[pr.fld0 + T63_SU(fw)] : pr.kcos_all;
                        const int l16 = lane_s & 15, rl = lane_s >> 4;
                        const double *src = buf + (fw * 16 + rl) * RS + 2 * l16;
                        // base = the pair's first field (scalar); lane offset = field within the pair, row within the chunk half, piece
                        const spdy_u4 rs_u4 = t63_rsrc_u4(pr.dst + pr.fld0 * (long)(IL * IX));
                        const int vlane = fw * (IL * IX * 8) + 16 * l16;
                        UNROLL for (int a = 0; a < 4; ++a) {
                            const int i_ = rl + 4 * (a & 1);
                            const int grow = (a >> 1) ? IL - 1 - CP * c - i_ : CP * c + i_;
                            const double cgv = cg[grow];
                            const double sc = kc == 1 ? 1.0 : cgv;                          // fourier.f90:47-51
                            // rows of the southern half ascend from CP c, those of the northern half descend from IL-1 - CP c
                            const int voff = vlane + ((a >> 1) ? (CP - 1 - i_) : i_) * (IX * 8);
                            const int soff = ((a >> 1) ? IL - CP - CP * c : CP * c) * (IX * 8);
                            UNROLL for (int qq = 0; qq < 6; ++qq) {
                                const double *sp_ = src + 4 * a * RS + 32 * qq;
                                // The store and its two wait states are ONE instruction group: on gfx950 the data registers of a 128-bit
                                // store are still being read (last lanes of every 16-lane row) when the next instructions issue, the
                                // compiler (ROCm 7.2) protects them with one wait state -- none for a buffer store with an SGPR soffset --
                                // and reused them at once for the next row's address and scaling (19 such pairs in this kernel:
                                // tools/scan_store_hazard.py).  tools/store_valu_hazard.hip: one wait state still loses dwords, two do
                                // not; the data operand stays live to the end of the group.  (DESIGN s4.3: this is what the
                                // T63_ROLE_MIX experiment ran into.)
                                if (BYCHUNK && b.wt) t63_bstore2_safe<false, true>(rs_u4, voff + 256 * qq, soff, make_double2(sp_[0] * sc, sp_[1] * sc));
                                else t63_bstore2_safe<STREAM>(rs_u4, voff + 256 * qq, soff, make_double2(sp_[0] * sc, sp_[1] * sc));
                            }
                        }
                    }
                }
            }
            T63_MARK(1, u, 4);
            lds_barrier();
        }
    } else {
        // =================================================================== Legendre waves (one loop per wave variant)
        if (wi == 0) t63_inv_legendre_wave<0, BYCHUNK, OPS>(p, b, lds, wk, lane, w);
        else if (wi == 1) t63_inv_legendre_wave<1, BYCHUNK, OPS>(p, b, lds, wk, lane, w);
        else if (wi == 2) t63_inv_legendre_wave<2, BYCHUNK, OPS>(p, b, lds, wk, lane, w);
        else t63_inv_legendre_wave<3, BYCHUNK, OPS>(p, b, lds, wk, lane, w);
    }
}

// pair0 / npairs of a batch whose segments' src, dst, nb, ... are filled in; segments with nb <= 0 are dropped
static int t63_finish_batch(T63Batch &b)
{
    // derived segments (inverse launches: T63_OP_*) lead the launch -- stable partition; every segment has its own arrays, so the
    // order of the segments within a launch is free
    for (int i = 1; i < b.nseg; ++i)
        for (int j = i; j > 0 && b.seg[j].op != T63_OP_NONE && b.seg[j - 1].op == T63_OP_NONE; --j) { const T63Seg t = b.seg[j]; b.seg[j] = b.seg[j - 1]; b.seg[j - 1] = t; }
    int n = 0, pairs = 0;
    for (int i = 0; i < b.nseg; ++i) {
        if (b.seg[i].nb <= 0) continue;
        b.seg[n] = b.seg[i];
        b.seg[n].pair0 = pairs;
        pairs += b.seg[n].op == T63_OP_VDS ? b.seg[n].nb : (b.seg[n].nb + 1) / 2;
        ++n;
    }
    b.nseg = n;
    b.npairs = pairs;
    long fields = 0;
    for (int i = 0; i < n; ++i) fields += b.seg[i].op == T63_OP_VDS ? 2L * b.seg[i].nb : b.seg[i].nb;
    return (int)fields;
}

// Whether a launch of `pairs` field pairs takes the by-chunk form with its one-item-per-workgroup operator region -- the only form
// that derives (callers otherwise run the operator kernel first) -- and its derived pairs (T63_OP_*) fit that region.  The size
// threshold is set by the lead operator's `lead_op_pairs` (U / V, or the gradient when it is alone); the region holds all `op_pairs`.
bool s2g_t63_derives(int max_wg, int pairs, int lead_op_pairs, int op_pairs)
{
    const int nwg = max_wg > 0 ? max_wg : 256;
    return lead_op_pairs > 0 && 2 * pairs <= nwg && 2 * lead_op_pairs * t63::NCH <= nwg && op_pairs * t63::NCH <= nwg;
}

hipError_t launch_s2g_fused_t63_batch(const DevPlan &p, T63Batch b, int max_wg, hipStream_t s)
{
    if (b.nseg < 0 || b.nseg > T63_MAX_SEG) return hipErrorInvalidValue;
    const int fields = t63_finish_batch(b);
    if (fields <= 0) return hipSuccess;
    if (p.trunc != t63::TRUNC || p.ix != t63::IX || p.il != t63::IL || !p.img_s2g63) return hipErrorInvalidValue;
    const int nwg = max_wg > 0 ? max_wg : 256;
    b.by_chunk = 2 * b.npairs <= nwg;           // fewer pairs than half the CUs: one (pair, chunk) item per workgroup step
    int op_pairs = 0;
    for (int i = 0; i < b.nseg; ++i) {
        if (b.seg[i].op < T63_OP_NONE || b.seg[i].op > T63_OP_GY) return hipErrorInvalidValue;
        if (b.seg[i].op == T63_OP_NONE) continue;
        if (!b.seg[i].scale || !p.uvdx || !p.gradx_e || (i > 0 && b.seg[i - 1].op == T63_OP_NONE)) return hipErrorInvalidValue;
        op_pairs += (b.seg[i].nb + 1) / 2;
    }
    b.wt = write_through_policy(p, (long)fields * t63::IL * t63::IX * 8);   // (by-chunk form only: the large forms stream)
    const int units = b.by_chunk ? b.npairs * t63::NCH : b.npairs;
    // by-chunk: consecutive items per workgroup -- the derived segments' items (they lead the launch: t63_finish_batch) one each
    b.nop_items = b.by_chunk ? op_pairs * t63::NCH : 0;
    if (b.nop_items > nwg) return hipErrorInvalidValue;                        // (callers keep larger derived batches on the operator-kernel route)
    b.ipw = b.by_chunk ? (units == b.nop_items ? 1 : (units - b.nop_items + (nwg - b.nop_items) - 1) / max(1, nwg - b.nop_items)) : 1;
    const dim3 grd((unsigned)(b.by_chunk ? b.nop_items + (units - b.nop_items + b.ipw - 1) / b.ipw : units < nwg ? units : nwg)), blk(t63::NTHR);
    const bool ops = op_pairs > 0;
    if (ops && !b.by_chunk) return hipErrorInvalidValue;   // derived segments: model-sized launches only (see t63_inv_load_b_op)
    const bool stream = !b.by_chunk && stream_policy((long)fields * t63::IL * t63::IX * 8);
    if (b.by_chunk && ops) hipLaunchKernelGGL((s2g_fused_t63_kernel<false, true, true>), grd, blk, t63::LDS_BYTES, s, p, b);
    else if (b.by_chunk) hipLaunchKernelGGL((s2g_fused_t63_kernel<false, true>), grd, blk, t63::LDS_BYTES, s, p, b);   // (small: never streams)
    else if (stream) hipLaunchKernelGGL((s2g_fused_t63_kernel<true, false>), grd, blk, t63::LDS_BYTES, s, p, b);
    else hipLaunchKernelGGL((s2g_fused_t63_kernel<false, false>), grd, blk, t63::LDS_BYTES, s, p, b);
    return hipGetLastError();
}

hipError_t launch_s2g_fused_t63(const DevPlan &p, int nb, const double *spec, const int *d_kcos, int kcos_all, double *grid, int max_wg,
                                hipStream_t s)
{
    T63Batch b{};
    b.nseg = 1;
    b.seg[0] = T63Seg{spec, grid, nullptr, d_kcos, nb, kcos_all, 0, 0};
    return launch_s2g_fused_t63_batch(p, b, max_wg, s);
}

bool g2s_t63_staged(const DevPlan &p, int max_wg, int pairs)
{
    const int nwg = max_wg > 0 ? max_wg : 256;
    return p.rows_ws && 2 * pairs <= p.rows_ws_fields && 3 * pairs <= nwg && !p.lo.t63_nostage;
}

hipError_t launch_g2s_fused_t63_batch(const DevPlan &p, T63Batch b, int max_wg, hipStream_t s)
{
    if (b.nseg < 0 || b.nseg > T63_MAX_SEG) return hipErrorInvalidValue;
    bool any_vds = false;
    for (int i = 0; i < b.nseg; ++i) {
        if (b.seg[i].op != T63_OP_NONE && b.seg[i].op != T63_OP_VDS) return hipErrorInvalidValue;
        if (b.seg[i].op == T63_OP_VDS && b.seg[i].nb > 0) {
            if (any_vds || !b.vds_src2 || !b.vds_dst2 || !p.vddym || !p.vddyp || !p.gradx) return hipErrorInvalidValue;   // (one such segment per launch)
            any_vds = true;
        }
    }
    const int fields = t63_finish_batch(b);
    if (fields <= 0) return hipSuccess;
    if (p.trunc != t63::TRUNC || p.ix != t63::IX || p.il != t63::IL || !p.img_g2s63) return hipErrorInvalidValue;
    const int nwg = max_wg > 0 ? max_wg : 256;
    const dim3 grd(b.npairs < nwg ? b.npairs : nwg), blk(t63::NTHR);
    bool scaled = false;
    for (int i = 0; i < b.nseg; ++i) scaled = scaled || b.seg[i].scale != nullptr;
    const bool stream = stream_policy((long)fields * t63::IL * t63::IX * 8);
    const bool no_split = p.lo.t63_nosplit != 0;
    // (round 5's three-pairs-per-workgroup form of this transform -- one wave per SIMD, accumulators in AGPRs; same bits, 6 us
    // slower at B = 1536 -- left the product in round 6: tools/experiments/r05_spdy_t63_tri.inc, DESIGN 4.3)
    if (any_vds && !g2s_t63_staged(p, max_wg, b.npairs)) return hipErrorInvalidValue;     // (vds rides in the staged form only)
    if (g2s_t63_staged(p, max_wg, b.npairs)) {
        // small batch, staged: the row FFTs over (pair, chunk, field) items, four per workgroup (one round of workgroups), then
        // the contraction over (pair, quad position) items
        const dim3 gr((2 * t63::NCH * b.npairs + 3) / 4);
        constexpr int RLDS = (4 * 16 * t63::RS + t63::TW) * 8 + 4 * 68;
        if (scaled) hipLaunchKernelGGL((g2s_rows_t63_kernel<1>), gr, dim3(256), RLDS, s, p, b);
        else hipLaunchKernelGGL((g2s_rows_t63_kernel<0>), gr, dim3(256), RLDS, s, p, b);
        if (any_vds) hipLaunchKernelGGL((g2s_contract_t63_kernel<1, true>), dim3(4 * b.npairs), dim3(256), 0, s, p, b);
        else if (b.npairs >= p.lo.t63_np2_from) hipLaunchKernelGGL(g2s_contract_t63_kernel<2>, dim3(4 * ((b.npairs + 1) / 2)), dim3(256), 0, s, p, b);
        else hipLaunchKernelGGL(g2s_contract_t63_kernel<1>, dim3(4 * b.npairs), dim3(256), 0, s, p, b);
    } else if (2 * b.npairs <= nwg && !no_split) {       // small batch: two workgroups per pair, each contracts half of the zonal wavenumbers
        const dim3 g2(2 * b.npairs);
        if (scaled) hipLaunchKernelGGL((g2s_fused_t63_kernel<1, false, true>), g2, blk, t63::LDS_BYTES, s, p, b);
        else hipLaunchKernelGGL((g2s_fused_t63_kernel<0, false, true>), g2, blk, t63::LDS_BYTES, s, p, b);
    } else if (scaled && stream) hipLaunchKernelGGL((g2s_fused_t63_kernel<1, true>), grd, blk, t63::LDS_BYTES, s, p, b);
    else if (scaled) hipLaunchKernelGGL((g2s_fused_t63_kernel<1, false>), grd, blk, t63::LDS_BYTES, s, p, b);
    else if (stream) hipLaunchKernelGGL((g2s_fused_t63_kernel<0, true>), grd, blk, t63::LDS_BYTES, s, p, b);
    else hipLaunchKernelGGL((g2s_fused_t63_kernel<0, false>), grd, blk, t63::LDS_BYTES, s, p, b);
    return hipGetLastError();
}

hipError_t launch_g2s_fused_t63(const DevPlan &p, int nb, const double *grid, const double *gscale, double *spec, int max_wg, hipStream_t s)
{
    T63Batch b{};
    b.nseg = 1;
    b.seg[0] = T63Seg{grid, spec, gscale, nullptr, nb, 1, 0, 0};
    return launch_g2s_fused_t63_batch(p, b, max_wg, s);
}
