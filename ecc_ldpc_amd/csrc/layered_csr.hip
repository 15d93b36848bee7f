// layered_csr.hip -- row-layered min-sum for ANY parity-check matrix: lam ON-CHIP (as fp16 or as f32), row records streamed from HBM.
//
// layered_lds.hip carried over from quasi-cyclic codes to CSR graphs.  Same arithmetic, same roundings (f32 arithmetic and records,
// every lam write saturated and rounded to binary16 -- specification oracle/emulate_f16.py decode_minsum_f16_layered, rows in
// ascending order, reproduced bit for bit), same row records {3/4 min1, 3/4 min2, signs | arg-min} in a per-workgroup scratch area,
// same persistent workgroups taking frames from a counter.  What differs is where a row's edges come from:
//   * a code-constant COLUMN TABLE in device memory, shared by all workgroups (L2-resident), 16-bit column indices laid out
//     [slab][edge k][thread]: a wave's k-th gather addresses are one contiguous 128-byte load;
//   * STEPS instead of block rows: each maximal run of consecutive layers (ldpc_code_set_layers; default one row per layer) that are
//     pairwise column-disjoint is one barrier step -- its rows touch distinct lam cells, so running them together gives what running
//     them one after the other gives.  A step's rows are sorted by weight (heaviest first) and cut into SLABS of T rows, thread t
//     taking row t of every slab of the step; rows lighter than their wave's heaviest are padded with neutral edges (index 0xFFFF:
//     no lam read or write, no part in min, sign, parity or flip).
// LDS: the frame's lam (sizeof(LT) N bytes, LT the type of a lam cell) + 32 bytes of control words; the short codes get several
// workgroups per CU.
// The lam cell's type LT is the kernel's second template parameter.  _Float16 (LDPC_F16) is everything said above.  float (LDPC_F32)
// keeps the cell as the arithmetic produced it -- nothing rounded, nothing saturated, N <= 40 952 -- and is,
// bit for bit, flood.hip's layered_kernel<float, min-sum> on the same code and layers (tests/test_layered_csr_f32_gpu.py).  Without
// saturation a frame that diverges reaches +-inf, then NaN, whose hard decisions are an all-zero "codeword": that instance carries the
// non-finite veto of ldpc_math.h kVetoesNonFinite -- when a frame's stop rule fires the workgroup scans its lam once, and any cell
// that is not finite turns "converged" into "failed" (flag 0, the sweep limit as its count, the channel's decisions and LLRs).
// int8_t (LDPC_I8) is a FIXED-POINT decoder, the kind hardware receivers implement -- specification tests/layered_i8_spec.py,
// reproduced bit for bit: the channel LLRs are quantised on load, q = clip(rint(llr * qscale), -127, 127) with one float multiply
// (int8 LLRs, format LLR_I8, are taken as they are, -128 as -127); lam is one byte per column (N + 32 bytes of LDS, byte LDS loads and
// stores); a row is 32-bit integer arithmetic with the 3/4 as (3 m + 2) >> 2 and every lam write clipped to +-127 -- no float
// instruction inside a sweep, no veto (the clip bounds the state); a row record is 8 bytes {3/4 min1 | 3/4 min2 << 16, signs |
// arg-min}, one dwordx2 each way: sweeps * 16 M bytes per frame.  Same column table, steps, slabs and control words.
// Algorithmic HBM bytes per frame: sweeps * 24 M (the first sweep writes only) + the LLRs in + the bits out; the column table
// (2 bytes per padded edge) is read by every workgroup every sweep and stays in L2.
// THE CHECK-NODE RULE (ldpc_ctx_config cn_scale = alpha, cn_offset = beta; specification tests/layered_rule_spec.py, reproduced bit for
// bit).  layered_csr_kernel<D, LT> computes |msg'| = 3/4 min as above and knows no other rule.  A context with another rule runs
// layered_csr_kernel<D, Ruled<LT>>: the same kernel compiled with RULE = true, in which the ONE line of a row that turns its two minima
// into its two message magnitudes reads the rule from the last member of the argument structure (wave-uniform: SGPRs) --
//   float cells: n = fl(fl(alpha) * m) - fl(beta), then n < 0 ? 0 : n (two roundings -- the library is built with contraction off and
//                the function says so again --, a compare-select so that a NaN stays a NaN and the f32 instance's veto sees what it saw);
//   int8 cells:  n = min(max(((a m + 8) >> 4) - b, 0), 511), a = clip(rint(16 alpha), 1, 16), b = rint(beta qscale): integers only.
// Nothing per edge: a subtract and a select (int8: a max and a min) per minimum, two minima per row.  The nine layered_csr_kernel
// plain instances are instruction for instruction what they were before the rule existed (profiles/r10_layered_rule_default_ab.txt).
// THE A-MIN* RULE (ldpc_ctx_config cn_rule = LDPC_CN_AMINSTAR; Jones, Valles, Smith, Villasenor 2003; specification
// tests/layered_aminstar_spec.py, reproduced bit for bit).  layered_csr_kernel<D, MinStar<LT>>, LT = _Float16 or float: the same kernel
// compiled with RULE = kRuleAMinStar.  A-min* sends two magnitudes per row, like min-sum -- Delta, the box-plus of every |t| but the least,
// to the arg-min edge, and n1 = Delta [+] m1 to every other edge -- so the row record {c1 = n1, c2 = Delta, signs | arg-min} is what it was
// and nothing of the soft output, the decode state or the HBM traffic changes.  What changes in a row: the first pass keeps the arg-min BY
// INDEX (the first edge with the least |t|: a strict compare and two selects per edge in place of med3 + min), a serial fold of
// a [+] b = max(min(a, b) + c(a + b) - c(|a - b|), 0), c(x) = max(0.625 - x / 4, 0), over the other edges (a min, three adds / subtracts,
// two multiplies, two subtracts from a constant and three compare-selects per edge, each rounded on its own: no transcendental, no table),
// and the write loop picks the magnitude by index -- an edge that ties with m1 takes n1, which here differs from Delta.  A row of weight 2
// is exact.  The 54 instances without it are instruction for instruction what they were (tools/same_kernels.py against a build of the
// parent commit; profiles/r23_aminstar.txt).
// THE SOFT OUTPUT (ldpc_decode_batch_dev_soft; specification tests/soft_output_spec.py, reproduced bit for bit).  In a layered schedule the
// lam cells in LDS ARE the posterior, so the output is an epilogue of the frame: lam as it stands when the frame stops -- converged, out of
// sweeps or vetoed alike --, or that less the channel LLR as the cell took it in, read from memory again; f32, fp16 or int8 out.  It lives in
// instances of their own, layered_csr_soft_kernel<D, CELL>, which take one more argument.  The body of the kernels is text,
// layered_csr_body.h, included once per kernel: the eighteen layered_csr_kernel instances are compiled from what they were compiled from before and
// are instruction for instruction and register for register what they were (profiles/r20_bicm_id.txt).
// THE DECODE THAT CONTINUES (ldpc_decode_state_*, ldpc_decode_batch_dev_continue; specification tests/decode_continue_spec.py, reproduced bit
// for bit).  The row records ARE a frame's check-to-variable messages, and with the per-column sum S of those messages they are all a decode
// needs to go on from where it stopped.  A decode state keeps both per frame slot in device memory -- [slot][nslab][T] records in the
// context's geometry, [slot][N] sums as float (int16 for int8 cells): 12 nslab T + 4 N bytes a slot, 8 nslab T + 2 N for int8 --, read once
// and written once per call on top of the plain decode's traffic.  layered_csr_cont_kernel<D, CELL> is the third inclusion of the body:
// lam <- cell(C' + S) in the prologue (a reset slot adds +0), the syndrome before the first sweep is that lam's, every sweep reads its
// records (a zero record is "no old message": t = l - (+0) is l bit for bit), the epilogue writes S <- lam - C' for every frame and the soft
// output when asked.  The 36 other instances are what they were (profiles/r21_decode_continue.txt).
// WHERE THINGS ARE.  Which of the 72 instances exist (3 families x 3 row classes x 8 cells), how a context's (dtype, rule, row class) picks
// one and what each is called is ONE list, instance_of below the kernels; a new cell type or rule is a line there.  The three decodes share
// one launch path, LayeredCsrState::run, and one residency query.  The graph work -- steps, slabs, the column table, the per-wave weights --
// is host code of its own, layered_csr_layout.{h,cc}, with a stand-alone driver that runs it under a sanitizer
// (tools/layered_csr_layout_main.cc, tests/test_layered_csr_layout.py).  Every kernel is the code it was (profiles/r25_layered_csr_host.txt).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "demap.h"
#include "layered_csr_layout.h"
#include "layered_qc.h"
#include "ldpc_math.h"
#include "mod_dispatch.h"

namespace ldpc {

typedef const __attribute__((address_space(4))) int32_t *ctab_t;   // graph tables: scalar loads (never written by the kernel)

struct CsrRec { float c1, c2; uint32_t meta; };   // meta: bit (deg-1-k) = sign bit of the message on edge k; bits 27..31 = an arg-min edge
// int8 lam: the two message magnitudes (3/4 min1 in bits 0..15, 3/4 min2 in bits 16..31; both < 2^9) and the same meta word
struct __attribute__((aligned(8))) CsrRecI8 { uint32_t mags, meta; };

struct CsrLayDev {             // (the four tables are built by layered_csr_layout.cc, which also defines kNoEdge)
    int N, T, nstep;
    const uint16_t *cols;       // per slab, [edge k < slab weight][thread]: column index, kNoEdge past the row's weight
    const int32_t *slab;        // [nslab][2]: {first entry in cols, slab weight (its heaviest row)}
    const int32_t *wdeg;        // [nslab][T / 64]: the heaviest row of each wave of the slab, | 0x100 when all 64 rows of the wave have that weight
    const int32_t *step_ptr;    // [nstep + 1]: the slabs of each barrier step
};

// the check-node rule of the Ruled instances (float cells read scale / offset, int8 cells a / b)
struct CsrRule { float scale, offset; int a, b; };
// the kernel's second template argument: the lam cell's type -- _Float16, float, int8_t: the 3/4 --, or Ruled<that type>: the same
// kernel with the context's rule in place of the 3/4 (a compile-time flag: the plain instances hold no trace of it)
template <typename LT> struct Ruled {};
// ... or MinStar<_Float16 / float>: the same kernel with the A-min* row (see THE A-MIN* RULE above) in place of the two minima
template <typename LT> struct MinStar {};
enum { kRule34 = 0, kRuleScaled = 1, kRuleAMinStar = 2 };
template <typename X> struct CellOf { typedef X type; static constexpr int rule = kRule34; };
template <typename X> struct CellOf<Ruled<X>> { typedef X type; static constexpr int rule = kRuleScaled; };
template <typename X> struct CellOf<MinStar<X>> { typedef X type; static constexpr int rule = kRuleAMinStar; };

struct CsrLayArgs {
    const void *llr; int llr_fmt;   // [batch][N]
    float qscale;                   // (int8 lam) the quantiser's scale
    uint8_t *bits; int32_t *iters; uint8_t *conv;
    double *final_lam;              // may be null
    int batch, max_iters;
    int *work_counter;              // next frame to take = gridDim.x + atomicAdd(work_counter, 1)
    CsrRule rule;                   // (last: the Ruled instances alone read it; every other member sits where it sat without it)
};

// the soft output of layered_csr_soft_kernel (ldpc_decode_batch_dev_soft): an argument of its own, after the three every instance takes
struct CsrSoftArgs {
    void *out;                      // [batch][N] of element type fmt
    int fmt;                        // MOD_LLR_F32 / _F16 / _I8 (= LDPC_LLR_*)
    int kind;                       // LDPC_SOFT_POSTERIOR: lam as it stands; LDPC_SOFT_EXTRINSIC: lam - the channel LLR as the cell took it in
    float qscale;                   // (float cells, fmt _I8) the scale of the output's quantiser
};

// the decode state of layered_csr_cont_kernel (ldpc_decode_batch_dev_continue): frame f of the call lives in slot first + f
struct CsrContArgs {
    void *rec;                      // [slots][nslab][T] row records (CsrRec, or CsrRecI8 with int8 lam), in the context's own geometry
    void *sum;                      // [slots][N] the sum of check messages per column: float (fp16 and f32 cells) or int16 (int8 cells)
    int first;
};

namespace {   // (the device helpers below are layered_lds.hip's, kept local to this file)

__device__ __forceinline__ void lds_barrier() {     // LDS traffic only: global loads / stores stay in flight across it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

__device__ __forceinline__ _Float16 sat16(float v) { return (_Float16)__builtin_amdgcn_fmed3f(v, -65504.f, 65504.f); }

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float8 __attribute__((ext_vector_type(8)));

// a lam cell of type LT: what a float becomes when it is stored (fp16: saturated and rounded; f32: itself), eight cells at once
template <typename LT> struct Cell;
template <> struct Cell<_Float16> {
    typedef half8 vec8;
    typedef CsrRec Rec;
    static __device__ __forceinline__ _Float16 of(float v) { return sat16(v); }
    static __device__ __forceinline__ _Float16 llr(float v) { return sat16(nan_as_zero(v)); }   // a channel LLR: a NaN is an erasure (ldpc_math.h)
    static __device__ __forceinline__ void st8(_Float16 *p, const half8 &h) { *reinterpret_cast<half8 *>(p) = h; }
    static __device__ __forceinline__ half8 ld8(const _Float16 *p) { return *reinterpret_cast<const half8 *>(p); }
};
template <> struct Cell<float> {
    typedef float8 vec8;
    typedef CsrRec Rec;
    static __device__ __forceinline__ float of(float v) { return v; }
    static __device__ __forceinline__ float llr(float v) { return v; }                          // (f32 state takes the values as they are)
    static __device__ __forceinline__ void st8(float *p, const float8 &h) {      // two 16-byte LDS stores
        *reinterpret_cast<float4 *>(p) = make_float4(h[0], h[1], h[2], h[3]);
        *reinterpret_cast<float4 *>(p + 4) = make_float4(h[4], h[5], h[6], h[7]);
    }
    static __device__ __forceinline__ float8 ld8(const float *p) {
        const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
        float8 h;
        h[0] = a.x; h[1] = a.y; h[2] = a.z; h[3] = a.w; h[4] = b.x; h[5] = b.y; h[6] = b.z; h[7] = b.w;
        return h;
    }
};

// eight channel LLRs as lam cells (16-byte requests)
template <typename LT, int FMT> __device__ __forceinline__ void load_llr8(const void *base, size_t i, typename Cell<LT>::vec8 &h) {
    if constexpr (FMT == LLR_F64) {
#pragma unroll
        for (int k = 0; k < 8; k++) h[k] = Cell<LT>::llr((float)reinterpret_cast<const double *>(base)[i + k]);
    } else if constexpr (FMT == LLR_F16) {
        const half8 v = *reinterpret_cast<const half8 *>(reinterpret_cast<const _Float16 *>(base) + i);
#pragma unroll
        for (int k = 0; k < 8; k++) h[k] = Cell<LT>::llr((float)v[k]);
    } else {
        const float4 a = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(base) + i);
        const float4 b = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(base) + i + 4);
        h[0] = Cell<LT>::llr(a.x); h[1] = Cell<LT>::llr(a.y); h[2] = Cell<LT>::llr(a.z); h[3] = Cell<LT>::llr(a.w);
        h[4] = Cell<LT>::llr(b.x); h[5] = Cell<LT>::llr(b.y); h[6] = Cell<LT>::llr(b.z); h[7] = Cell<LT>::llr(b.w);
    }
}

template <typename LT> __device__ __forceinline__ __attribute__((address_space(3))) LT *lds_cell(uint32_t byte_addr) {
    return (__attribute__((address_space(3))) LT *)(uintptr_t)byte_addr;
}

// ---- int8 lam (LDPC_I8): the quantiser of tests/layered_i8_spec.py, the frame's way in and out, the row in integers
template <> struct Cell<int8_t> { typedef uint2 vec8; typedef CsrRecI8 Rec; };      // (eight cells: the bytes of two words)
template <typename LT> struct Cell<Ruled<LT>> : Cell<LT> {};                         // (the rule changes no cell and no record)
template <typename LT> struct Cell<MinStar<LT>> : Cell<LT> {};

__device__ __forceinline__ int quant_i8(float v, float qs) {
    const float r = __builtin_rintf(v * qs);           // ONE float multiply (no contraction), ties to even
    return r != r ? 0 : (int)__builtin_amdgcn_fmed3f(r, -127.f, 127.f);
}
// LLR_I8 is dispatched here only: the other kernels' prologues (ldpc_math.h with_llr_format / load_llr_as) do not know it
template <class F> __device__ __forceinline__ void with_llr_format_i8(int fmt, F &&f) {
    if (fmt == LLR_I8) f(std::integral_constant<int, LLR_I8>{});
    else with_llr_format(fmt, f);
}
template <int FMT> __device__ __forceinline__ int load_q(const void *base, size_t i, float qs) {
    if constexpr (FMT == LLR_I8) return max((int)reinterpret_cast<const int8_t *>(base)[i], -127);
    else return quant_i8(load_llr_as<float, FMT>(base, i), qs);
}
// eight channel LLRs as the eight cells of two words (one 8-byte request of int8 LLRs, 16-byte requests of fp16 / f32 ones)
template <int FMT> __device__ __forceinline__ uint2 load_q8(const void *base, size_t i, float qs) {
    int q[8];
    if constexpr (FMT == LLR_I8) {
        const uint2 w = *reinterpret_cast<const uint2 *>(reinterpret_cast<const int8_t *>(base) + i);
#pragma unroll
        for (int k = 0; k < 4; k++) { q[k] = max((int)(int8_t)(w.x >> (8 * k)), -127); q[k + 4] = max((int)(int8_t)(w.y >> (8 * k)), -127); }
    } else if constexpr (FMT == LLR_F16) {
        const half8 v = *reinterpret_cast<const half8 *>(reinterpret_cast<const _Float16 *>(base) + i);
#pragma unroll
        for (int k = 0; k < 8; k++) q[k] = quant_i8((float)v[k], qs);
    } else if constexpr (FMT == LLR_F32) {
        const float4 a = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(base) + i);
        const float4 b = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(base) + i + 4);
        q[0] = quant_i8(a.x, qs); q[1] = quant_i8(a.y, qs); q[2] = quant_i8(a.z, qs); q[3] = quant_i8(a.w, qs);
        q[4] = quant_i8(b.x, qs); q[5] = quant_i8(b.y, qs); q[6] = quant_i8(b.z, qs); q[7] = quant_i8(b.w, qs);
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) q[k] = load_q<FMT>(base, i + k, qs);
    }
    uint2 w = make_uint2(0u, 0u);
#pragma unroll
    for (int k = 0; k < 4; k++) { w.x |= ((uint32_t)q[k] & 0xFFu) << (8 * k); w.y |= ((uint32_t)q[k + 4] & 0xFFu) << (8 * k); }
    return w;
}
// the hard decisions of eight cells, one byte per bit
__device__ __forceinline__ uint2 hard_q8(uint2 w) {
    uint2 b = make_uint2(0u, 0u);
#pragma unroll
    for (int k = 0; k < 4; k++) { b.x |= ((int8_t)(w.x >> (8 * k)) > 0 ? 1u : 0u) << (8 * k); b.y |= ((int8_t)(w.y >> (8 * k)) > 0 ? 1u : 0u) << (8 * k); }
    return b;
}

// (a continuing decode) eight int8 cells plus eight int16 sums of check messages, clipped to +-127; and eight cells less eight cells as int16
__device__ __forceinline__ uint2 add_sum_q8(uint2 w, uint4 s) {
    const uint32_t sw[4] = {s.x, s.y, s.z, s.w};
    uint2 r = make_uint2(0u, 0u);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int lo = min(max((int)(int8_t)(w.x >> (8 * k)) + (int)(int16_t)(sw[k >> 1] >> (16 * (k & 1))), -127), 127);
        const int hi = min(max((int)(int8_t)(w.y >> (8 * k)) + (int)(int16_t)(sw[2 + (k >> 1)] >> (16 * (k & 1))), -127), 127);
        r.x |= ((uint32_t)lo & 0xFFu) << (8 * k); r.y |= ((uint32_t)hi & 0xFFu) << (8 * k);
    }
    return r;
}
__device__ __forceinline__ uint4 diff_q8(uint2 w, uint2 c) {
    uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int lo = (int)(int8_t)(w.x >> (8 * k)) - (int)(int8_t)(c.x >> (8 * k)), hi = (int)(int8_t)(w.y >> (8 * k)) - (int)(int8_t)(c.y >> (8 * k));
        d[k >> 1] |= ((uint32_t)lo & 0xFFFFu) << (16 * (k & 1)); d[2 + (k >> 1)] |= ((uint32_t)hi & 0xFFFFu) << (16 * (k & 1));
    }
    return make_uint4(d[0], d[1], d[2], d[3]);
}

// a message magnitude under the rule (alpha, beta), float cells: the product rounded, then the difference rounded -- never one fused
// multiply-add --, then a compare-select (not a max: max(NaN, 0) is 0, and a NaN has to stay one)
__device__ __forceinline__ float rule_mag(float m, float alpha, float beta) {
#pragma clang fp contract(off)
    const float p = alpha * m;
    const float n = p - beta;
    return n < 0.f ? 0.f : n;
}

// the A-min* rule's correction c(x) = max(0.625 - x / 4, 0), the two-segment fit of log(1 + exp(-x)), and a [+] b = max(min(a, b) + c(a + b)
// - c(|a - b|), 0) for two magnitudes: every operation rounded on its own (no fused multiply-add), compare-selects so that a NaN stays one.
// c is non-increasing and a + b >= |a - b|, so a [+] b <= min(a, b); the operands commute bit for bit
__device__ __forceinline__ float amin_corr(float x) {
#pragma clang fp contract(off)
    const float p = 0.25f * x;
    const float n = 0.625f - p;
    return n < 0.f ? 0.f : n;
}
__device__ __forceinline__ float boxplus(float a, float b) {
#pragma clang fp contract(off)
    const float s = fminf(a, b) + amin_corr(a + b);
    const float n = s - amin_corr(fabsf(a - b));
    return n < 0.f ? 0.f : n;
}

// one check row in 32-bit integers (tests/layered_i8_spec.py row_update); same table walk, same meta word as csr_row below
template <typename LT, int D, bool EXACT, bool FIRST, int RULE>
__device__ __forceinline__ void csr_row(const uint16_t *cp, int T, int wd, uint32_t lam0, const CsrRecI8 &in, CsrRecI8 &out, bool &odd, bool &flip, CsrRule rule) {
    uint32_t ad[D];
    int t[D];
    int deg = EXACT ? D : 0;
#pragma unroll
    for (int k = 0; k < D; k++) {
        const uint32_t c = (EXACT || k < wd) ? (uint32_t)cp[(size_t)k * T] : (uint32_t)kNoEdge;
        const bool v = EXACT || c != kNoEdge;
        if constexpr (!EXACT) deg += v ? 1 : 0;
        ad[k] = lam0 + (v ? c : 0u);
    }
#pragma unroll
    for (int k = 0; k < D; k++) t[k] = (int)*lds_cell<int8_t>(ad[k]);
    uint32_t hl = 0, X = 0;                             // hl: hard(lam) of edge k at bit k; X: bit 31 = xor of the signs of t
    int m1 = 0x7FFF, m2 = 0x7FFF;
    const int i1 = (int)(in.mags & 0xFFFFu), i2 = (int)(in.mags >> 16);
    const uint32_t oidx = in.meta >> 27;
#pragma unroll
    for (int k = 0; k < D; k++) {
        if (EXACT || k < deg) {
            hl |= (t[k] > 0 ? 1u : 0u) << k;
            if constexpr (!FIRST) {
                const int mag = ((uint32_t)k == oidx) ? i2 : i1;
                const int sg = (int)(in.meta << (32 - deg + k)) >> 31;      // -1: the message is negative
                t[k] -= (mag ^ sg) - sg;
            }
            X ^= (uint32_t)t[k];
            const int a = abs(t[k]);
            m2 = min(m2, max(m1, a));
            m1 = min(m1, a);
        }
    }
    odd |= (__builtin_popcount(hl) & 1) != 0;
    int n1, n2;
    if constexpr (RULE == kRuleScaled) {   // a / 16 rounded half up, less b, in 0..511 (the cap: at a = 16 no induction keeps a magnitude below 2^9)
        n1 = min(max(((rule.a * m1 + 8) >> 4) - rule.b, 0), 511); n2 = min(max(((rule.a * m2 + 8) >> 4) - rule.b, 0), 511);
    } else {
        n1 = (3 * m1 + 2) >> 2; n2 = (3 * m2 + 2) >> 2;             // 3/4, rounded half up
    }
    // message k is negative iff (deg odd) ^ (xor of all signs of t) ^ (sign of t_k)
    const int fl = -(int)(((X >> 31) ^ (uint32_t)deg) & 1u);       // -1 or 0
    uint32_t tsig = 0, nidx = 0;
#pragma unroll
    for (int k = 0; k < D; k++) {
        if (EXACT || k < deg) {
            const bool ismin = abs(t[k]) == m1;             // ties: n2 == n1, either answer gives the same message
            const int sg = fl ^ (t[k] >> 31);
            const int mag = ismin ? n2 : n1;
            nidx = ismin ? (uint32_t)k : nidx;
            tsig = (tsig << 1) | ((uint32_t)t[k] >> 31);
            const int nw = min(max(t[k] + ((mag ^ sg) - sg), -127), 127);
            flip |= (nw > 0) != (((hl >> k) & 1u) != 0);
            *lds_cell<int8_t>(ad[k]) = (int8_t)nw;
        }
    }
    const uint32_t nsig = tsig ^ (fl ? ((1u << deg) - 1u) : 0u);
    out.mags = (uint32_t)n1 | ((uint32_t)n2 << 16); out.meta = nsig | (nidx << 27);
}

// one check row: layered_lds.hip lds_row with the row's weight per LANE (deg <= D; EXACT: every lane's row has weight D).  cp: this
// lane's entry of edge 0 in the column table, edge k at cp[k T]; wd: the heaviest row of the wave (entries past it are not read).
template <typename LT, int D, bool EXACT, bool FIRST, int RULE>
__device__ __forceinline__ void csr_row(const uint16_t *cp, int T, int wd, uint32_t lam0, const CsrRec &in, CsrRec &out, bool &odd, bool &flip, CsrRule rule) {
    uint32_t ad[D];
    float l[D], t[D];
    int deg = EXACT ? D : 0;
#pragma unroll
    for (int k = 0; k < D; k++) {
        const uint32_t c = (EXACT || k < wd) ? (uint32_t)cp[(size_t)k * T] : (uint32_t)kNoEdge;
        const bool v = EXACT || c != kNoEdge;       // (the neutral entries are the last ones of a row)
        if constexpr (!EXACT) deg += v ? 1 : 0;
        ad[k] = lam0 + (uint32_t)sizeof(LT) * (v ? c : 0u);
    }
#pragma unroll
    for (int k = 0; k < D; k++) l[k] = (float)*lds_cell<LT>(ad[k]);
    bool par = false;
    uint32_t X = 0;
    float m1 = INFINITY;
    [[maybe_unused]] float m2 = INFINITY;
    [[maybe_unused]] uint32_t imin = 0;                 // (A-min*) the arg-min edge
    const uint32_t oidx = in.meta >> 27;
#pragma unroll
    for (int k = 0; k < D; k++) {
        if (EXACT || k < deg) {
            par ^= hard(l[k]);
            float old = 0.f;
            if constexpr (!FIRST) {
                const uint32_t mag = __float_as_uint(((uint32_t)k == oidx) ? in.c2 : in.c1);
                old = __uint_as_float(mag | ((in.meta << (32 - deg + k)) & 0x80000000u));
            }
            t[k] = l[k] - old;
            X ^= __float_as_uint(t[k]);
            const float a = fabsf(t[k]);
            if constexpr (RULE == kRuleAMinStar) {          // the arg-min by index: the FIRST edge with the least |t|
                const bool lt = a < m1;
                imin = lt ? (uint32_t)k : imin;
                m1 = lt ? a : m1;
            } else {
                m2 = __builtin_amdgcn_fmed3f(m1, m2, a);
                m1 = fminf(m1, a);
            }
        } else t[k] = INFINITY;
    }
    odd |= par;
    float n1, n2;
    if constexpr (RULE == kRuleAMinStar) {
        // n2 = Delta, the [+] of every |t_k| but the arg-min's, folded in ascending k from the first such edge (edge 0, or edge 1 when
        // the arg-min is edge 0); n1 = Delta [+] m1.  A row of weight 2 is exact: Delta is the other edge's |t|, n1 = m1
        float dl = fabsf(imin == 0 ? t[1] : t[0]);
#pragma unroll
        for (int k = 1; k < D; k++) {
            if (EXACT || k < deg) {
                const float nd = boxplus(dl, fabsf(t[k]));
                dl = ((uint32_t)k == imin || (k == 1 && imin == 0)) ? dl : nd;
            }
        }
        n2 = dl;
        if constexpr (EXACT && D == 2) n1 = m1;
        else n1 = deg <= 2 ? m1 : boxplus(dl, m1);
    } else if constexpr (RULE == kRuleScaled) {
        n1 = rule_mag(m1, rule.scale, rule.offset); n2 = rule_mag(m2, rule.scale, rule.offset);
    } else {
        n1 = 0.75f * m1; n2 = 0.75f * m2;               // |(-3/4) * acc|: the one rounding of Min.hs:78
    }
    // sign bit of message k = (deg odd) ^ (xor of all sign bits of t) ^ (sign bit of t_k)   (cn_update_padded)
    const uint32_t fl = (X ^ ((deg & 1) ? 0x80000000u : 0u)) & 0x80000000u;
    uint32_t c1 = __float_as_uint(n1) ^ fl, c2 = __float_as_uint(n2) ^ fl;
    uint32_t tsig = 0, nidx = 0;                        // tsig: the sign bits of t, edge k at bit deg - 1 - k
#pragma unroll
    for (int k = 0; k < D; k++) {
        if (EXACT || k < deg) {
            bool ismin;
            if constexpr (RULE == kRuleAMinStar) ismin = (uint32_t)k == imin;   // by index: a tie with m1 elsewhere takes n1, which is not n2 here
            else ismin = fabsf(t[k]) == m1;                 // ties: n2 == n1, either answer gives the same message
            const uint32_t nmb = __builtin_amdgcn_bitop3_b32(ismin ? c2 : c1, __float_as_uint(t[k]), 0x80000000u, 0x78);   // a ^ (b & c)
            nidx = ismin ? (uint32_t)k : nidx;
            tsig = __builtin_amdgcn_alignbit(tsig, __float_as_uint(t[k]), 31);
            const LT nw = Cell<LT>::of(t[k] + __uint_as_float(nmb));
            flip |= (nw > (LT)0) != hard(l[k]);
            *lds_cell<LT>(ad[k]) = nw;
        }
    }
    const uint32_t nsig = tsig ^ (fl ? ((1u << deg) - 1u) : 0u);
    out.c1 = n1; out.c2 = n2; out.meta = nsig | (nidx << 27);
}

// the instance for a wave: wd = its heaviest row, uni = all its rows have that weight
template <typename LT, int DCLASS, bool FIRST, int RULE>
__device__ __forceinline__ void csr_row_at(const uint16_t *cp, int T, int wd, bool uni, uint32_t lam0, const typename Cell<LT>::Rec &in,
                                           typename Cell<LT>::Rec &out, bool &odd, bool &flip, CsrRule rule) {
    if (uni) {
        switch (wd) {
            case 2: csr_row<LT, 2, true, FIRST, RULE>(cp, T, wd, lam0, in, out, odd, flip, rule); return;
            case 3: csr_row<LT, 3, true, FIRST, RULE>(cp, T, wd, lam0, in, out, odd, flip, rule); return;
            case 4: csr_row<LT, 4, true, FIRST, RULE>(cp, T, wd, lam0, in, out, odd, flip, rule); return;
            case 5: csr_row<LT, 5, true, FIRST, RULE>(cp, T, wd, lam0, in, out, odd, flip, rule); return;
            case 6: csr_row<LT, 6, true, FIRST, RULE>(cp, T, wd, lam0, in, out, odd, flip, rule); return;
            case 7: csr_row<LT, 7, true, FIRST, RULE>(cp, T, wd, lam0, in, out, odd, flip, rule); return;
            case 8: csr_row<LT, 8, true, FIRST, RULE>(cp, T, wd, lam0, in, out, odd, flip, rule); return;
            default: break;
        }
    }
    if (wd <= 0) { out = in; return; }                  // (a wave of idle lanes or empty rows)
    if (wd <= 4) { csr_row<LT, 4, false, FIRST, RULE>(cp, T, wd, lam0, in, out, odd, flip, rule); return; }
    if (wd <= 8) { csr_row<LT, 8, false, FIRST, RULE>(cp, T, wd, lam0, in, out, odd, flip, rule); return; }
    if constexpr (DCLASS >= 20) {
        if (wd <= 12) { csr_row<LT, 12, false, FIRST, RULE>(cp, T, wd, lam0, in, out, odd, flip, rule); return; }
        if (wd <= 20) { csr_row<LT, 20, false, FIRST, RULE>(cp, T, wd, lam0, in, out, odd, flip, rule); return; }
    }
    if constexpr (DCLASS >= 32) csr_row<LT, 27, false, FIRST, RULE>(cp, T, wd, lam0, in, out, odd, flip, rule);
}

// ---- the soft output's element: a float cell's value through the demappers' llr_out; an int8 cell's integer v as v / qscale (ONE
// division), that float as fp16, or the integer clipped
template <class F> __device__ __forceinline__ void with_soft_format(int fmt, F &&f) {
    if (fmt == MOD_LLR_F16) f((__half *)nullptr);
    else if (fmt == MOD_LLR_I8) f((int8_t *)nullptr);
    else f((float *)nullptr);
}
template <typename OT> __device__ __forceinline__ OT soft_of_q(int v, float cq) {
    if constexpr (std::is_same<OT, int8_t>::value) return (int8_t)min(max(v, -127), 127);
    else return llr_out<OT>((float)v / cq, 0.f);
}
// eight consecutive elements: 16-byte stores (int8: one 8-byte store)
template <typename OT> __device__ __forceinline__ void st_soft8(OT *p, const OT (&o)[8]) {
    if constexpr (sizeof(OT) == 1) {
        uint2 a;
        __builtin_memcpy(&a, o, 8);
        *reinterpret_cast<uint2 *>(p) = a;
    } else {
        uint4 a;
        __builtin_memcpy(&a, o, 16);
        *reinterpret_cast<uint4 *>(p) = a;
        if constexpr (sizeof(OT) == 4) {
            __builtin_memcpy(&a, o + 4, 16);
            *reinterpret_cast<uint4 *>(p + 4) = a;
        }
    }
}

}  // namespace

// block = T threads (a multiple of 64, at most csr_max_threads); grid = resident workgroups (persistent).  Rows above weight 20 keep
// up to 27 addresses, LLRs and differences per lane: that instance is built for 512 threads (256 registers per lane, no spill).
constexpr int csr_max_threads(int dclass) { return dclass > 20 ? 512 : 1024; }
// CELL: the lam cell's type (the 3/4, A.rule is not read), or Ruled<that type> (the rule of A.rule)
template <int DCLASS, typename CELL = _Float16>
__global__ __launch_bounds__(csr_max_threads(DCLASS)) void layered_csr_kernel(CsrLayDev g, typename Cell<CELL>::Rec *rec_all, CsrLayArgs A) {
#define LAYERED_CSR_SOFT 0
#define LAYERED_CSR_CONT 0
#include "layered_csr_body.h"
#undef LAYERED_CSR_CONT
#undef LAYERED_CSR_SOFT
}
// the same decode with the soft output S (ldpc_decode_batch_dev_soft): instances of their own beside the eighteen above
template <int DCLASS, typename CELL = _Float16>
__global__ __launch_bounds__(csr_max_threads(DCLASS)) void layered_csr_soft_kernel(CsrLayDev g, typename Cell<CELL>::Rec *rec_all, CsrLayArgs A, CsrSoftArgs S) {
#define LAYERED_CSR_SOFT 1
#define LAYERED_CSR_CONT 0
#include "layered_csr_body.h"
#undef LAYERED_CSR_CONT
#undef LAYERED_CSR_SOFT
}
// the decode that CONTINUES from a decode state and leaves the new state behind (ldpc_decode_batch_dev_continue): a third family of
// instances.  Records are the slot's (K.rec), the prologue adds the slot's sums (K.sum), every sweep reads its records -- the "first sweep
// writes only" branch is not instantiated --, the epilogue writes the new sums for every frame and the soft output when S.out is not null
template <int DCLASS, typename CELL = _Float16>
__global__ __launch_bounds__(csr_max_threads(DCLASS)) void layered_csr_cont_kernel(CsrLayDev g, CsrLayArgs A, CsrSoftArgs S, CsrContArgs K) {
#define LAYERED_CSR_SOFT 1
#define LAYERED_CSR_CONT 1
#include "layered_csr_body.h"
#undef LAYERED_CSR_CONT
#undef LAYERED_CSR_SOFT
}

namespace {

int dclass_of(int max_row_deg) { return max_row_deg <= 8 ? 8 : (max_row_deg <= 20 ? 20 : 32); }
size_t cell_bytes(int dtype) { return dtype == LDPC_F32 ? 4 : dtype == LDPC_I8 ? 1 : 2; }
size_t rec_bytes(int dtype) { return dtype == LDPC_I8 ? sizeof(CsrRecI8) : sizeof(CsrRec); }
size_t lds_bytes_for(const ldpc_code &c, int dtype) { return (((size_t)c.N * cell_bytes(dtype) + 15) & ~(size_t)15) + 32; }

// ------------------------------------------------------------------ THE INSTANCES: 3 families x 3 row classes x 8 cells = 72 kernels.
// Every one is named here and nowhere else; `word` is what the error texts call the family
enum { kPlain = 0, kSoft = 1, kCont = 2 };
const struct { const char *kernel, *word; } kFamily[3] = {{"layered_csr_kernel", ""}, {"layered_csr_soft_kernel", "soft "}, {"layered_csr_cont_kernel", "continuing "}};
// a kernel, launched through hipLaunchKernel, and its name as the demangler writes it (LaunchInfo::name, ldpc_ctx_kernel_name)
struct Instance { const void *kern = nullptr; char name[sizeof(LaunchInfo::name)] = ""; };

template <int DCLASS, typename CELL> const void *kernel_of(int family) {    // family -> kernel template
    return family == kSoft   ? (const void *)layered_csr_soft_kernel<DCLASS, CELL>
           : family == kCont ? (const void *)layered_csr_cont_kernel<DCLASS, CELL> : (const void *)layered_csr_kernel<DCLASS, CELL>;
}
// row class -> DCLASS.  cell: CELL as the demangler writes it, "" where it is the template's default and not written
template <typename CELL> Instance instance(int family, int dclass, const std::string &cell) {
    Instance r;
    r.kern = dclass == 8 ? kernel_of<8, CELL>(family) : dclass == 20 ? kernel_of<20, CELL>(family) : kernel_of<32, CELL>(family);
    snprintf(r.name, sizeof(r.name), "ldpc::%s<%d%s%s>", kFamily[family].kernel, dclass, cell.empty() ? "" : ", ", cell.c_str());
    return r;
}
// dtype -> LT; rule -> cell: the 3/4 LT, scaled Ruled<LT>, A-min* MinStar<LT> -- for float cells only: MinStar<int8_t> is never named, so
// it is not instantiated (select.cc refuses the request; an Instance without a kernel fails its creation)
Instance instance_of(int family, int dclass, int dtype, int rule) {
    auto cell = [&](auto t, const std::string &lt) {
        typedef typename decltype(t)::type LT;
        if (rule == kRule34) return instance<LT>(family, dclass, std::is_same<LT, _Float16>::value ? "" : lt);
        if (rule == kRuleScaled) return instance<Ruled<LT>>(family, dclass, "ldpc::Ruled<" + lt + ">");
        if constexpr (!std::is_same<LT, int8_t>::value) return instance<MinStar<LT>>(family, dclass, "ldpc::MinStar<" + lt + ">");
        else return Instance{};
    };
    return dtype == LDPC_F32 ? cell(Fmt<float>{}, "float") : dtype == LDPC_I8 ? cell(Fmt<int8_t>{}, "signed char") : cell(Fmt<_Float16>{}, "_Float16");
}

// resident workgroups of an instance at T threads and lds bytes of LDS: the attribute that grants it that LDS, its occupancy, the CUs
hipError_t resident_workgroups(const void *kern, int T, size_t lds, int *n) {
    int per_cu = 0, dev = 0;
    hipDeviceProp_t prop;
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, dev);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, T, lds);
    *n = e == hipSuccess ? per_cu * prop.multiProcessorCount : 0;
    return e;
}

// ------------------------------------------------------------------ host side
struct LayeredCsrState : Backend {
    int max_batch = 0, dclass = 8, grid = 0, nslab = 0;
    int dtype = LDPC_F16;       // the lam cell: fp16 (LDPC_F16), float (LDPC_F32) or int8 (LDPC_I8)
    float qscale = 0.f;         // (LDPC_I8) the quantiser's scale
    int has_rule = kRule34;     // a check-node rule other than the 3/4: kRuleScaled, the Ruled instances with `rule`; kRuleAMinStar, the MinStar instances
    CsrRule rule{};
    size_t lds = 0;
    CsrLayDev g{};
    uint16_t *d_cols = nullptr;
    int32_t *d_slab = nullptr, *d_wdeg = nullptr, *d_step = nullptr;
    int *d_counter = nullptr;
    void *rec = nullptr;        // [grid][nslab][T] row records (CsrRec, or CsrRecI8 with int8 lam)
    Instance inst[3];           // by family.  The plain one is set at creation, the others by their first call; info.name is that of the last launch
    int resident[3] = {0, 0, 0};    // resident workgroups of each (0: not asked yet); `grid` is the plain one's, at most max_batch

    ~LayeredCsrState() override {
        (void)hipFree(d_cols); (void)hipFree(d_slab); (void)hipFree(d_wdeg); (void)hipFree(d_step); (void)hipFree(d_counter); (void)hipFree(rec);
    }
    int decode_state_bytes(size_t *rec_b, size_t *sum_b) override {
        *rec_b = rec_bytes(dtype) * (size_t)std::max(nslab, 1) * g.T;
        *sum_b = (dtype == LDPC_I8 ? sizeof(int16_t) : sizeof(float)) * (size_t)g.N;
        return LDPC_OK;
    }
    // What the three decodes share: one launch of the context's instance of `family`, with the same tables, counter and geometry.  so, k: the
    // family's further arguments (null where it has none)
    int run(int family, hipStream_t st, int max_iters, int batch, const void *d_llr, int llr_fmt, uint8_t *d_bits, int32_t *d_iters, uint8_t *d_conv,
            double *d_final, CsrSoftArgs *so, CsrContArgs *k) {
        if (llr_fmt == LLR_I8 && dtype != LDPC_I8) return set_error(LDPC_EUNSUPPORTED, "int8 LLRs are taken by LDPC_I8 contexts only");
        Instance &in = inst[family];
        if (!resident[family]) {        // asked for once
            in = instance_of(family, dclass, dtype, has_rule);
            const hipError_t e = resident_workgroups(in.kern, g.T, lds, &resident[family]);
            if (e != hipSuccess) return set_error(LDPC_EHIP, "layered_csr %sinstance: %s", kFamily[family].word, hipGetErrorString(e));
            if (resident[family] <= 0) return set_error(LDPC_EHIP, "layered_csr: no workgroup of %d threads and %zu B of LDS of the %sinstance is resident", g.T, lds, kFamily[family].word);
        }
        // the plain and the soft instance write the context's records, sized for `grid` workgroups; the continuing one writes the state's
        const int bound = family == kPlain ? grid : family == kSoft ? std::min(grid, resident[kSoft]) : resident[kCont];
        CsrLayArgs a{};
        a.llr = d_llr; a.llr_fmt = llr_fmt; a.qscale = qscale; a.bits = d_bits; a.iters = d_iters; a.conv = d_conv; a.final_lam = d_final;
        a.batch = batch; a.max_iters = max_iters; a.work_counter = d_counter; a.rule = rule;
        hipError_t e = hipMemsetAsync(d_counter, 0, sizeof(int), st);
        if (e != hipSuccess) return set_error(LDPC_EHIP, "layered_csr: %s", hipGetErrorString(e));
        void *args[3][4] = {{&g, &rec, &a, nullptr}, {&g, &rec, &a, so}, {&g, &a, so, k}};     // the continuing kernel takes no `rec`
        memcpy(info.name, in.name, sizeof(info.name));
        if (timer) timer->begin(st);
        (void)hipLaunchKernel(in.kern, dim3(std::min(batch, bound)), dim3(g.T), args[family], lds, st);
        if (timer) timer->end(st);
        e = hipGetLastError();
        if (e != hipSuccess) return set_error(LDPC_EHIP, "layered_csr %slaunch: %s", kFamily[family].word, hipGetErrorString(e));
        return LDPC_OK;
    }
    int decode(hipStream_t st, int max_iters, int batch, const void *d_llr, int llr_fmt, uint8_t *d_bits, int32_t *d_iters,
               uint8_t *d_conv, double *d_final, double *d_trace) override {
        if (d_trace) return set_error(LDPC_EUNSUPPORTED, has_rule == kRuleAMinStar ? "layered_csr: no per-sweep trace with a check-node rule (cn_rule = LDPC_CN_AMINSTAR; decode without one)" : has_rule ? "layered_csr: no per-sweep trace with a check-node rule (cn_scale / cn_offset; decode without one)" : "layered_csr: no per-sweep trace (decode without one)");
        return run(kPlain, st, max_iters, batch, d_llr, llr_fmt, d_bits, d_iters, d_conv, d_final, nullptr, nullptr);
    }
    // The soft instance of the context's kernel: same tables, records, counter and geometry.  It holds more registers than the plain one in
    // its epilogue only; its grid is bounded by the records the context owns (sized for the plain instance's resident workgroups) and by its
    // own residency.
    int decode_soft(hipStream_t st, int max_iters, int batch, const void *d_llr, int llr_fmt, uint8_t *d_bits, int32_t *d_iters,
                    uint8_t *d_conv, void *d_soft, int soft_fmt, float soft_qscale, int soft_kind) override {
        CsrSoftArgs so{d_soft, soft_fmt, soft_kind, soft_qscale};
        return run(kSoft, st, max_iters, batch, d_llr, llr_fmt, d_bits, d_iters, d_conv, nullptr, &so, nullptr);
    }
    // The continuing instance of the context's kernel: same tables, counter and geometry; its records and sums are the state's slots
    // first .. first + batch - 1 (st_rec, st_sum: slot 0), so its grid is bounded by its own residency alone.
    int decode_continue(hipStream_t st, void *st_rec, void *st_sum, int first, int max_iters, int batch, const void *d_llr, int llr_fmt, uint8_t *d_bits,
                        int32_t *d_iters, uint8_t *d_conv, void *d_soft, int soft_fmt, float soft_qscale, int soft_kind) override {
        CsrSoftArgs so{d_soft, soft_fmt, soft_kind, soft_qscale};
        CsrContArgs k{st_rec, st_sum, first};
        return run(kCont, st, max_iters, batch, d_llr, llr_fmt, d_bits, d_iters, d_conv, nullptr, &so, &k);
    }
    int step(hipStream_t, int, const double *, const double *, const double *, double *, double *, uint8_t *) override {
        if (has_rule == kRuleAMinStar) return set_error(LDPC_EUNSUPPORTED, "no teacher-forced step with a check-node rule (cn_rule = LDPC_CN_AMINSTAR: the record kernels keep no per-edge messages)");
        if (has_rule) return set_error(LDPC_EUNSUPPORTED, "no teacher-forced step with a check-node rule (cn_scale / cn_offset: the record kernels keep no per-edge messages)");
        return set_error(LDPC_EUNSUPPORTED, dtype == LDPC_I8 ? "no teacher-forced step with LDPC_I8 (fixed-point state; the record kernels keep no per-edge messages)"
                                            : dtype == LDPC_F32 ? "no teacher-forced step on the on-chip layered kernel for any H (the record kernels keep no per-edge messages)"
                                                                : "no teacher-forced step with fp16 lam storage (the record kernels keep no per-edge messages)");
    }
    bool reads_llr_once(int) const override { return true; }
};

}  // namespace

const char *layered_csr_why_not(const ldpc_code &c, int variant, int dtype) {
    if (variant != LDPC_MINSUM) return "the on-chip layered kernel for any H implements min-sum";
    if (dtype != LDPC_F16 && dtype != LDPC_F32 && dtype != LDPC_I8) return "the on-chip layered kernel for any H stores lam in fp16 (LDPC_F16), in f32 (LDPC_F32) or in int8 (LDPC_I8)";
    if (c.max_row_deg > 27) return "check rows above weight 27 (a row record holds 27 sign bits)";
    if (dtype != LDPC_I8 && lds_bytes_for(c, dtype) > 160 * 1024) return dtype == LDPC_F32 ? "a frame's f32 LLRs exceed the 160 KB of LDS" : "a frame's fp16 LLRs exceed the 160 KB of LDS";
    if (c.N > 65535) return "more than 65 535 columns (16-bit column table)";
    const char *e = getenv("LDPC_LAYERED_CSR");
    if (e && !strcmp(e, "0")) return "disabled (LDPC_LAYERED_CSR=0)";
    return nullptr;
}

// The graph work -- steps, slabs, the column table -- is csrc/layered_csr_layout.cc; here are the decisions that need the device: T, the
// allocations and uploads, the resident workgroups
Backend *layered_csr_create(const ldpc_code &c, int dtype, int max_batch, float qscale, const CnRule *cn) {
    LayeredCsrState *s = new (std::nothrow) LayeredCsrState();
    if (!s) { set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    try {
        // lam stays on-chip for the whole decode in one launch (only the row records travel to HBM): reported as the on-chip path
        s->path = LDPC_PATH_FUSED;
        s->max_batch = max_batch; s->dclass = dclass_of(c.max_row_deg); s->dtype = dtype; s->qscale = qscale;
        if (cn && cn->kind == LDPC_CN_AMINSTAR) s->has_rule = kRuleAMinStar;
        else if (cn) { s->has_rule = kRuleScaled; s->rule.scale = cn->scale; s->rule.offset = cn->offset; s->rule.a = cn->a; s->rule.b = cn->b; }
        const CsrSteps steps = csr_layout_steps(c.N, c.row_ptr.data(), c.col_idx.data(), c.layer_ptr.data(), (int)c.layer_ptr.size() - 1);
        int T = (int)std::min<size_t>(csr_max_threads(s->dclass), (steps.rmax + 63) / 64 * 64);
        s->lds = lds_bytes_for(c, dtype);
        s->inst[kPlain] = instance_of(kPlain, s->dclass, dtype, s->has_rule);
        const void *kern = s->inst[kPlain].kern;
        hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s->lds);
        // int8 lam: a frame of N = 64 800 takes 64.8 KB of LDS, so two workgroups fit a CU -- when the registers allow it.  1024 threads
        // at more than 64 VGPRs fill the CU's register files alone; 512 threads leave room for a second workgroup, whose rows run
        // while the first waits at a barrier.  Taken when it at least doubles the resident workgroups; the slabs only regroup rows
        // of one step (column-disjoint), so the results do not depend on it.  The choice is to rest on the measurement that
        // tools/layered_csr_rate.py --lam i8 makes of both sizes (LDPC_LAYERED_CSR_THREADS forces one); until that has been run on an
        // MI355X it rests on this occupancy arithmetic alone.
        if (dtype == LDPC_I8 && T > 512 && e == hipSuccess) {
            int occ_t = 0, occ_half = 0;
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_t, kern, T, s->lds);
            if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_half, kern, 512, s->lds);
            if (e == hipSuccess && occ_half >= 2 * std::max(occ_t, 1)) T = 512;
        }
        if (const char *force = getenv("LDPC_LAYERED_CSR_THREADS")) {      // A/B switch (any lam type): a multiple of 64 within the instance's bound
            const int t = atoi(force);
            if (t >= 64 && t % 64 == 0 && t <= csr_max_threads(s->dclass)) T = t;
        }
        const CsrLayout lay = csr_layout_pack(steps, c.row_ptr.data(), c.col_idx.data(), T);
        s->nslab = lay.nslab;
        s->g.N = c.N; s->g.T = T; s->g.nstep = (int)steps.rows.size();
        if (e == hipSuccess) e = resident_workgroups(kern, T, s->lds, &s->resident[kPlain]);
        if (e == hipSuccess && s->resident[kPlain] <= 0) { set_error(LDPC_EHIP, "layered_csr: no workgroup of %d threads and %zu B of LDS is resident", T, s->lds); delete s; return nullptr; }
        if (e == hipSuccess) s->grid = std::min(max_batch, s->resident[kPlain]);
        if (e == hipSuccess) e = hipMalloc((void **)&s->d_cols, sizeof(uint16_t) * std::max<size_t>(lay.cols.size(), 1));
        if (e == hipSuccess) e = hipMalloc((void **)&s->d_slab, sizeof(int32_t) * std::max<size_t>(lay.slab.size(), 2));
        if (e == hipSuccess) e = hipMalloc((void **)&s->d_wdeg, sizeof(int32_t) * std::max<size_t>(lay.wdeg.size(), 1));
        if (e == hipSuccess) e = hipMalloc((void **)&s->d_step, sizeof(int32_t) * lay.step_ptr.size());
        if (e == hipSuccess) e = hipMalloc((void **)&s->d_counter, sizeof(int));
        if (e == hipSuccess) e = hipMalloc(&s->rec, rec_bytes(dtype) * (size_t)s->grid * std::max(s->nslab, 1) * T);
        if (e == hipSuccess && !lay.cols.empty()) e = hipMemcpy(s->d_cols, lay.cols.data(), sizeof(uint16_t) * lay.cols.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess && !lay.slab.empty()) e = hipMemcpy(s->d_slab, lay.slab.data(), sizeof(int32_t) * lay.slab.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess && !lay.wdeg.empty()) e = hipMemcpy(s->d_wdeg, lay.wdeg.data(), sizeof(int32_t) * lay.wdeg.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(s->d_step, lay.step_ptr.data(), sizeof(int32_t) * lay.step_ptr.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            set_error(e == hipErrorOutOfMemory ? LDPC_ENOMEM : LDPC_EHIP, "layered_csr_create (%d workgroups x %zu bytes of records): %s", s->grid,
                      rec_bytes(dtype) * (size_t)s->nslab * T, hipGetErrorString(e));
            delete s;
            return nullptr;
        }
        s->g.cols = s->d_cols; s->g.slab = s->d_slab; s->g.wdeg = s->d_wdeg; s->g.step_ptr = s->d_step;
        memcpy(s->info.name, s->inst[kPlain].name, sizeof(s->info.name));
        s->info.threads = T; s->info.frames_per_wg = 1;
        return s;
    } catch (...) { delete s; set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
}

}  // namespace ldpc
