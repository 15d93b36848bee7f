// demap_rm.hip -- the receive side of rate matching and HARQ: the max-log soft demapper summing through a table whose entries may repeat
// (ldpc_demap_dev_rm), optionally onto the soft buffer of earlier rounds, and the table alone on LLRs (ldpc_ratematch_llr_dev).  I/Q
// samples [batch][ceil(E / m)][2] (and a power gain per symbol) -> LLRs [batch][N] in the decoders' input formats, one pass, no memset
// before it and no atomic in it.  The table: ratematch.h; the rule is restated in tests/ratematch_spec.py.
// LANE = CODEWORD ELEMENT (frame f, position c): a GATHER.  The lane walks its list inv_t[inv_ptr[c] .. inv_ptr[c + 1]) of transmitted
// indices, ascending; for each t it loads the sample of symbol t / m (m a template argument) and its gain, evaluates the LLR of bit
// t % m ALONE, and adds in float32, left to right: one defined order, where the lane = symbol scatter of demap_il.hip would need atomics
// (no order, and the fp16 and int8 buffers saturate).  The lane is the only one that touches its element:
//   accumulate = 0: every element of [batch][N] is written exactly once and none is read; a position nothing names gets 0;
//   accumulate = 1: an element that some t names is read once and then written once (int8 with a NaN sum: read, not written: the
//                   buffer keeps its value); an element nothing names is neither read nor written.
// THE LLR OF ONE BIT is the value demap.h demap_llrs / demap_product.h axis_llrs give it, bit for bit: the same distances in the same
// float32 operations, and two running minima m0 / m1 over them, a distance entering the one its label's bit selects (the other takes
// +inf).  A min of floats is exact in any order.  A NaN sample leaves both minima +inf, and inf - inf = NaN as there.  The price of the
// gather: the distances of a symbol are computed again by the lane of each of its bits (2^m a bit for a table object, 2^b for a product
// object) -- profiles/r18_ratematch.txt has what that costs.
// The constellation rides in the kernel arguments (scalar loads), as demap.hip.  The walk is a loop, and inside a loop the compiler
// hoists those loads out as invariants and spills the scalar registers (demap_product.hip): the table is indexed with a zero that an
// empty asm statement hides from the optimiser in every turn, so the loads stay where they are used.
// Lanes of a wave may walk lists of different lengths; the wave runs the longest.  For a circular table consecutive c have consecutive
// t, hence the same or neighbouring samples, and equal lengths up to one.
// ONE ITEM A LANE, no grid-stride loop, as demap_il.hip.
// THE LOG-MAP RULE (demap.h DEMAP_LOGMAP, a template argument of the two rules below): a second walk over the same distances adds the
// exponentials of the bit's two subsets, 2^m (2^b) a bit; the value then enters the sum and the store exactly as a max-log one.
#include "demap_product.h"
#include "fading.h"
#include "mod_dispatch.h"
#include "ratematch.h"

namespace ldpc {

constexpr float kRmInf = __builtin_inff();

// a zero the optimiser cannot see through, in a scalar register
static __device__ __forceinline__ int rm_hidden_zero() {
    int z = 0;
    __asm__ volatile("" : "+s"(z));
    return z;
}

// the LLR of transmitted bit t of frame f, a table object of M bits: bit j = t % M (the first one the MSB) of symbol s = t / M
template <int M, int RULE>
struct RmTableRule {
    ModTab tab;
    const float *sym, *gain;   // gain may be null: inv_s = inv
    int n_sym;
    float inv;
    __device__ __forceinline__ float operator()(size_t f, int t) const {
        const uint32_t s = (uint32_t)t / (uint32_t)M, j = (uint32_t)t - s * (uint32_t)M;
        const size_t at = f * (size_t)n_sym + s;
        const float2 y = *reinterpret_cast<const float2 *>(sym + 2 * at);
        const float inv_s = gain ? fade_inv(inv, gain[at]) : inv;
        const uint32_t mask = 1u << (M - 1 - j);
        const int z = rm_hidden_zero();
        float m0 = kRmInf, m1 = kRmInf;
#pragma unroll
        for (int p = 0; p < (1 << M); p++) {
            const float dx = y.x - tab.pt[p + z][0], dy = y.y - tab.pt[p + z][1];
            const float d = dx * dx + dy * dy;
            const bool one = (mask & (uint32_t)p) != 0u;
            m0 = __builtin_fminf(m0, one ? kRmInf : d);
            m1 = __builtin_fminf(m1, one ? d : kRmInf);
        }
        if constexpr (RULE == DEMAP_MAXLOG || M == 1) return (m0 - m1) * inv_s;
        // log-MAP (demap.h demap_llrs_logmap, this bit alone): a second walk over the table, behind a hidden zero of its own, adds
        // exp(-(d_p - m_v) inv_s) to the sum its label's bit selects; the other sum takes a +0, which changes no sum.  16 points at a
        // time in a loop that is NOT unrolled, as RmProductRule: with the first walk's minima live, the 128 coordinates of m = 6 at
        // once do not fit the scalar registers
        constexpr int CH = (1 << M) < 16 ? (1 << M) : 16;
        float s0 = 0.f, s1 = 0.f;
#pragma unroll 1
        for (int p0 = rm_hidden_zero(); p0 < (1 << M); p0 += CH) {
#pragma unroll
            for (int p = 0; p < CH; p++) {
                const float dx = y.x - tab.pt[p0 + p][0], dy = y.y - tab.pt[p0 + p][1];
                const float d = dx * dx + dy * dy;
                const bool one = (mask & (uint32_t)(p0 + p)) != 0u;
                const float e = __expf(((one ? m1 : m0) - d) * inv_s);
                s0 += one ? 0.f : e;
                s1 += one ? e : 0.f;
            }
        }
        return logmap_llr((m0 - m1) * inv_s, s0, s1);
    }
};

// the same of a product object of B bits an axis: bits 0 .. B - 1 of a symbol are the I axis's, B .. 2 B - 1 the Q axis's
template <int B, int RULE>
struct RmProductRule {
    AxisTab tab;
    const float *sym, *gain;
    int n_sym;
    float inv;
    __device__ __forceinline__ float operator()(size_t f, int t) const {
        constexpr uint32_t M = 2 * B;
        const uint32_t s = (uint32_t)t / M, j = (uint32_t)t - s * M;
        const bool q = j >= (uint32_t)B;
        const size_t at = f * (size_t)n_sym + s;
        const float y = sym[2 * at + (q ? 1 : 0)];
        const float inv_s = gain ? fade_inv(inv, gain[at]) : inv;
        const uint32_t mask = 1u << (B - 1 - (q ? j - (uint32_t)B : j));
        const int z = rm_hidden_zero();
        float m0 = kRmInf, m1 = kRmInf;
        // the axis is the lane's, so the levels of BOTH axes are loaded and one is selected: 16 levels an axis at a time, in a loop that
        // is NOT unrolled, keep that inside the scalar registers for b = 5 and 6
        constexpr int CH = (1 << B) < 16 ? (1 << B) : 16;
#pragma unroll 1
        for (int l0 = z; l0 < (1 << B); l0 += CH) {
#pragma unroll
            for (int l = 0; l < CH; l++) {
                const float dx = y - (q ? tab.lev[1][l0 + l] : tab.lev[0][l0 + l]);
                const float d = dx * dx;
                const bool one = (mask & (uint32_t)(l0 + l)) != 0u;
                m0 = __builtin_fminf(m0, one ? kRmInf : d);
                m1 = __builtin_fminf(m1, one ? d : kRmInf);
            }
        }
        if constexpr (RULE == DEMAP_MAXLOG || B == 1) return (m0 - m1) * inv_s;
        // log-MAP (demap_product.h axis_llrs_logmap, this bit alone): the same chunked walk again, as RmTableRule's second one
        float s0 = 0.f, s1 = 0.f;
#pragma unroll 1
        for (int l0 = rm_hidden_zero(); l0 < (1 << B); l0 += CH) {
#pragma unroll
            for (int l = 0; l < CH; l++) {
                const float dx = y - (q ? tab.lev[1][l0 + l] : tab.lev[0][l0 + l]);
                const float d = dx * dx;
                const bool one = (mask & (uint32_t)(l0 + l)) != 0u;
                const float e = __expf(((one ? m1 : m0) - d) * inv_s);
                s0 += one ? 0.f : e;
                s1 += one ? e : 0.f;
            }
        }
        return logmap_llr((m0 - m1) * inv_s, s0, s1);
    }
};

// the table alone: the LLR of transmitted bit t is element t of the caller's row
struct RmLoadRule {
    const float *llr_tx;
    int E;
    __device__ __forceinline__ float operator()(size_t f, int t) const { return llr_tx[f * (size_t)E + t]; }
};

// the sum v of a position into its element.  accumulate = 0: llr_out.  accumulate = 1, onto the element's value `old`:
//   float32  fl(old + v);   fp16  llr_out of fl(f32(old) + v): clamped to +-65504, a NaN stays;
//   int8     clip(rint(fl(f32(old) + fl(v qs))), -127, 127); a NaN v (the only way to a NaN here) writes nothing: an erasure, as the
//            quantiser's NaN -> 0
template <typename OT> __device__ __forceinline__ void rm_store(OT *dst, float v, float qs, bool acc);
template <> __device__ __forceinline__ void rm_store<float>(float *dst, float v, float, bool acc) {
    if (acc) v = *dst + v;
    *dst = v;
}
template <> __device__ __forceinline__ void rm_store<__half>(__half *dst, float v, float qs, bool acc) {
    if (acc) v = __half2float(*dst) + v;
    *dst = llr_out<__half>(v, qs);
}
template <> __device__ __forceinline__ void rm_store<int8_t>(int8_t *dst, float v, float qs, bool acc) {
    if (!acc) {
        *dst = llr_out<int8_t>(v, qs);
    } else {
        const float r = __builtin_rintf((float)*dst + v * qs);
        if (r == r) *dst = (int8_t)(int)__builtin_amdgcn_fmed3f(r, -127.f, 127.f);
    }
}

template <class RULE, typename OT>
__global__ __launch_bounds__(256) void rm_gather_kernel(RULE rule, RmTab rm, OT *llr, size_t total, float qs, int acc) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)rm.N;
        const int c = (int)(i - f * (size_t)rm.N);
        const int beg = rm.inv_ptr[c], end = rm.inv_ptr[c + 1];
        if (beg == end) {
            if (!acc) llr[i] = llr_out<OT>(0.f, qs);
        } else {
            float v = 0.f;
            for (int k = beg; k < end; k++) {
                const float l = rule(f, rm.inv_t[k]);
                v = k == beg ? l : v + l;                 // (not 0 + l: that would turn a -0 into +0)
            }
            rm_store<OT>(llr + i, v, qs, acc != 0);
        }
    }
}

template <class RULE>
static int rm_launch(const char *what, hipStream_t st, const RULE &rule, const RmTab &rm, int batch, void *d_llr, int fmt, float qs, bool acc) {
    const size_t total = (size_t)batch * (size_t)rm.N;
    const int rc = check_items(what, (size_t)batch * (size_t)std::max(rm.E, rm.N));
    if (rc != LDPC_OK) return rc;
    return launched(what, dispatch_fmt(fmt, [&](auto t) {
        typedef typename decltype(t)::type OT;
        hipLaunchKernelGGL((rm_gather_kernel<RULE, OT>), grid_lanes(total), dim3(256), 0, st, rule, rm, (OT *)d_llr, total, qs, (int)acc);
        return LDPC_OK;
    }));
}

int demap_rm_launch(hipStream_t st, const ModTab &tab, int m, int rule, const RmTab &rm, int batch, const float *d_sym, const float *d_gain, float inv, void *d_llr, int fmt,
                    float qscale, bool accumulate) {
    const char *what = "ldpc_demap_dev_rm";
    return dispatch_rule(rule, [&](auto r) { return dispatch_bits(what, m, [&](auto k) {
        constexpr int M = decltype(k)::value;
        const RmTableRule<M, decltype(r)::value> lane{tab, d_sym, d_gain, mod_symbols(rm.E, M), inv};
        return rm_launch(what, st, lane, rm, batch, d_llr, fmt, qscale, accumulate);
    }); });
}

int demap_rm_product_launch(hipStream_t st, const AxisTab &tab, int b, int rule, const RmTab &rm, int batch, const float *d_sym, const float *d_gain, float inv, void *d_llr,
                            int fmt, float qscale, bool accumulate) {
    const char *what = "ldpc_demap_dev_rm";
    return dispatch_rule(rule, [&](auto r) { return dispatch_bits(what, b, [&](auto k) {
        constexpr int B = decltype(k)::value;
        const RmProductRule<B, decltype(r)::value> lane{tab, d_sym, d_gain, mod_symbols(rm.E, 2 * B), inv};
        return rm_launch(what, st, lane, rm, batch, d_llr, fmt, qscale, accumulate);
    }); });
}

int ratematch_llr_launch(hipStream_t st, const RmTab &rm, int batch, const float *d_llr_tx, void *d_llr, int fmt, float qscale, bool accumulate) {
    const RmLoadRule rule{d_llr_tx, rm.E};
    return rm_launch("ldpc_ratematch_llr_dev", st, rule, rm, batch, d_llr, fmt, qscale, accumulate);
}

}  // namespace ldpc
