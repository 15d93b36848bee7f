// demap.h -- the modulation object and the device functions of the mapper and the max-log soft demapper, shared by the stand-alone
// demapper (demap.hip) and the frame source's modulated path (sim_mod.hip): one copy of the symbol rule and of the LLR rule, so the
// fused kernel equals the two-step one bit for bit.  The rule is restated in tests/modulation_spec.py.  The stand-alone demappers also
// hold the exact (log-MAP) rule, chosen by the modulation object's `rule` (demap_llrs_logmap below; tests/demap_logmap_spec.py).
#pragma once
#include "internal.h"
#ifdef __HIPCC__
#include <hip/hip_fp16.h>
#endif

namespace ldpc {
constexpr int kModMaxBits = 6, kModMaxPoints = 1 << kModMaxBits;
// the constellation as a kernel argument: wave-uniform, so the instances template on m read their 2^m points through scalar loads
// from the kernel-argument segment and never per lane
struct ModTab {
    float pt[kModMaxPoints][2];   // [label]: I, Q; entries >= 2^m are not read
};
enum { MOD_LLR_F32 = 0, MOD_LLR_F16 = 1, MOD_LLR_I8 = 2 };   // = LDPC_LLR_*
// most kernels of the modulation files work ONE item a lane, with no grid-stride loop (demap_product.hip says why): their launch grid is
// ceil(items / 256) blocks, and their launchers refuse more items than a grid of 2^32 - 1 lanes holds (mod_dispatch.h check_items)
constexpr size_t kLaneMaxItems = 0xffffffffull - 255;
// a product constellation (I-axis levels x Q-axis levels, label = I-label << b | Q-label) as a kernel argument: the two level tables,
// 512 bytes as ModTab, for up to 6 bits an axis (4096 points).  Its device functions and kernels: demap_product.h, demap_product.hip,
// sim_mod_product.hip
constexpr int kAxisMaxBits = 6, kAxisMaxLevels = 1 << kAxisMaxBits;
struct AxisTab {
    float lev[2][kAxisMaxLevels];   // [axis: I, Q][axis label]; entries >= 2^b are not read
};

// d_llr [batch][N] <- the LLRs of d_sym [batch][n_sym][2]; inv = float32(1 / (2 sigma^2))
int demap_launch(hipStream_t st, const ModTab &tab, int m, int rule, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, int fmt, float qscale);
// d_cw: packed codewords [batch][PB] (bit i in byte i / 8 at bit i % 8, pad bits 0).  d_sym [batch][n_sym][2] <- the noisy symbols
int mod_transmit_launch(hipStream_t st, const ModTab &tab, int m, int batch, int n_tx, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg,
                        float *d_sym);
// the two in one kernel: the samples stay in registers
int mod_generate_launch(hipStream_t st, const ModTab &tab, int m, int batch, int n_tx, int N, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg,
                        float inv, void *d_llr, int fmt, float qscale);

// the same three for a product constellation of b bits an axis (m = 2 b)
int demap_product_launch(hipStream_t st, const AxisTab &tab, int b, int rule, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, int fmt, float qscale);
int product_transmit_launch(hipStream_t st, const AxisTab &tab, int b, int batch, int n_tx, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg,
                            float *d_sym);
int product_generate_launch(hipStream_t st, const AxisTab &tab, int b, int batch, int n_tx, int N, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame,
                            float sg, float inv, void *d_llr, int fmt, float qscale);

#ifdef __HIPCC__
// constellation point of a per-lane label: a binary select tree over the uniform table (2^M - 1 selects per coordinate), label bit 0
// first -- no per-lane table read
template <int M>
__device__ __forceinline__ void mod_point(const ModTab &tab, uint32_t label, float &cI, float &cQ) {
    float vi[1 << M], vq[1 << M];
#pragma unroll
    for (int p = 0; p < (1 << M); p++) { vi[p] = tab.pt[p][0]; vq[p] = tab.pt[p][1]; }
#pragma unroll
    for (int lev = 0; lev < M; lev++) {
        const bool one = (label >> lev) & 1u;
#pragma unroll
        for (int p = 0; p < (1 << (M - 1 - lev)); p++) {
            vi[p] = one ? vi[2 * p + 1] : vi[2 * p];
            vq[p] = one ? vq[2 * p + 1] : vq[2 * p];
        }
    }
    cI = vi[0]; cQ = vq[0];
}

// label of symbol s of a packed codeword row: bits M s .. M s + M - 1, the first one the MSB; positions >= n_tx are pad bits, 0 in the row
template <int M>
__device__ __forceinline__ uint32_t mod_label(const uint8_t *__restrict__ row, int PB, int s) {
    const int first = M * s, b0 = first >> 3;
    uint32_t w = b0 < PB ? row[b0] : 0u;
    if (M > 1 && b0 + 1 < PB) w |= (uint32_t)row[b0 + 1] << 8;      // (7 + 6 bits at the most: two bytes)
    w >>= first & 7;
    uint32_t label = 0u;
#pragma unroll
    for (int j = 0; j < M; j++) label |= ((w >> j) & 1u) << (M - 1 - j);
    return label;
}

// the channel: y = fl(c + fl(sg z)) per coordinate
template <int M>
__device__ __forceinline__ void mod_symbol(const ModTab &tab, uint32_t label, float zI, float zQ, float sg, float &yI, float &yQ) {
    float cI, cQ;
    mod_point<M>(tab, label, cI, cQ);
    yI = cI + sg * zI;
    yQ = cQ + sg * zQ;
}

// max-log LLRs of one sample: llr[j] = fl(fl(m0_j - m1_j) inv), m0_j / m1_j = the smallest squared distance to a point whose label bit
// j (MSB first) is 0 / 1.  p and j are constants after unrolling: every distance feeds exactly M mins, no selects.  A NaN sample makes
// every distance NaN, and min(NaN, NaN) = NaN: NaN LLRs
template <int M>
__device__ __forceinline__ void demap_llrs(const ModTab &tab, float yI, float yQ, float inv, float (&llr)[M]) {
    float m0[M], m1[M];
#pragma unroll
    for (int p = 0; p < (1 << M); p++) {
        const float dx = yI - tab.pt[p][0], dy = yQ - tab.pt[p][1];
        const float d = dx * dx + dy * dy;
#pragma unroll
        for (int j = 0; j < M; j++) {
            const int bit = (p >> (M - 1 - j)) & 1;
            if (bit) m1[j] = (p == (1 << (M - 1 - j))) ? d : __builtin_fminf(m1[j], d);
            else m0[j] = (p == 0) ? d : __builtin_fminf(m0[j], d);
        }
    }
#pragma unroll
    for (int j = 0; j < M; j++) llr[j] = (m0[j] - m1[j]) * inv;
}

// the log-MAP correction of one bit from the two sums of its subsets: c1 - c0, c_v = log(sum_v).  Every sum holds an exp(0) = 1, so it
// lies in [1, 2^(M-1)] and no log sees a 0.  Where the correction is zero (single-point subsets; high SNR, where every other term has
// underflowed; a scale of 0, where both sums are the same integer) the max-log value stands as it is, the sign of a zero included:
// -0 + 0 would be +0.  A NaN correction is not zero and makes the LLR NaN
__device__ __forceinline__ float logmap_llr(float maxlog, float s0, float s1) {
    const float corr = __logf(s1) - __logf(s0);
    return corr != 0.f ? maxlog + corr : maxlog;
}

// log-MAP LLRs of one sample (include/ldpc_hip.h, "The LLR rule"): the max-log value of demap_llrs, bit for bit, plus c1 - c0,
// c_v = log(sum over the points p whose bit j is v of exp(-(d_p - m_v) inv)).  Two passes: the minima, then the M 2^M exponentials;
// the second pass computes the distances again from the uniform table (5 operations a point beside M exponentials) -- the same
// float32 operations, hence the same values -- where keeping them would hold 2^M registers across it.  The sums run in label order
template <int M>
__device__ __forceinline__ void demap_llrs_logmap(const ModTab &tab, float yI, float yQ, float inv, float (&llr)[M]) {
    float m0[M], m1[M], s0[M], s1[M];
#pragma unroll
    for (int p = 0; p < (1 << M); p++) {
        const float dx = yI - tab.pt[p][0], dy = yQ - tab.pt[p][1];
        const float d = dx * dx + dy * dy;
#pragma unroll
        for (int j = 0; j < M; j++) {
            const int bit = (p >> (M - 1 - j)) & 1;
            if (bit) m1[j] = (p == (1 << (M - 1 - j))) ? d : __builtin_fminf(m1[j], d);
            else m0[j] = (p == 0) ? d : __builtin_fminf(m0[j], d);
        }
    }
    if constexpr (M == 1) {                               // one point a subset: both sums are exp(0)
        llr[0] = (m0[0] - m1[0]) * inv;
        return;
    }
#pragma unroll
    for (int p = 0; p < (1 << M); p++) {
        const float dx = yI - tab.pt[p][0], dy = yQ - tab.pt[p][1];
        const float d = dx * dx + dy * dy;
#pragma unroll
        for (int j = 0; j < M; j++) {
            const int bit = (p >> (M - 1 - j)) & 1;
            const float e = __expf((bit ? m1[j] - d : m0[j] - d) * inv);
            if (bit) s1[j] = (p == (1 << (M - 1 - j))) ? e : s1[j] + e;
            else s0[j] = (p == 0) ? e : s0[j] + e;
        }
    }
#pragma unroll
    for (int j = 0; j < M; j++) llr[j] = logmap_llr((m0[j] - m1[j]) * inv, s0[j], s1[j]);
}

// the LLRs of one sample by the rule of the modulation object (LDPC_DEMAP_MAXLOG = 0, LDPC_DEMAP_LOGMAP = 1): a template argument of
// every demapper kernel, so a max-log instance holds demap_llrs alone, as before the rule existed
enum { DEMAP_MAXLOG = 0, DEMAP_LOGMAP = 1 };
template <int M, int RULE>
__device__ __forceinline__ void demap_llrs_by(const ModTab &tab, float yI, float yQ, float inv, float (&llr)[M]) {
    if constexpr (RULE == DEMAP_LOGMAP) demap_llrs_logmap<M>(tab, yI, yQ, inv, llr);
    else demap_llrs<M>(tab, yI, yQ, inv, llr);
}

// one output element in the decoder's input formats
template <typename OT> __device__ __forceinline__ OT llr_out(float v, float qs);
template <> __device__ __forceinline__ float llr_out<float>(float v, float) { return v; }
template <> __device__ __forceinline__ __half llr_out<__half>(float v, float) {   // round_f16 of sim_frame_kernel, written with compares: a NaN
    const float c = v < -65504.f ? -65504.f : (v > 65504.f ? 65504.f : v);           // fails both and passes (fmaxf(NaN, x) would give x)
    return __float2half_rn(c);
}
template <> __device__ __forceinline__ int8_t llr_out<int8_t>(float v, float qs) {   // = quant_i8 of layered_csr.hip, tests/layered_i8_spec.quantize
    const float r = __builtin_rintf(v * qs);
    return r != r ? (int8_t)0 : (int8_t)(int)__builtin_amdgcn_fmed3f(r, -127.f, 127.f);
}

// the vector store of a lane's M consecutive elements exists where M sizeof(OT) is 4, 8 or 16 bytes (f32: M = 2, 4; fp16: 2, 4; int8: 4)
template <int M, typename OT> constexpr bool kDemapVec = M > 1 && (M * sizeof(OT) == 4 || M * sizeof(OT) == 8 || M * sizeof(OT) == 16);
template <int BYTES> struct VecOf;
template <> struct VecOf<4> { typedef uint32_t type; };
template <> struct VecOf<8> { typedef uint2 type; };
template <> struct VecOf<16> { typedef uint4 type; };

// slot s of a row of N elements = elements M s .. M s + M - 1: the LLRs of symbol s below n_tx, 0 from n_tx on, nothing from N on.
// VEC (the host grants it when N % M == 0 and the buffer is aligned to M elements): one store; otherwise element stores
template <int M, typename OT, bool VEC>
__device__ __forceinline__ void store_slot(OT *__restrict__ row, int s, int n_tx, int N, const float (&llr)[M], float qs) {
    const int e0 = M * s;
    OT v[M];
#pragma unroll
    for (int j = 0; j < M; j++) v[j] = llr_out<OT>(e0 + j < n_tx ? llr[j] : 0.f, qs);
    if constexpr (VEC) {
        typedef typename VecOf<M * sizeof(OT)>::type V;
        V pack;
        __builtin_memcpy(&pack, v, sizeof(V));
        *reinterpret_cast<V *>(row + e0) = pack;
    } else {
#pragma unroll
        for (int j = 0; j < M; j++)
            if (e0 + j < N) row[e0 + j] = v[j];
    }
}
#endif  // __HIPCC__
}  // namespace ldpc

// (host) the object behind include/ldpc_hip.h ldpc_modulation
struct ldpc_modulation {
    int m = 0;
    ldpc::ModTab tab{};   // a table object (b == 0)
    double es = 0.0;
    int b = 0;            // a product object: bits per axis, m = 2 b
    ldpc::AxisTab ax{};
    int rule = 0;         // LDPC_DEMAP_MAXLOG, or LDPC_DEMAP_LOGMAP (ldpc_modulation_with_rule): the demappers' LLR rule
};
