// demap_product.h -- device functions of the mapper and the max-log demapper for PRODUCT constellations (demap.h AxisTab): an I-axis
// level set times a Q-axis level set, b = 1..6 bits an axis, label = I-label << b | Q-label.  The max-log rule separates exactly: the
// other axis's smallest distance adds to m0 and m1 alike and cancels, so a sample costs 2 * 2^b distances, not 4^b.  Shared by
// demap_product.hip and sim_mod_product.hip, so the fused kernel equals the two-step one bit for bit.  The rule is restated in
// tests/product_modulation_spec.py.
#pragma once
#include "demap.h"

#ifdef __HIPCC__
namespace ldpc {

// level of a per-lane axis label: a binary select tree over the uniform table (2^B - 1 selects), label bit 0 first, as mod_point
template <int B>
__device__ __forceinline__ float axis_level(const float (&lev)[kAxisMaxLevels], uint32_t idx) {
    float v[1 << B];
#pragma unroll
    for (int p = 0; p < (1 << B); p++) v[p] = lev[p];
#pragma unroll
    for (int k = 0; k < B; k++) {
        const bool one = (idx >> k) & 1u;
#pragma unroll
        for (int p = 0; p < (1 << (B - 1 - k)); p++) v[p] = one ? v[2 * p + 1] : v[2 * p];
    }
    return v[0];
}

// label of symbol s of a packed codeword row: bits M s .. M s + M - 1, the first one the MSB, M = 2 B up to 12.  A label starts at bit
// M s % 8 of its first byte, a multiple of gcd(M, 8), so it spans ceil((8 - gcd(M, 8) + M) / 8) bytes at the most: one for M = 2, 4, 8
// and two for M = 6, 10, 12 (an odd M of 11 would need three).  No byte at or past PB is read; positions >= n_tx are pad bits, 0 in the row
template <int M>
__device__ __forceinline__ uint32_t product_label(const uint8_t *__restrict__ row, int PB, int s) {
    constexpr int G = (M % 8 == 0) ? 8 : (M % 4 == 0) ? 4 : (M % 2 == 0) ? 2 : 1, NB = (8 - G + M + 7) / 8;
    static_assert(NB <= 4, "the label must fit one 32-bit word");
    const int first = M * s, b0 = first >> 3;
    uint32_t w = 0u;
#pragma unroll
    for (int i = 0; i < NB; i++)
        if (b0 + i < PB) w |= (uint32_t)row[b0 + i] << (8 * i);
    w >>= first & 7;
    return __builtin_bitreverse32(w) >> (32 - M);        // bit j of w -> bit M - 1 - j; the bits from M on fall out
}

// axis label of a symbol label: the I index (a = 0) is its high B bits, the Q index (a = 1) its low B
template <int B>
__device__ __forceinline__ uint32_t axis_index(uint32_t label, int a) { return a ? label & ((1u << B) - 1u) : label >> B; }

// the channel, one coordinate: y = fl(c + fl(sg z)), c = the level of the axis label (I: label >> B, Q: label & (2^B - 1))
template <int B>
__device__ __forceinline__ float axis_symbol(const float (&lev)[kAxisMaxLevels], uint32_t idx, float z, float sg) {
    return axis_level<B>(lev, idx) + sg * z;
}

// max-log LLRs of one coordinate: llr[j] = fl(fl(m0_j - m1_j) inv), m0_j / m1_j = the smallest fl(fl(y - a_l)^2) over the axis
// labels l whose bit j (MSB first) is 0 / 1.  A min of floats is exact in any order, so the mins run down a prefix tree over the label:
// T_B = the distances, T_k[p] = min(T_k+1[2p], T_k+1[2p + 1]), and bit j's m0 / m1 are the mins of the even / odd entries of T_j+1 --
// about 3 * 2^B mins where the literal form takes B * 2^B.  A NaN coordinate makes every distance of its axis NaN and so its B LLRs
template <int B>
__device__ __forceinline__ void axis_llrs(const float (&lev)[kAxisMaxLevels], float y, float inv, float (&llr)[B]) {
    float t[1 << B];
#pragma unroll
    for (int l = 0; l < (1 << B); l++) {
        const float dx = y - lev[l];
        t[l] = dx * dx;
    }
#pragma unroll
    for (int k = B; k >= 1; k--) {                        // t holds T_k: 2^k entries
        float m0 = t[0], m1 = t[1];
#pragma unroll
        for (int p = 1; p < (1 << (k - 1)); p++) {
            m0 = __builtin_fminf(m0, t[2 * p]);
            m1 = __builtin_fminf(m1, t[2 * p + 1]);
        }
        llr[k - 1] = (m0 - m1) * inv;
#pragma unroll
        for (int p = 0; p < (1 << (k - 1)); p++) t[p] = __builtin_fminf(t[2 * p], t[2 * p + 1]);
    }
}

// log-MAP LLRs of one coordinate (include/ldpc_hip.h, "The LLR rule"): the max-log value of axis_llrs, bit for bit, plus c1 - c0,
// c_v = log(sum over the axis labels l whose bit j is v of exp(-(e_l - m_v) inv)).  Exact for the product constellation, not an
// approximation: the other axis's factor is common to both subsets and cancels.  Two passes, as demap_llrs_logmap: axis_llrs's prefix
// tree with the minima kept, then the B 2^B exponentials over distances computed again from the uniform levels (2 operations a level)
// -- the tree has consumed the first ones.  The sums run in label order
template <int B>
__device__ __forceinline__ void axis_llrs_logmap(const float (&lev)[kAxisMaxLevels], float y, float inv, float (&llr)[B]) {
    float t[1 << B], m0[B], m1[B], s0[B], s1[B];
#pragma unroll
    for (int l = 0; l < (1 << B); l++) {
        const float dx = y - lev[l];
        t[l] = dx * dx;
    }
#pragma unroll
    for (int k = B; k >= 1; k--) {                        // t holds T_k: 2^k entries
        float a0 = t[0], a1 = t[1];
#pragma unroll
        for (int p = 1; p < (1 << (k - 1)); p++) {
            a0 = __builtin_fminf(a0, t[2 * p]);
            a1 = __builtin_fminf(a1, t[2 * p + 1]);
        }
        m0[k - 1] = a0; m1[k - 1] = a1;
#pragma unroll
        for (int p = 0; p < (1 << (k - 1)); p++) t[p] = __builtin_fminf(t[2 * p], t[2 * p + 1]);
    }
    if constexpr (B == 1) {                               // one level a subset: both sums are exp(0)
        llr[0] = (m0[0] - m1[0]) * inv;
        return;
    }
#pragma unroll
    for (int l = 0; l < (1 << B); l++) {
        const float dx = y - lev[l];
        const float d = dx * dx;
#pragma unroll
        for (int j = 0; j < B; j++) {
            const int bit = (l >> (B - 1 - j)) & 1;
            const float e = __expf((bit ? m1[j] - d : m0[j] - d) * inv);
            if (bit) s1[j] = (l == (1 << (B - 1 - j))) ? e : s1[j] + e;
            else s0[j] = (l == 0) ? e : s0[j] + e;
        }
    }
#pragma unroll
    for (int j = 0; j < B; j++) llr[j] = logmap_llr((m0[j] - m1[j]) * inv, s0[j], s1[j]);
}

// the LLRs of one coordinate by the rule of the modulation object, as demap_llrs_by
template <int B, int RULE>
__device__ __forceinline__ void axis_llrs_by(const float (&lev)[kAxisMaxLevels], float y, float inv, float (&llr)[B]) {
    if constexpr (RULE == DEMAP_LOGMAP) axis_llrs_logmap<B>(lev, y, inv, llr);
    else axis_llrs<B>(lev, y, inv, llr);
}

// (The kernels that hold more than one sample work AXIS-MAJOR, in a loop of two turns that is not unrolled -- sim_mod_product.hip says
// why.  That loop has no helper here on purpose: as a device function every kernel that has one compiled to other code)

// store_slot's rule for any even M: a slot's M sizeof(OT) bytes go out in the largest 16 / 8 / 4-byte pieces that divide them
// (0: no such piece -- int8 with M = 2, 6, 10)
template <int M, typename OT>
constexpr int kSlotPiece = (M * sizeof(OT)) % 16 == 0 ? 16 : (M * sizeof(OT)) % 8 == 0 ? 8 : (M * sizeof(OT)) % 4 == 0 ? 4 : 0;

// slot s of a row of N elements, as store_slot.  VEC (the host grants it when N % M == 0 and the buffer is aligned to the piece): vector
// stores of kSlotPiece bytes; otherwise element stores
template <int M, typename OT, bool VEC>
__device__ __forceinline__ void store_slot_pieces(OT *__restrict__ row, int s, int n_tx, int N, const float (&llr)[M], float qs) {
    const int e0 = M * s;
    OT v[M];
#pragma unroll
    for (int j = 0; j < M; j++) v[j] = llr_out<OT>(e0 + j < n_tx ? llr[j] : 0.f, qs);
    if constexpr (VEC) {
        constexpr int P = kSlotPiece<M, OT>, PE = P / (int)sizeof(OT);
        typedef typename VecOf<P>::type V;
#pragma unroll
        for (int k = 0; k < M / PE; k++) {
            V pack;
            __builtin_memcpy(&pack, v + k * PE, sizeof(V));
            reinterpret_cast<V *>(row + e0)[k] = pack;
        }
    } else {
#pragma unroll
        for (int j = 0; j < M; j++)
            if (e0 + j < N) row[e0 + j] = v[j];
    }
}

}  // namespace ldpc
#endif  // __HIPCC__
