// interleaver.h -- the bit interleaver of include/ldpc_hip.h (ldpc_interleaver): a position table between codeword order and transmitted
// order.  Transmitted bit t is codeword bit pos[t]; the codeword positions no pos[t] names are punctured (the sorted hole list).  The
// host side (validation, the block rule): interleaver.cc.  The kernels that read the table: demap_il.hip (the demapper writing through
// it, and the table alone on bits and on LLRs) and sim_mod_il.hip (the frame source's modulated path gathering its labels through it).
// The rule is restated in tests/interleaver_spec.py.
#pragma once
#include "demap.h"

namespace ldpc {
// a lane reads the m entries of its symbol in vector loads, the lane of a frame's last symbol up to m - 1 entries past n_tx: the
// device table is padded by this many entries, all 0: the label gather reads bit 0 of the row for a pad bit and drops it, and no LLR
// is stored for one
constexpr int kIlPad = 32;

// the table as a kernel argument (device pointers)
struct IlTab {
    const int32_t *pos;     // [n_tx + kIlPad]
    const int32_t *holes;   // [n_holes], ascending
    int n_tx, N, n_holes;
};

// pos [n_tx] is an injection into 0..N-1, 1 <= n_tx <= N: LDPC_OK and the sorted complement in `holes`, or LDPC_EINVAL
int interleaver_check(const char *what, int n_tx, int N, const int32_t *pos, std::vector<int32_t> &holes);

// ldpc_demap_dev_il: d_llr [batch][N] <- the LLRs of d_sym [batch][n_sym][2] at their codeword positions, 0 at the holes
int demap_il_launch(hipStream_t st, const ModTab &tab, int m, int rule, const IlTab &il, int batch, const float *d_sym, float inv, void *d_llr, int fmt, float qscale);
int demap_il_product_launch(hipStream_t st, const AxisTab &tab, int b, int rule, const IlTab &il, int batch, const float *d_sym, float inv, void *d_llr, int fmt, float qscale);
// the table alone.  Bits: rows of N (bytes) or ceil(N / 8) (packed) -> rows of n_tx or ceil(n_tx / 8); LLRs: [batch][n_tx] -> [batch][N]
// elements of `elem` bytes (1, 2, 4)
int interleave_bits_launch(hipStream_t st, const IlTab &il, int batch, const uint8_t *d_in, bool in_packed, uint8_t *d_out, bool out_packed);
int deinterleave_llr_launch(hipStream_t st, const IlTab &il, int batch, const void *d_in, void *d_out, int elem);
// ldpc_sim_transmit_il / ldpc_sim_generate_mod_il: as mod_transmit_launch / mod_generate_launch (demap.h), the label of symbol s gathered
// from bits pos[m s + j] of the packed row; every pos[t] < 8 PB (the entry points see to it)
int mod_transmit_il_launch(hipStream_t st, const ModTab &tab, int m, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg,
                           float *d_sym);
int mod_generate_il_launch(hipStream_t st, const ModTab &tab, int m, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg,
                           float inv, void *d_llr, int fmt, float qscale);
int product_transmit_il_launch(hipStream_t st, const AxisTab &tab, int b, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame,
                               float sg, float *d_sym);
int product_generate_il_launch(hipStream_t st, const AxisTab &tab, int b, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame,
                               float sg, float inv, void *d_llr, int fmt, float qscale);

#ifdef __HIPCC__
// the M table entries of a symbol from src = pos + M s (transmitted bits M s .. M s + M - 1), in the largest 16 / 8 / 4-byte loads that
// divide 4 M bytes: the table is 16-byte aligned, so entry M s is aligned to that piece.  Reads up to entry M s + M - 1 <= n_tx + kIlPad - 1
// for s < n_sym.  The kernels hand a symbol's place in the table on as this pointer and as rem = n_tx - M s (> 0 for s < n_sym), the
// number of its bits that are no pad bits if below M: two per-lane values, where pos, s and n_tx would be scalar registers kept alive
template <int M>
__device__ __forceinline__ void il_positions(const int32_t *__restrict__ src, int32_t (&p)[M]) {
    if constexpr (M % 4 == 0) {
#pragma unroll
        for (int k = 0; k < M / 4; k++) {
            const int4 q = reinterpret_cast<const int4 *>(src)[k];
            p[4 * k] = q.x; p[4 * k + 1] = q.y; p[4 * k + 2] = q.z; p[4 * k + 3] = q.w;
        }
    } else if constexpr (M % 2 == 0) {
#pragma unroll
        for (int k = 0; k < M / 2; k++) {
            const int2 q = reinterpret_cast<const int2 *>(src)[k];
            p[2 * k] = q.x; p[2 * k + 1] = q.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < M; j++) p[j] = src[j];
    }
}

// the same of the symbol PAIR g of the frame source's kernels: src = pos + M 2g, rem = n_tx - M 2g (> 0).  Symbol 2g + 1 is at src + M
// with rem - M, which is <= 0 from n_sym on (the second of the last pair when n_sym is odd): such a symbol has no entries, none are
// loaded and none looked at
template <int M>
__device__ __forceinline__ void il_pair_positions(const int32_t *__restrict__ src, int rem, int32_t (&p0)[M], int32_t (&p1)[M]) {
    il_positions<M>(src, p0);
#pragma unroll
    for (int j = 0; j < M; j++) p1[j] = 0;
    if (rem > M) il_positions<M>(src + M, p1);
}

// the LLRs of a symbol go to their codeword positions; those of pad bits (j >= rem) are not written
template <int M, typename OT>
__device__ __forceinline__ void il_store(OT *__restrict__ row, const int32_t (&p)[M], int rem, const float (&llr)[M], float qs) {
#pragma unroll
    for (int j = 0; j < M; j++)
        if (j < rem) row[p[j]] = llr_out<OT>(llr[j], qs);
}

// holes first .. first + K - 1 of the list get 0
template <int K, typename OT>
__device__ __forceinline__ void il_store_holes(OT *__restrict__ row, const IlTab &il, int first, float qs) {
#pragma unroll
    for (int j = 0; j < K; j++)
        if (first + j < il.n_holes) row[il.holes[first + j]] = llr_out<OT>(0.f, qs);
}

// label of a symbol gathered from a packed codeword row: bit j (the first one the MSB) is bit p[j] of the row; pad bits (j >= rem) are 0.
// Branch-free: the entry of a pad bit is 0 (the table's padding; the zeros il_pair_positions gives a missing symbol), so it reads bit 0
// of the row, always there, and the mask drops it: the label keeps its top rem bits
template <int M>
__device__ __forceinline__ uint32_t il_label(const uint8_t *__restrict__ row, const int32_t (&p)[M], int rem) {
    uint32_t label = 0u;
#pragma unroll
    for (int j = 0; j < M; j++) label |= (((uint32_t)row[p[j] >> 3] >> (p[j] & 7)) & 1u) << (M - 1 - j);
    const uint32_t keep = rem >= M ? ~0u : rem <= 0 ? 0u : ~((1u << (M - rem)) - 1u);
    return label & keep;
}
#endif  // __HIPCC__
}  // namespace ldpc

// (host) the object behind include/ldpc_hip.h ldpc_interleaver
struct ldpc_interleaver {
    int n_tx = 0, N = 0, device = -1;
    int max_pos = 0;                 // the largest entry: the frame source's paths need it below their n_tx
    std::vector<int32_t> pos;        // [n_tx]
    int n_holes = 0;
    int32_t *d_tab = nullptr;        // one allocation: pos [n_tx] | pad [kIlPad, rounded up to 4 entries] | holes [n_holes]
    ldpc::IlTab tab{};
};
