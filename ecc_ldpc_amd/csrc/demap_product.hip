// demap_product.hip -- ldpc_demap_dev for product constellations (demap.h AxisTab, b = 1..6 bits an axis, up to 4096-QAM): I/Q samples
// [batch][n_sym][2] -> LLRs [batch][N], one pass.  The rule and its device functions: demap_product.h; restated in
// tests/product_modulation_spec.py, which the kernel reproduces bit for bit.
// LANE = SLOT, as demap.hip: slot s of a frame is output elements m s .. m s + m - 1, m = 2 b: the b LLRs of the I coordinate, then the b
// of the Q coordinate.  A lane works its two axes one after the other, so 2^b distances are live at a time, and the two level tables ride
// in the kernel arguments (scalar loads).  A slot's m elements are contiguous: they go out in 16 / 8 / 4-byte vector stores where the row
// alignment allows it (demap_product.h store_slot_pieces).
// ONE SLOT A LANE, no grid-stride loop: inside a loop the compiler hoists the 128 level loads (and, in sim_mod_product.hip, the Philox key
// schedule) out of it as loop invariants and then spills those scalar registers; without one they are loaded where they are used.
#include "demap_product.h"

namespace ldpc {

template <int B, typename OT, bool VEC>
__global__ __launch_bounds__(256) void demap_product_kernel(AxisTab tab, const float *__restrict__ sym, OT *__restrict__ llr, int n_tx, int N, int n_sym, int slots,
                                                            size_t total, float inv, float qs) {
    constexpr int M = 2 * B;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)slots;
        const int s = (int)(i - f * (size_t)slots);
        float v[M];
        if (s < n_sym) {
            const float2 y = *reinterpret_cast<const float2 *>(sym + 2 * (f * (size_t)n_sym + s));
            float vi[B], vq[B];
            axis_llrs<B>(tab.lev[0], y.x, inv, vi);       // the axes one after the other: 2^B distances live at a time
            axis_llrs<B>(tab.lev[1], y.y, inv, vq);
#pragma unroll
            for (int j = 0; j < B; j++) { v[j] = vi[j]; v[B + j] = vq[j]; }
        } else {
#pragma unroll
            for (int j = 0; j < M; j++) v[j] = 0.f;
        }
        store_slot_pieces<M, OT, VEC>(llr + f * (size_t)N, s, n_tx, N, v, qs);
    }
}

template <int B, typename OT>
static void demap_product_as(hipStream_t st, const AxisTab &tab, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, float qs) {
    constexpr int M = 2 * B;
    const int n_sym = (n_tx + M - 1) / M, slots = (N + M - 1) / M;
    const size_t total = (size_t)batch * slots;
    const dim3 grid((unsigned)((total + 255) / 256));
    if constexpr (kSlotPiece<M, OT> != 0) {
        if (N % M == 0 && (uintptr_t)d_llr % kSlotPiece<M, OT> == 0) {
            hipLaunchKernelGGL((demap_product_kernel<B, OT, true>), grid, dim3(256), 0, st, tab, d_sym, (OT *)d_llr, n_tx, N, n_sym, slots, total, inv, qs);
            return;
        }
    }
    hipLaunchKernelGGL((demap_product_kernel<B, OT, false>), grid, dim3(256), 0, st, tab, d_sym, (OT *)d_llr, n_tx, N, n_sym, slots, total, inv, qs);
}

template <int B>
static void demap_product_b(hipStream_t st, const AxisTab &tab, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, int fmt, float qs) {
    if (fmt == MOD_LLR_I8) demap_product_as<B, int8_t>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, qs);
    else if (fmt == MOD_LLR_F16) demap_product_as<B, __half>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, qs);
    else demap_product_as<B, float>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, qs);
}

int demap_product_launch(hipStream_t st, const AxisTab &tab, int b, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, int fmt, float qscale) {
    if ((size_t)batch * (size_t)N > kProductMaxItems) return set_error(LDPC_EINVAL, "demap: batch * N = %zu is more than one launch holds", (size_t)batch * (size_t)N);
    switch (b) {
        case 1: demap_product_b<1>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        case 2: demap_product_b<2>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        case 3: demap_product_b<3>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        case 4: demap_product_b<4>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        case 5: demap_product_b<5>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        case 6: demap_product_b<6>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        default: return set_error(LDPC_EINVAL, "demap: %d bits per axis", b);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "demap: %s", hipGetErrorString(e));
    return LDPC_OK;
}

}  // namespace ldpc
