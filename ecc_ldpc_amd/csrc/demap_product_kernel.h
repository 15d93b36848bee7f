// demap_product_kernel.h -- the kernel of ldpc_demap_dev for product constellations and its launcher, templated on the LLR rule
// (demap.h DEMAP_MAXLOG / DEMAP_LOGMAP).  Two translation units instantiate it, one rule each: demap_product.hip (max-log, and the
// dispatch by rule) and demap_product_logmap.hip.  What the kernel does and why it has no grid-stride loop: demap_product.hip.
#pragma once
#include "demap_product.h"

namespace ldpc {

template <int B, typename OT, bool VEC, int RULE>
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
            axis_llrs_by<B, RULE>(tab.lev[0], y.x, inv, vi);       // the axes one after the other: 2^B distances live at a time
            axis_llrs_by<B, RULE>(tab.lev[1], y.y, inv, vq);
#pragma unroll
            for (int j = 0; j < B; j++) { v[j] = vi[j]; v[B + j] = vq[j]; }
        } else {
#pragma unroll
            for (int j = 0; j < M; j++) v[j] = 0.f;
        }
        store_slot_pieces<M, OT, VEC>(llr + f * (size_t)N, s, n_tx, N, v, qs);
    }
}

template <int B, typename OT, int RULE>
static void demap_product_as(hipStream_t st, const AxisTab &tab, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, float qs) {
    constexpr int M = 2 * B;
    const int n_sym = (n_tx + M - 1) / M, slots = (N + M - 1) / M;
    const size_t total = (size_t)batch * slots;
    const dim3 grid((unsigned)((total + 255) / 256));
    if constexpr (kSlotPiece<M, OT> != 0) {
        if (N % M == 0 && (uintptr_t)d_llr % kSlotPiece<M, OT> == 0) {
            hipLaunchKernelGGL((demap_product_kernel<B, OT, true, RULE>), grid, dim3(256), 0, st, tab, d_sym, (OT *)d_llr, n_tx, N, n_sym, slots, total, inv, qs);
            return;
        }
    }
    hipLaunchKernelGGL((demap_product_kernel<B, OT, false, RULE>), grid, dim3(256), 0, st, tab, d_sym, (OT *)d_llr, n_tx, N, n_sym, slots, total, inv, qs);
}

template <int B, int RULE>
static void demap_product_b(hipStream_t st, const AxisTab &tab, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, int fmt, float qs) {
    if (fmt == MOD_LLR_I8) demap_product_as<B, int8_t, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, qs);
    else if (fmt == MOD_LLR_F16) demap_product_as<B, __half, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, qs);
    else demap_product_as<B, float, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, qs);
}

template <int RULE>
static int demap_product_launch_r(hipStream_t st, const AxisTab &tab, int b, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, int fmt, float qscale) {
    if ((size_t)batch * (size_t)N > kProductMaxItems) return set_error(LDPC_EINVAL, "demap: batch * N = %zu is more than one launch holds", (size_t)batch * (size_t)N);
    switch (b) {
        case 1: demap_product_b<1, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        case 2: demap_product_b<2, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        case 3: demap_product_b<3, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        case 4: demap_product_b<4, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        case 5: demap_product_b<5, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        case 6: demap_product_b<6, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        default: return set_error(LDPC_EINVAL, "demap: %d bits per axis", b);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "demap: %s", hipGetErrorString(e));
    return LDPC_OK;
}

// the log-MAP instances (demap_product_logmap.hip)
int demap_product_logmap_launch(hipStream_t st, const AxisTab &tab, int b, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, int fmt, float qscale);

}  // namespace ldpc
