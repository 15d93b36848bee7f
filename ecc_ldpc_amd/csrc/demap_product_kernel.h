// demap_product_kernel.h -- the kernel of ldpc_demap_dev for product constellations and its launcher, templated on the LLR rule
// (demap.h DEMAP_MAXLOG / DEMAP_LOGMAP).  Two translation units instantiate it, one rule each: demap_product.hip (max-log, and the
// dispatch by rule) and demap_product_logmap.hip.  What the kernel does and why it has no grid-stride loop: demap_product.hip.
#pragma once
#include "demap_product.h"
#include "mod_dispatch.h"

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

// the instances of one rule: each of the two translation units calls this with its own
template <int RULE>
static int demap_product_launch_r(hipStream_t st, const AxisTab &tab, int b, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, int fmt, float qscale) {
    const int rc = check_items("demap", (size_t)batch * (size_t)N, "batch * N");
    if (rc != LDPC_OK) return rc;
    return launched("demap", dispatch_bits_fmt("demap", b, fmt, [&](auto k, auto t) {
        constexpr int B = decltype(k)::value, M = 2 * B;
        typedef typename decltype(t)::type OT;
        const int n_sym = mod_symbols(n_tx, M), slots = mod_symbols(N, M);
        const size_t total = (size_t)batch * slots;
        if constexpr (kSlotPiece<M, OT> != 0) {
            if (grant_slot_store(N, M, d_llr, kSlotPiece<M, OT>)) {
                hipLaunchKernelGGL((demap_product_kernel<B, OT, true, RULE>), grid_lanes(total), dim3(256), 0, st, tab, d_sym, (OT *)d_llr, n_tx, N, n_sym, slots, total, inv, qscale);
                return LDPC_OK;
            }
        }
        hipLaunchKernelGGL((demap_product_kernel<B, OT, false, RULE>), grid_lanes(total), dim3(256), 0, st, tab, d_sym, (OT *)d_llr, n_tx, N, n_sym, slots, total, inv, qscale);
        return LDPC_OK;
    }));
}

// the log-MAP instances (demap_product_logmap.hip)
int demap_product_logmap_launch(hipStream_t st, const AxisTab &tab, int b, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, int fmt, float qscale);

}  // namespace ldpc

