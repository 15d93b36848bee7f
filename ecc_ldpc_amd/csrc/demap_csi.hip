// demap_csi.hip -- the max-log soft demapper with per-symbol channel state, writing through a bit interleaver (ldpc_demap_dev_il_csi):
// demap_il.hip's kernels with one more input, the power gain of every symbol, d_gain [batch][n_sym].  The LLRs of symbol s are the rule of
// demap.h / demap_product.h with the scale inv_s = fl(inv a) of fading.h in place of inv: the same device functions, called with a
// per-lane scale, so gains of 1 give ldpc_demap_dev_il's output bit for bit.  The rule is restated in tests/fading_spec.py.
// LANE = SYMBOL, as demap_il.hip: lane s < n_sym of a frame loads its sample (8 bytes) and its own gain (4 bytes; consecutive lanes,
// consecutive floats), and stores its m LLRs through the table.  The lanes from n_sym on take the hole list and read no gain.
// ONE ITEM A LANE, no grid-stride loop, for the reason demap_product.hip gives.
// The LLR rule (demap.h DEMAP_MAXLOG / DEMAP_LOGMAP) is a template argument of both kernels; the log-MAP sums use inv_s as the minima do.
#include "demap_product.h"
#include "fading.h"
#include "mod_dispatch.h"

namespace ldpc {

template <int M, typename OT, int RULE>
__global__ __launch_bounds__(256) void demap_csi_kernel(ModTab tab, IlTab il, const float *__restrict__ sym, const float *__restrict__ gain, OT *__restrict__ llr, int n_sym,
                                                        int lanes, size_t total, float inv, float qs) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)lanes;
        const int s = (int)(i - f * (size_t)lanes);
        OT *row = llr + f * (size_t)il.N;
        if (s < n_sym) {
            const size_t at = f * (size_t)n_sym + s;
            const float2 y = *reinterpret_cast<const float2 *>(sym + 2 * at);
            const float inv_s = fade_inv(inv, gain[at]);
            float v[M];
            int32_t p[M];
            demap_llrs_by<M, RULE>(tab, y.x, y.y, inv_s, v);
            il_positions<M>(il.pos + (size_t)M * s, p);
            il_store<M, OT>(row, p, il.n_tx - M * s, v, qs);
        } else {
            il_store_holes<M, OT>(row, il, M * (s - n_sym), qs);
        }
    }
}

template <int B, typename OT, int RULE>
__global__ __launch_bounds__(256) void demap_csi_product_kernel(AxisTab tab, IlTab il, const float *__restrict__ sym, const float *__restrict__ gain, OT *__restrict__ llr,
                                                                int n_sym, int lanes, size_t total, float inv, float qs) {
    constexpr int M = 2 * B;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)lanes;
        const int s = (int)(i - f * (size_t)lanes);
        OT *row = llr + f * (size_t)il.N;
        if (s < n_sym) {
            const size_t at = f * (size_t)n_sym + s;
            const float2 y = *reinterpret_cast<const float2 *>(sym + 2 * at);
            const float inv_s = fade_inv(inv, gain[at]);
            float v[M];
            int32_t p[M];
            // the axes one after the other, in a loop of two turns that is NOT unrolled, as demap_il_product_kernel
#pragma unroll 1
            for (int a = 0; a < 2; a++) {
                float r[B];
                axis_llrs_by<B, RULE>(tab.lev[a], a ? y.y : y.x, inv_s, r);
#pragma unroll
                for (int j = 0; j < B; j++) {
                    if (a) v[B + j] = r[j]; else v[j] = r[j];
                }
            }
            il_positions<M>(il.pos + (size_t)M * s, p);
            il_store<M, OT>(row, p, il.n_tx - M * s, v, qs);
        } else {
            il_store_holes<M, OT>(row, il, M * (s - n_sym), qs);
        }
    }
}

int demap_csi_launch(hipStream_t st, const ModTab &tab, int m, int rule, const IlTab &il, int batch, const float *d_sym, const float *d_gain, float inv, void *d_llr, int fmt,
                     float qscale) {
    const char *what = "ldpc_demap_dev_il_csi";
    return launched(what, dispatch_rule_bits_fmt(what, rule, m, fmt, [&](auto r, auto k, auto t) {
        constexpr int M = decltype(k)::value, RULE = decltype(r)::value;
        typedef typename decltype(t)::type OT;
        const int n_sym = mod_symbols(il.n_tx, M), lanes = mod_lanes(n_sym, il.n_holes, M);
        const size_t total = (size_t)batch * lanes;
        const int rc = check_items(what, total);
        if (rc == LDPC_OK)
            hipLaunchKernelGGL((demap_csi_kernel<M, OT, RULE>), grid_lanes(total), dim3(256), 0, st, tab, il, d_sym, d_gain, (OT *)d_llr, n_sym, lanes, total, inv, qscale);
        return rc;
    }));
}

int demap_csi_product_launch(hipStream_t st, const AxisTab &tab, int b, int rule, const IlTab &il, int batch, const float *d_sym, const float *d_gain, float inv, void *d_llr,
                             int fmt, float qscale) {
    const char *what = "ldpc_demap_dev_il_csi";
    return launched(what, dispatch_rule_bits_fmt(what, rule, b, fmt, [&](auto r, auto k, auto t) {
        constexpr int B = decltype(k)::value, M = 2 * B, RULE = decltype(r)::value;
        typedef typename decltype(t)::type OT;
        const int n_sym = mod_symbols(il.n_tx, M), lanes = mod_lanes(n_sym, il.n_holes, M);
        const size_t total = (size_t)batch * lanes;
        const int rc = check_items(what, total);
        if (rc == LDPC_OK)
            hipLaunchKernelGGL((demap_csi_product_kernel<B, OT, RULE>), grid_lanes(total), dim3(256), 0, st, tab, il, d_sym, d_gain, (OT *)d_llr, n_sym, lanes, total, inv, qscale);
        return rc;
    }));
}

}  // namespace ldpc
