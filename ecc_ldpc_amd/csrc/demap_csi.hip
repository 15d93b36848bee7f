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

namespace ldpc {

// lanes per frame: the symbols, then ceil(n_holes / K) lanes of K holes each
static int csi_lanes(int items, int n_holes, int K) { return items + (n_holes + K - 1) / K; }

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

template <int M, typename OT, int RULE>
static int demap_csi_as(hipStream_t st, const ModTab &tab, const IlTab &il, int batch, const float *d_sym, const float *d_gain, float inv, void *d_llr, float qs) {
    const int n_sym = (il.n_tx + M - 1) / M, lanes = csi_lanes(n_sym, il.n_holes, M);
    const size_t total = (size_t)batch * lanes;
    if (total > kIlMaxItems) return set_error(LDPC_EINVAL, "ldpc_demap_dev_il_csi: %zu items are more than one launch holds", total);
    hipLaunchKernelGGL((demap_csi_kernel<M, OT, RULE>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, tab, il, d_sym, d_gain, (OT *)d_llr, n_sym, lanes, total, inv, qs);
    return LDPC_OK;
}

template <int B, typename OT, int RULE>
static int demap_csi_product_as(hipStream_t st, const AxisTab &tab, const IlTab &il, int batch, const float *d_sym, const float *d_gain, float inv, void *d_llr, float qs) {
    constexpr int M = 2 * B;
    const int n_sym = (il.n_tx + M - 1) / M, lanes = csi_lanes(n_sym, il.n_holes, M);
    const size_t total = (size_t)batch * lanes;
    if (total > kIlMaxItems) return set_error(LDPC_EINVAL, "ldpc_demap_dev_il_csi: %zu items are more than one launch holds", total);
    hipLaunchKernelGGL((demap_csi_product_kernel<B, OT, RULE>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, tab, il, d_sym, d_gain, (OT *)d_llr, n_sym, lanes, total,
                       inv, qs);
    return LDPC_OK;
}

template <int M, int RULE>
static int demap_csi_m(hipStream_t st, const ModTab &tab, const IlTab &il, int batch, const float *d_sym, const float *d_gain, float inv, void *d_llr, int fmt, float qs) {
    if (fmt == MOD_LLR_I8) return demap_csi_as<M, int8_t, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, qs);
    if (fmt == MOD_LLR_F16) return demap_csi_as<M, __half, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, qs);
    return demap_csi_as<M, float, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, qs);
}

template <int B, int RULE>
static int demap_csi_product_b(hipStream_t st, const AxisTab &tab, const IlTab &il, int batch, const float *d_sym, const float *d_gain, float inv, void *d_llr, int fmt,
                               float qs) {
    if (fmt == MOD_LLR_I8) return demap_csi_product_as<B, int8_t, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, qs);
    if (fmt == MOD_LLR_F16) return demap_csi_product_as<B, __half, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, qs);
    return demap_csi_product_as<B, float, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, qs);
}

static int csi_launched(int rc) {
    if (rc != LDPC_OK) return rc;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "ldpc_demap_dev_il_csi: %s", hipGetErrorString(e));
    return LDPC_OK;
}

template <int RULE>
static int demap_csi_launch_r(hipStream_t st, const ModTab &tab, int m, const IlTab &il, int batch, const float *d_sym, const float *d_gain, float inv, void *d_llr, int fmt,
                              float qscale) {
    int rc;
    switch (m) {
        case 1: rc = demap_csi_m<1, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, fmt, qscale); break;
        case 2: rc = demap_csi_m<2, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, fmt, qscale); break;
        case 3: rc = demap_csi_m<3, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, fmt, qscale); break;
        case 4: rc = demap_csi_m<4, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, fmt, qscale); break;
        case 5: rc = demap_csi_m<5, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, fmt, qscale); break;
        case 6: rc = demap_csi_m<6, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, fmt, qscale); break;
        default: return set_error(LDPC_EINVAL, "ldpc_demap_dev_il_csi: %d bits per symbol", m);
    }
    return csi_launched(rc);
}

template <int RULE>
static int demap_csi_product_launch_r(hipStream_t st, const AxisTab &tab, int b, const IlTab &il, int batch, const float *d_sym, const float *d_gain, float inv, void *d_llr,
                                      int fmt, float qscale) {
    int rc;
    switch (b) {
        case 1: rc = demap_csi_product_b<1, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, fmt, qscale); break;
        case 2: rc = demap_csi_product_b<2, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, fmt, qscale); break;
        case 3: rc = demap_csi_product_b<3, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, fmt, qscale); break;
        case 4: rc = demap_csi_product_b<4, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, fmt, qscale); break;
        case 5: rc = demap_csi_product_b<5, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, fmt, qscale); break;
        case 6: rc = demap_csi_product_b<6, RULE>(st, tab, il, batch, d_sym, d_gain, inv, d_llr, fmt, qscale); break;
        default: return set_error(LDPC_EINVAL, "ldpc_demap_dev_il_csi: %d bits per axis", b);
    }
    return csi_launched(rc);
}

int demap_csi_launch(hipStream_t st, const ModTab &tab, int m, int rule, const IlTab &il, int batch, const float *d_sym, const float *d_gain, float inv, void *d_llr, int fmt,
                     float qscale) {
    if (rule == DEMAP_LOGMAP) return demap_csi_launch_r<DEMAP_LOGMAP>(st, tab, m, il, batch, d_sym, d_gain, inv, d_llr, fmt, qscale);
    return demap_csi_launch_r<DEMAP_MAXLOG>(st, tab, m, il, batch, d_sym, d_gain, inv, d_llr, fmt, qscale);
}

int demap_csi_product_launch(hipStream_t st, const AxisTab &tab, int b, int rule, const IlTab &il, int batch, const float *d_sym, const float *d_gain, float inv, void *d_llr,
                             int fmt, float qscale) {
    if (rule == DEMAP_LOGMAP) return demap_csi_product_launch_r<DEMAP_LOGMAP>(st, tab, b, il, batch, d_sym, d_gain, inv, d_llr, fmt, qscale);
    return demap_csi_product_launch_r<DEMAP_MAXLOG>(st, tab, b, il, batch, d_sym, d_gain, inv, d_llr, fmt, qscale);
}

}  // namespace ldpc
