// demap.hip -- the stand-alone max-log soft demapper (ldpc_demap_dev): I/Q samples [batch][n_sym][2] -> LLRs [batch][N] in the
// decoders' input formats (float32, fp16, int8), one pass.  The rule and its device functions: demap.h; restated in
// tests/modulation_spec.py, which the kernel reproduces bit for bit.
// LANE = SLOT: slot s of a frame is output elements m s .. m s + m - 1, the m LLRs of symbol s.  Slots from n_sym on (the punctured tail
// n_tx .. N - 1) hold zeros only.  The constellation rides in the kernel arguments (scalar loads); the instances are templated on m, so the
// 2^m-point loop unrolls: per point 2 subtracts, 2 multiplies, 1 add and m mins.
// Where a lane's m elements fit no vector store (m = 3, 5, 6; rows that miss the alignment) it stores them one by one.  The alternative, a
// transpose through LDS with whole-dword stores by the workgroup, was built and measured on 8PSK (65 536 frames of jpl.4096.4.5): slower
// into float32 (0.672 against 0.650 ms) and into int8 (0.566 against 0.460 ms), so it is not kept.
// The LLR rule (demap.h DEMAP_MAXLOG / DEMAP_LOGMAP) is a template argument: a log-MAP instance adds a second pass of m 2^m exponentials.
#include "demap.h"
#include <algorithm>

namespace ldpc {

template <int M, typename OT, bool VEC, int RULE>
__global__ __launch_bounds__(256) void demap_kernel(ModTab tab, const float *__restrict__ sym, OT *__restrict__ llr, int n_tx, int N, int n_sym, int slots, size_t total,
                                                    float inv, float qs) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t f = i / (size_t)slots;
        const int s = (int)(i - f * (size_t)slots);
        float v[M];
        if (s < n_sym) {
            const float2 y = *reinterpret_cast<const float2 *>(sym + 2 * (f * (size_t)n_sym + s));
            demap_llrs_by<M, RULE>(tab, y.x, y.y, inv, v);
        } else {
#pragma unroll
            for (int j = 0; j < M; j++) v[j] = 0.f;
        }
        store_slot<M, OT, VEC>(llr + f * (size_t)N, s, n_tx, N, v, qs);
    }
}

template <int M, typename OT, int RULE>
static void demap_launch_as(hipStream_t st, const ModTab &tab, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, float qs) {
    const int n_sym = (n_tx + M - 1) / M, slots = (N + M - 1) / M;
    const size_t total = (size_t)batch * slots;
    const dim3 grid((unsigned)std::min<size_t>((total + 255) / 256, (size_t)1 << 20));
    if constexpr (kDemapVec<M, OT>) {
        if (N % M == 0 && (uintptr_t)d_llr % (M * sizeof(OT)) == 0) {
            hipLaunchKernelGGL((demap_kernel<M, OT, true, RULE>), grid, dim3(256), 0, st, tab, d_sym, (OT *)d_llr, n_tx, N, n_sym, slots, total, inv, qs);
            return;
        }
    }
    hipLaunchKernelGGL((demap_kernel<M, OT, false, RULE>), grid, dim3(256), 0, st, tab, d_sym, (OT *)d_llr, n_tx, N, n_sym, slots, total, inv, qs);
}

template <int M, int RULE>
static void demap_launch_m(hipStream_t st, const ModTab &tab, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, int fmt, float qs) {
    if (fmt == MOD_LLR_I8) demap_launch_as<M, int8_t, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, qs);
    else if (fmt == MOD_LLR_F16) demap_launch_as<M, __half, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, qs);
    else demap_launch_as<M, float, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, qs);
}

template <int RULE>
static int demap_launch_r(hipStream_t st, const ModTab &tab, int m, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, int fmt, float qscale) {
    switch (m) {
        case 1: demap_launch_m<1, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        case 2: demap_launch_m<2, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        case 3: demap_launch_m<3, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        case 4: demap_launch_m<4, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        case 5: demap_launch_m<5, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        case 6: demap_launch_m<6, RULE>(st, tab, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale); break;
        default: return set_error(LDPC_EINVAL, "demap: %d bits per symbol", m);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "demap: %s", hipGetErrorString(e));
    return LDPC_OK;
}

int demap_launch(hipStream_t st, const ModTab &tab, int m, int rule, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, int fmt, float qscale) {
    if (rule == DEMAP_LOGMAP) return demap_launch_r<DEMAP_LOGMAP>(st, tab, m, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale);
    return demap_launch_r<DEMAP_MAXLOG>(st, tab, m, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale);
}

}  // namespace ldpc
