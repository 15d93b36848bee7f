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
#include "mod_dispatch.h"

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

int demap_launch(hipStream_t st, const ModTab &tab, int m, int rule, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, int fmt, float qscale) {
    return launched("demap", dispatch_rule_bits_fmt("demap", rule, m, fmt, [&](auto r, auto k, auto t) {
        constexpr int M = decltype(k)::value, RULE = decltype(r)::value;
        typedef typename decltype(t)::type OT;
        const int n_sym = mod_symbols(n_tx, M), slots = mod_symbols(N, M);
        const size_t total = (size_t)batch * slots;
        if constexpr (kDemapVec<M, OT>) {
            if (grant_slot_store(N, M, d_llr, M * sizeof(OT))) {
                hipLaunchKernelGGL((demap_kernel<M, OT, true, RULE>), grid_stride(total), dim3(256), 0, st, tab, d_sym, (OT *)d_llr, n_tx, N, n_sym, slots, total, inv, qscale);
                return LDPC_OK;
            }
        }
        hipLaunchKernelGGL((demap_kernel<M, OT, false, RULE>), grid_stride(total), dim3(256), 0, st, tab, d_sym, (OT *)d_llr, n_tx, N, n_sym, slots, total, inv, qscale);
        return LDPC_OK;
    }));
}

}  // namespace ldpc
