// sim_mod.hip -- the frame source's modulated path (ldpc_sim_transmit, ldpc_sim_generate_mod): packed codewords -> constellation symbols
// -> complex AWGN -> (generate_mod) max-log LLRs, in one kernel.  The codewords come from the parity stages of sim.hip / sim_sparse.hip /
// sim_systematic.hip unchanged, packed as ldpc_sim_encode_messages packs them.
// LANE = SYMBOL PAIR g = symbols 2g and 2g + 1 of a frame: ONE Philox call, counter (frame lo, frame hi, g, stream 2), feeds the four
// normals of the pair (sim_noise.h box_muller4, the BPSK source's own): (z0, z1) -> I, Q of symbol 2g, (z2, z3) -> I, Q of 2g + 1.
// The symbol rule and the LLR rule are the device functions of demap.h, the ones demap_kernel calls: the fused kernel equals
// transmit + ldpc_demap_dev bit for bit, the sample never leaves its registers.
#include "mod_dispatch.h"
#include "sim_noise.h"

namespace ldpc {

// the two noisy symbols of pair g of frame f; a symbol from n_sym on (the second of the last pair when n_sym is odd) is not made
template <int M>
__device__ __forceinline__ void mod_pair(const ModTab &tab, const uint8_t *__restrict__ row, int PB, int g, int n_sym, uint64_t seed, uint64_t frame, float sg, float (&y)[4]) {
    uint32_t r[4];
    float z[4];
    Philox::gen(seed, frame, (uint32_t)g, 2u, r);
    box_muller4(r, z);
    mod_symbol<M>(tab, mod_label<M>(row, PB, 2 * g), z[0], z[1], sg, y[0], y[1]);
    y[2] = 0.f; y[3] = 0.f;
    if (2 * g + 1 < n_sym) mod_symbol<M>(tab, mod_label<M>(row, PB, 2 * g + 1), z[2], z[3], sg, y[2], y[3]);
}

// vec4: n_sym even and a 16-byte aligned buffer -- every pair is whole and starts on a 16-byte boundary
template <int M>
__global__ __launch_bounds__(256) void mod_transmit_kernel(ModTab tab, const uint8_t *__restrict__ cw, int PB, float *__restrict__ sym, int n_sym, int pairs, size_t total,
                                                           uint64_t seed, uint64_t first_frame, float sg, int vec4) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t f = i / (size_t)pairs;
        const int g = (int)(i - f * (size_t)pairs);
        float y[4];
        mod_pair<M>(tab, cw + f * (size_t)PB, PB, g, n_sym, seed, first_frame + f, sg, y);
        float *dst = sym + 2 * (f * (size_t)n_sym + 2 * (size_t)g);
        if (vec4) {
            *reinterpret_cast<float4 *>(dst) = make_float4(y[0], y[1], y[2], y[3]);
        } else {
            *reinterpret_cast<float2 *>(dst) = make_float2(y[0], y[1]);
            if (2 * g + 1 < n_sym) *reinterpret_cast<float2 *>(dst + 2) = make_float2(y[2], y[3]);
        }
    }
}

// pslots = ceil(slots / 2) lanes per frame, slots = ceil(N / M): lane g owns slots 2g and 2g + 1 (demap.h store_slot)
template <int M, typename OT, bool VEC>
__global__ __launch_bounds__(256) void mod_generate_kernel(ModTab tab, const uint8_t *__restrict__ cw, int PB, OT *__restrict__ llr, int n_tx, int N, int n_sym, int slots,
                                                           int pslots, size_t total, uint64_t seed, uint64_t first_frame, float sg, float inv, float qs) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t f = i / (size_t)pslots;
        const int g = (int)(i - f * (size_t)pslots);
        float v0[M], v1[M];
#pragma unroll
        for (int j = 0; j < M; j++) { v0[j] = 0.f; v1[j] = 0.f; }
        if (2 * g < n_sym) {
            float y[4];
            mod_pair<M>(tab, cw + f * (size_t)PB, PB, g, n_sym, seed, first_frame + f, sg, y);
            demap_llrs<M>(tab, y[0], y[1], inv, v0);
            if (2 * g + 1 < n_sym) demap_llrs<M>(tab, y[2], y[3], inv, v1);
        }
        OT *row = llr + f * (size_t)N;
        store_slot<M, OT, VEC>(row, 2 * g, n_tx, N, v0, qs);
        if (2 * g + 1 < slots) store_slot<M, OT, VEC>(row, 2 * g + 1, n_tx, N, v1, qs);
    }
}

int mod_transmit_launch(hipStream_t st, const ModTab &tab, int m, int batch, int n_tx, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg,
                        float *d_sym) {
    return launched("ldpc_sim_transmit", dispatch_bits("modulation", m, [&](auto k) {
        constexpr int M = decltype(k)::value;
        const int n_sym = mod_symbols(n_tx, M), pairs = mod_pairs(n_sym);
        const size_t total = (size_t)batch * pairs;
        hipLaunchKernelGGL((mod_transmit_kernel<M>), grid_stride(total), dim3(256), 0, st, tab, d_cw, PB, d_sym, n_sym, pairs, total, seed, first_frame, sg,
                           grant_pair_store(n_sym, d_sym, 16));
        return LDPC_OK;
    }));
}

int mod_generate_launch(hipStream_t st, const ModTab &tab, int m, int batch, int n_tx, int N, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg,
                        float inv, void *d_llr, int fmt, float qscale) {
    return launched("ldpc_sim_generate_mod", dispatch_bits_fmt("modulation", m, fmt, [&](auto k, auto t) {
        constexpr int M = decltype(k)::value;
        typedef typename decltype(t)::type OT;
        const int n_sym = mod_symbols(n_tx, M), slots = mod_symbols(N, M), pslots = mod_pairs(slots);
        const size_t total = (size_t)batch * pslots;
        if constexpr (kDemapVec<M, OT>) {
            if (grant_slot_store(N, M, d_llr, M * sizeof(OT))) {
                hipLaunchKernelGGL((mod_generate_kernel<M, OT, true>), grid_stride(total), dim3(256), 0, st, tab, d_cw, PB, (OT *)d_llr, n_tx, N, n_sym, slots, pslots, total, seed,
                                   first_frame, sg, inv, qscale);
                return LDPC_OK;
            }
        }
        hipLaunchKernelGGL((mod_generate_kernel<M, OT, false>), grid_stride(total), dim3(256), 0, st, tab, d_cw, PB, (OT *)d_llr, n_tx, N, n_sym, slots, pslots, total, seed,
                           first_frame, sg, inv, qscale);
        return LDPC_OK;
    }));
}

}  // namespace ldpc
