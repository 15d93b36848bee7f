// sim_mod_product.hip -- the frame source's modulated path (ldpc_sim_transmit, ldpc_sim_generate_mod) for product constellations
// (demap.h AxisTab, b = 1..6 bits an axis): packed codewords -> symbols -> complex AWGN -> (generate_mod) max-log LLRs, in one kernel.
// LANE = SYMBOL PAIR and the channel are sim_mod.hip's, unchanged: one Philox call, counter (frame lo, frame hi, g, stream 2), feeds the
// four normals of symbols 2g and 2g + 1.  The symbol rule and the LLR rule are the device functions of demap_product.h, the ones
// demap_product_kernel calls: the fused kernel equals transmit + ldpc_demap_dev bit for bit.
#include "demap_product.h"
#include "mod_dispatch.h"
#include "sim_noise.h"

namespace ldpc {

// the labels and the four normals of pair g of frame f.  A symbol from n_sym on (the second of the last pair when n_sym is odd, the
// punctured tail) reads no byte at or past PB and gets label bits 0; what is computed for it is never stored
template <int B>
__device__ __forceinline__ void product_pair_draw(const uint8_t *__restrict__ row, int PB, int g, uint64_t seed, uint64_t frame, uint32_t (&label)[2], float (&z)[4]) {
    uint32_t r[4];
    Philox::gen(seed, frame, (uint32_t)g, 2u, r);
    box_muller4(r, z);
    label[0] = product_label<2 * B>(row, PB, 2 * g);
    label[1] = product_label<2 * B>(row, PB, 2 * g + 1);
}

// AXIS-MAJOR, in a loop of two turns that is NOT unrolled: coordinate a of both symbols of the pair, then the other axis.  The level
// table of the turn is tab.lev[a], a wave-uniform index into the kernel arguments: 2^B levels are in scalar registers at a time, where
// straight-line code loads all 2 * 2^B at once and, at B = 6, spills them.  What a turn reads and writes per lane is picked by selects on
// a, never by indexing a register array with it
// vec4: n_sym even and a 16-byte aligned buffer -- every pair is whole and starts on a 16-byte boundary
template <int B>
__global__ __launch_bounds__(256) void product_transmit_kernel(AxisTab tab, const uint8_t *__restrict__ cw, int PB, float *__restrict__ sym, int n_sym, int pairs,
                                                               size_t total, uint64_t seed, uint64_t first_frame, float sg, int vec4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)pairs;
        const int g = (int)(i - f * (size_t)pairs);
        uint32_t label[2];
        float z[4], y[4];
        product_pair_draw<B>(cw + f * (size_t)PB, PB, g, seed, first_frame + f, label, z);
#pragma unroll 1
        for (int a = 0; a < 2; a++) {
            const float (&lev)[kAxisMaxLevels] = tab.lev[a];
            const float y0 = axis_symbol<B>(lev, axis_index<B>(label[0], a), a ? z[1] : z[0], sg);
            const float y1 = axis_symbol<B>(lev, axis_index<B>(label[1], a), a ? z[3] : z[2], sg);
            if (a) { y[1] = y0; y[3] = y1; } else { y[0] = y0; y[2] = y1; }
        }
        float *dst = sym + 2 * (f * (size_t)n_sym + 2 * (size_t)g);
        if (vec4) {
            *reinterpret_cast<float4 *>(dst) = make_float4(y[0], y[1], y[2], y[3]);
        } else {
            *reinterpret_cast<float2 *>(dst) = make_float2(y[0], y[1]);
            if (2 * g + 1 < n_sym) *reinterpret_cast<float2 *>(dst + 2) = make_float2(y[2], y[3]);
        }
    }
}

// pslots = ceil(slots / 2) lanes per frame, slots = ceil(N / M): lane g owns slots 2g and 2g + 1.  store_slot_pieces writes 0 from n_tx
// on, so the LLRs of a symbol from n_sym on are not looked at
template <int B, typename OT, bool VEC>
__global__ __launch_bounds__(256) void product_generate_kernel(AxisTab tab, const uint8_t *__restrict__ cw, int PB, OT *__restrict__ llr, int n_tx, int N, int n_sym,
                                                               int slots, int pslots, size_t total, uint64_t seed, uint64_t first_frame, float sg, float inv, float qs) {
    constexpr int M = 2 * B;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)pslots;
        const int g = (int)(i - f * (size_t)pslots);
        float v0[M], v1[M];
#pragma unroll
        for (int j = 0; j < M; j++) { v0[j] = 0.f; v1[j] = 0.f; }
        if (2 * g < n_sym) {
            uint32_t label[2];
            float z[4];
            product_pair_draw<B>(cw + f * (size_t)PB, PB, g, seed, first_frame + f, label, z);
#pragma unroll 1
            for (int a = 0; a < 2; a++) {
                const float (&lev)[kAxisMaxLevels] = tab.lev[a];
                float r0[B], r1[B];
                axis_llrs<B>(lev, axis_symbol<B>(lev, axis_index<B>(label[0], a), a ? z[1] : z[0], sg), inv, r0);
                axis_llrs<B>(lev, axis_symbol<B>(lev, axis_index<B>(label[1], a), a ? z[3] : z[2], sg), inv, r1);
#pragma unroll
                for (int j = 0; j < B; j++) {
                    if (a) { v0[B + j] = r0[j]; v1[B + j] = r1[j]; } else { v0[j] = r0[j]; v1[j] = r1[j]; }
                }
            }
        }
        OT *row = llr + f * (size_t)N;
        store_slot_pieces<M, OT, VEC>(row, 2 * g, n_tx, N, v0, qs);
        if (2 * g + 1 < slots) store_slot_pieces<M, OT, VEC>(row, 2 * g + 1, n_tx, N, v1, qs);
    }
}

int product_transmit_launch(hipStream_t st, const AxisTab &tab, int b, int batch, int n_tx, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg,
                            float *d_sym) {
    const int rc = check_items("ldpc_sim_transmit", (size_t)batch * (size_t)n_tx, "batch * n_tx");
    if (rc != LDPC_OK) return rc;
    return launched("ldpc_sim_transmit", dispatch_bits("modulation", b, [&](auto k) {
        constexpr int B = decltype(k)::value;
        const int n_sym = mod_symbols(n_tx, 2 * B), pairs = mod_pairs(n_sym);
        const size_t total = (size_t)batch * pairs;
        hipLaunchKernelGGL((product_transmit_kernel<B>), grid_lanes(total), dim3(256), 0, st, tab, d_cw, PB, d_sym, n_sym, pairs, total, seed, first_frame, sg,
                           grant_pair_store(n_sym, d_sym, 16));
        return LDPC_OK;
    }));
}

int product_generate_launch(hipStream_t st, const AxisTab &tab, int b, int batch, int n_tx, int N, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame,
                            float sg, float inv, void *d_llr, int fmt, float qscale) {
    const int rc = check_items("ldpc_sim_generate_mod", (size_t)batch * (size_t)N, "batch * N");
    if (rc != LDPC_OK) return rc;
    return launched("ldpc_sim_generate_mod", dispatch_bits_fmt("modulation", b, fmt, [&](auto k, auto t) {
        constexpr int B = decltype(k)::value, M = 2 * B;
        typedef typename decltype(t)::type OT;
        const int n_sym = mod_symbols(n_tx, M), slots = mod_symbols(N, M), pslots = mod_pairs(slots);
        const size_t total = (size_t)batch * pslots;
        if constexpr (kSlotPiece<M, OT> != 0) {
            if (grant_slot_store(N, M, d_llr, kSlotPiece<M, OT>)) {
                hipLaunchKernelGGL((product_generate_kernel<B, OT, true>), grid_lanes(total), dim3(256), 0, st, tab, d_cw, PB, (OT *)d_llr, n_tx, N, n_sym, slots, pslots, total, seed,
                                   first_frame, sg, inv, qscale);
                return LDPC_OK;
            }
        }
        hipLaunchKernelGGL((product_generate_kernel<B, OT, false>), grid_lanes(total), dim3(256), 0, st, tab, d_cw, PB, (OT *)d_llr, n_tx, N, n_sym, slots, pslots, total, seed,
                           first_frame, sg, inv, qscale);
        return LDPC_OK;
    }));
}

}  // namespace ldpc
