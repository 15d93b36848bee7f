// sim_mod_fading.hip -- the frame source's modulated path through a bit interleaver over a FADING channel (ldpc_sim_transmit_il_fading,
// ldpc_sim_generate_mod_il_fading): sim_mod_il.hip's kernels with a power gain per symbol.  Packed codewords -> labels gathered through
// the position table -> constellation symbols -> noise of sigma / sqrt(a) per symbol -> (generate) max-log LLRs scaled by a, stored
// through the same table, in one kernel: neither samples nor gains need reach memory.
// LANE = SYMBOL PAIR, the noise (stream 2) and the labels are sim_mod_il.hip's, unchanged.  The gains are fading.h's: a lane draws those
// of its two symbols from stream 3 -- one more Philox call, whatever the block length: the two symbols of a pair always lie in one
// block pair (fading.h says why) -- and hands the per-symbol sigma and LLR scale to the device functions of demap.h and
// demap_product.h, the ones demap_csi.hip calls: the fused kernel equals ldpc_sim_transmit_il_fading + ldpc_demap_dev_il_csi bit for
// bit.  A non-null d_gain [batch][n_sym] receives the gains.  The rule is restated in tests/fading_spec.py.
// The gains are drawn, turned into the four per-lane scales and stored FIRST, so the descriptor and the gain pointer are dead before
// the distances are live.  ONE ITEM A LANE, no grid-stride loop (demap_product.hip says why).
#include "fading.h"
#include "mod_dispatch.h"
#include "sim_mod_pair.h"

namespace ldpc {

// the gains of pair g of frame f, stored where the caller wants them (vec2: n_sym even and an 8-byte aligned buffer), and the per-symbol
// sigma of the channel.  `second`: symbol 2g + 1 exists
__device__ __forceinline__ void fade_pair(const FadeArg &fad, uint64_t seed, uint64_t frame, int g, bool second, float sg, float *__restrict__ gain_row, int vec2, float &a0,
                                          float &a1, float &sg0, float &sg1) {
    fade_pair_gains(fad, seed, frame, 2 * g, a0, a1);
    if (gain_row) {
        if (vec2) {
            *reinterpret_cast<float2 *>(gain_row + 2 * g) = make_float2(a0, a1);
        } else {
            gain_row[2 * g] = a0;
            if (second) gain_row[2 * g + 1] = a1;
        }
    }
    sg0 = fade_sigma(sg, a0);
    sg1 = fade_sigma(sg, a1);
}

// vec4: n_sym even and a 16-byte aligned sample buffer; vec2: n_sym even and an 8-byte aligned gain buffer
template <int M>
__global__ __launch_bounds__(256) void fading_transmit_kernel(ModTab tab, IlTab il, FadeArg fad, const uint8_t *__restrict__ cw, int PB, float *__restrict__ sym,
                                                              float *__restrict__ gain, int n_sym, int pairs, size_t total, uint64_t seed, uint64_t first_frame, float sg,
                                                              int vec4, int vec2) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)pairs;
        const int g = (int)(i - f * (size_t)pairs);
        const int rem = il.n_tx - 2 * M * g;
        float a0, a1, sg0, sg1;
        fade_pair(fad, seed, first_frame + f, g, rem > M, sg, gain ? gain + f * (size_t)n_sym : nullptr, vec2, a0, a1, sg0, sg1);
        int32_t p0[M], p1[M];
        float y[4];
        il_pair_positions<M>(il.pos + (size_t)(2 * M) * g, rem, p0, p1);
        mod_pair_il<M>(tab, cw + f * (size_t)PB, p0, p1, g, rem, seed, first_frame + f, sg0, sg1, y);
        store_pair_il<M>(sym + 2 * (f * (size_t)n_sym + 2 * (size_t)g), y, rem, vec4);
    }
}

// lanes = pairs + ceil(n_holes / 2M) per frame; the lanes of the hole list draw nothing
template <int M, typename OT>
__global__ __launch_bounds__(256) void fading_generate_kernel(ModTab tab, IlTab il, FadeArg fad, const uint8_t *__restrict__ cw, int PB, OT *__restrict__ llr,
                                                              float *__restrict__ gain, int n_sym, int pairs, int lanes, size_t total, uint64_t seed, uint64_t first_frame,
                                                              float sg, float inv, float qs, int vec2) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)lanes;
        const int g = (int)(i - f * (size_t)lanes);
        OT *row = llr + f * (size_t)il.N;
        if (g < pairs) {
            const int rem = il.n_tx - 2 * M * g;
            float a0, a1, sg0, sg1;
            fade_pair(fad, seed, first_frame + f, g, rem > M, sg, gain ? gain + f * (size_t)n_sym : nullptr, vec2, a0, a1, sg0, sg1);
            int32_t p0[M], p1[M];
            float y[4], v[M];
            il_pair_positions<M>(il.pos + (size_t)(2 * M) * g, rem, p0, p1);
            mod_pair_il<M>(tab, cw + f * (size_t)PB, p0, p1, g, rem, seed, first_frame + f, sg0, sg1, y);
            demap_llrs<M>(tab, y[0], y[1], fade_inv(inv, a0), v);
            il_store<M, OT>(row, p0, rem, v, qs);
            if (rem > M) {
                demap_llrs<M>(tab, y[2], y[3], fade_inv(inv, a1), v);
                il_store<M, OT>(row, p1, rem - M, v, qs);
            }
        } else {
            il_store_holes<2 * M, OT>(row, il, 2 * M * (g - pairs), qs);
        }
    }
}

// ---- product constellations: sim_mod_il.hip's product kernels, AXIS-MAJOR in a loop of two turns that is NOT unrolled, with the
// per-symbol sigma and LLR scale in four per-lane registers
template <int B>
__global__ __launch_bounds__(256) void fading_product_transmit_kernel(AxisTab tab, IlTab il, FadeArg fad, const uint8_t *__restrict__ cw, int PB, float *__restrict__ sym,
                                                                      float *__restrict__ gain, int n_sym, int pairs, size_t total, uint64_t seed, uint64_t first_frame,
                                                                      float sg, int vec4, int vec2) {
    constexpr int M = 2 * B;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)pairs;
        const int g = (int)(i - f * (size_t)pairs);
        const int rem = il.n_tx - 2 * M * g;
        float a0, a1, sg0, sg1;
        fade_pair(fad, seed, first_frame + f, g, rem > M, sg, gain ? gain + f * (size_t)n_sym : nullptr, vec2, a0, a1, sg0, sg1);
        int32_t p0[M], p1[M];
        uint32_t label[2];
        float z[4], y[4];
        il_pair_positions<M>(il.pos + (size_t)(2 * M) * g, rem, p0, p1);
        product_pair_draw_il<B>(cw + f * (size_t)PB, p0, p1, g, rem, seed, first_frame + f, label, z);
#pragma unroll 1
        for (int a = 0; a < 2; a++) {
            const float (&lev)[kAxisMaxLevels] = tab.lev[a];
            const float y0 = axis_symbol<B>(lev, axis_index<B>(label[0], a), a ? z[1] : z[0], sg0);
            const float y1 = axis_symbol<B>(lev, axis_index<B>(label[1], a), a ? z[3] : z[2], sg1);
            if (a) { y[1] = y0; y[3] = y1; } else { y[0] = y0; y[2] = y1; }
        }
        store_pair_il<M>(sym + 2 * (f * (size_t)n_sym + 2 * (size_t)g), y, rem, vec4);
    }
}

template <int B, typename OT>
__global__ __launch_bounds__(256) void fading_product_generate_kernel(AxisTab tab, IlTab il, FadeArg fad, const uint8_t *__restrict__ cw, int PB, OT *__restrict__ llr,
                                                                      float *__restrict__ gain, int n_sym, int pairs, int lanes, size_t total, uint64_t seed,
                                                                      uint64_t first_frame, float sg, float inv, float qs, int vec2) {
    constexpr int M = 2 * B;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)lanes;
        const int g = (int)(i - f * (size_t)lanes);
        OT *row = llr + f * (size_t)il.N;
        if (g < pairs) {
            const int32_t *src = il.pos + (size_t)(2 * M) * g;
            const int rem = il.n_tx - 2 * M * g;
            float a0, a1, sg0, sg1;
            fade_pair(fad, seed, first_frame + f, g, rem > M, sg, gain ? gain + f * (size_t)n_sym : nullptr, vec2, a0, a1, sg0, sg1);
            const float inv0 = fade_inv(inv, a0), inv1 = fade_inv(inv, a1);
            int32_t p0[M], p1[M];
            uint32_t label[2];
            float z[4], v0[M], v1[M];
            il_pair_positions<M>(src, rem, p0, p1);
            product_pair_draw_il<B>(cw + f * (size_t)PB, p0, p1, g, rem, seed, first_frame + f, label, z);
            // the 2 M entries are loaded again for the stores below and not kept in registers across the axis loop, as
            // product_generate_il_kernel: the compiler barrier keeps the two loads apart
            __asm__ volatile("" ::: "memory");
#pragma unroll 1
            for (int a = 0; a < 2; a++) {
                const float (&lev)[kAxisMaxLevels] = tab.lev[a];
                float r0[B], r1[B];
                axis_llrs<B>(lev, axis_symbol<B>(lev, axis_index<B>(label[0], a), a ? z[1] : z[0], sg0), inv0, r0);
                axis_llrs<B>(lev, axis_symbol<B>(lev, axis_index<B>(label[1], a), a ? z[3] : z[2], sg1), inv1, r1);
#pragma unroll
                for (int j = 0; j < B; j++) {
                    if (a) { v0[B + j] = r0[j]; v1[B + j] = r1[j]; } else { v0[j] = r0[j]; v1[j] = r1[j]; }
                }
            }
            const int32_t *src2 = src;
            int rem2 = rem;
            __asm__ volatile("" : "+v"(src2), "+v"(rem2) : : "memory");
            il_pair_positions<M>(src2, rem2, p0, p1);
            il_store<M, OT>(row, p0, rem2, v0, qs);
            il_store<M, OT>(row, p1, rem2 - M, v1, qs);      // (nothing for a symbol from n_sym on: rem - M <= 0)
        } else {
            il_store_holes<2 * M, OT>(row, il, 2 * M * (g - pairs), qs);
        }
    }
}

// ---- launchers.  transmit: pairs lanes per frame; generate: pairs + ceil(n_holes / 2M).  vec4: n_sym even and a 16-byte aligned sample
// buffer; vec2: n_sym even and an 8-byte aligned gain buffer (a null one is)
int fading_transmit_launch(hipStream_t st, const ModTab &tab, int m, const IlTab &il, const FadeArg &fad, int batch, const uint8_t *d_cw, int PB, uint64_t seed,
                           uint64_t first_frame, float sg, float *d_sym, float *d_gain) {
    const char *what = "ldpc_sim_transmit_il_fading";
    return launched(what, dispatch_bits(what, m, [&](auto k) {
        constexpr int M = decltype(k)::value;
        const int n_sym = mod_symbols(il.n_tx, M), pairs = mod_pairs(n_sym);
        const size_t total = (size_t)batch * pairs;
        const int rc = check_items(what, total);
        if (rc == LDPC_OK)
            hipLaunchKernelGGL((fading_transmit_kernel<M>), grid_lanes(total), dim3(256), 0, st, tab, il, fad, d_cw, PB, d_sym, d_gain, n_sym, pairs, total, seed, first_frame, sg,
                               grant_pair_store(n_sym, d_sym, 16), grant_pair_store(n_sym, d_gain, 8));
        return rc;
    }));
}

int fading_product_transmit_launch(hipStream_t st, const AxisTab &tab, int b, const IlTab &il, const FadeArg &fad, int batch, const uint8_t *d_cw, int PB, uint64_t seed,
                                   uint64_t first_frame, float sg, float *d_sym, float *d_gain) {
    const char *what = "ldpc_sim_transmit_il_fading";
    return launched(what, dispatch_bits(what, b, [&](auto k) {
        constexpr int B = decltype(k)::value;
        const int n_sym = mod_symbols(il.n_tx, 2 * B), pairs = mod_pairs(n_sym);
        const size_t total = (size_t)batch * pairs;
        const int rc = check_items(what, total);
        if (rc == LDPC_OK)
            hipLaunchKernelGGL((fading_product_transmit_kernel<B>), grid_lanes(total), dim3(256), 0, st, tab, il, fad, d_cw, PB, d_sym, d_gain, n_sym, pairs, total, seed,
                               first_frame, sg, grant_pair_store(n_sym, d_sym, 16), grant_pair_store(n_sym, d_gain, 8));
        return rc;
    }));
}

int fading_generate_launch(hipStream_t st, const ModTab &tab, int m, const IlTab &il, const FadeArg &fad, int batch, const uint8_t *d_cw, int PB, uint64_t seed,
                           uint64_t first_frame, float sg, float inv, void *d_llr, int fmt, float qscale, float *d_gain) {
    const char *what = "ldpc_sim_generate_mod_il_fading";
    return launched(what, dispatch_bits_fmt(what, m, fmt, [&](auto k, auto t) {
        constexpr int M = decltype(k)::value;
        typedef typename decltype(t)::type OT;
        const int n_sym = mod_symbols(il.n_tx, M), pairs = mod_pairs(n_sym), lanes = mod_lanes(pairs, il.n_holes, 2 * M);
        const size_t total = (size_t)batch * lanes;
        const int rc = check_items(what, total);
        if (rc == LDPC_OK)
            hipLaunchKernelGGL((fading_generate_kernel<M, OT>), grid_lanes(total), dim3(256), 0, st, tab, il, fad, d_cw, PB, (OT *)d_llr, d_gain, n_sym, pairs, lanes, total, seed,
                               first_frame, sg, inv, qscale, grant_pair_store(n_sym, d_gain, 8));
        return rc;
    }));
}

int fading_product_generate_launch(hipStream_t st, const AxisTab &tab, int b, const IlTab &il, const FadeArg &fad, int batch, const uint8_t *d_cw, int PB, uint64_t seed,
                                   uint64_t first_frame, float sg, float inv, void *d_llr, int fmt, float qscale, float *d_gain) {
    const char *what = "ldpc_sim_generate_mod_il_fading";
    return launched(what, dispatch_bits_fmt(what, b, fmt, [&](auto k, auto t) {
        constexpr int B = decltype(k)::value, M = 2 * B;
        typedef typename decltype(t)::type OT;
        const int n_sym = mod_symbols(il.n_tx, M), pairs = mod_pairs(n_sym), lanes = mod_lanes(pairs, il.n_holes, 2 * M);
        const size_t total = (size_t)batch * lanes;
        const int rc = check_items(what, total);
        if (rc == LDPC_OK)
            hipLaunchKernelGGL((fading_product_generate_kernel<B, OT>), grid_lanes(total), dim3(256), 0, st, tab, il, fad, d_cw, PB, (OT *)d_llr, d_gain, n_sym, pairs, lanes, total,
                               seed, first_frame, sg, inv, qscale, grant_pair_store(n_sym, d_gain, 8));
        return rc;
    }));
}

}  // namespace ldpc
