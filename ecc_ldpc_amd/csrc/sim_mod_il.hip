// sim_mod_il.hip -- the frame source's modulated path through a bit interleaver (ldpc_sim_transmit_il, ldpc_sim_generate_mod_il): packed
// codewords -> labels gathered through the position table -> constellation symbols -> complex AWGN -> (generate_mod_il) max-log LLRs
// stored through the same table, in one kernel.
// LANE = SYMBOL PAIR and the channel are sim_mod.hip's, unchanged: one Philox call, counter (frame lo, frame hi, g, stream 2), feeds the
// four normals of symbols 2g and 2g + 1.  The symbol rule and the LLR rule are the device functions of demap.h and demap_product.h, the
// table's those of interleaver.h, the ones the kernels of demap_il.hip call: the fused kernel equals ldpc_sim_transmit_il +
// ldpc_demap_dev_il bit for bit, and with the identity table both equal the kernels of sim_mod.hip / sim_mod_product.hip.
// A lane loads the 2 m table entries of its pair (vector loads where m allows); the label gather is branch-free, one byte load a bit.  The
// table kernels keep the entries for the LLR stores; the fused product kernel loads them a second time after its axis loop (a cache hit)
// so that they are not live next to the 2^b distances.  In generate_mod_il the lanes from ceil(n_sym / 2) on take the hole list, 2 m
// holes a lane.  ONE ITEM A LANE, no grid-stride loop (demap_product.hip says why).
#include "mod_dispatch.h"
#include "sim_mod_pair.h"

namespace ldpc {

template <int M>
__global__ __launch_bounds__(256) void mod_transmit_il_kernel(ModTab tab, IlTab il, const uint8_t *__restrict__ cw, int PB, float *__restrict__ sym, int n_sym, int pairs,
                                                              size_t total, uint64_t seed, uint64_t first_frame, float sg, int vec4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)pairs;
        const int g = (int)(i - f * (size_t)pairs);
        const int rem = il.n_tx - 2 * M * g;
        int32_t p0[M], p1[M];
        float y[4];
        il_pair_positions<M>(il.pos + (size_t)(2 * M) * g, rem, p0, p1);
        mod_pair_il<M>(tab, cw + f * (size_t)PB, p0, p1, g, rem, seed, first_frame + f, sg, sg, y);
        store_pair_il<M>(sym + 2 * (f * (size_t)n_sym + 2 * (size_t)g), y, rem, vec4);
    }
}

// lanes = pairs + ceil(n_holes / 2M) per frame
template <int M, typename OT>
__global__ __launch_bounds__(256) void mod_generate_il_kernel(ModTab tab, IlTab il, const uint8_t *__restrict__ cw, int PB, OT *__restrict__ llr, int pairs, int lanes,
                                                              size_t total, uint64_t seed, uint64_t first_frame, float sg, float inv, float qs) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)lanes;
        const int g = (int)(i - f * (size_t)lanes);
        OT *row = llr + f * (size_t)il.N;
        if (g < pairs) {
            const int rem = il.n_tx - 2 * M * g;
            int32_t p0[M], p1[M];
            float y[4], v[M];
            il_pair_positions<M>(il.pos + (size_t)(2 * M) * g, rem, p0, p1);
            mod_pair_il<M>(tab, cw + f * (size_t)PB, p0, p1, g, rem, seed, first_frame + f, sg, sg, y);
            demap_llrs<M>(tab, y[0], y[1], inv, v);
            il_store<M, OT>(row, p0, rem, v, qs);
            if (rem > M) {
                demap_llrs<M>(tab, y[2], y[3], inv, v);
                il_store<M, OT>(row, p1, rem - M, v, qs);
            }
        } else {
            il_store_holes<2 * M, OT>(row, il, 2 * M * (g - pairs), qs);
        }
    }
}

// ---- product constellations: sim_mod_product.hip's kernels, AXIS-MAJOR in a loop of two turns that is NOT unrolled (2^B levels in
// scalar registers at a time), with the labels gathered and the LLRs stored through the table
template <int B>
__global__ __launch_bounds__(256) void product_transmit_il_kernel(AxisTab tab, IlTab il, const uint8_t *__restrict__ cw, int PB, float *__restrict__ sym, int n_sym,
                                                                  int pairs, size_t total, uint64_t seed, uint64_t first_frame, float sg, int vec4) {
    constexpr int M = 2 * B;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)pairs;
        const int g = (int)(i - f * (size_t)pairs);
        const int rem = il.n_tx - 2 * M * g;
        int32_t p0[M], p1[M];
        uint32_t label[2];
        float z[4], y[4];
        il_pair_positions<M>(il.pos + (size_t)(2 * M) * g, rem, p0, p1);
        product_pair_draw_il<B>(cw + f * (size_t)PB, p0, p1, g, rem, seed, first_frame + f, label, z);
#pragma unroll 1
        for (int a = 0; a < 2; a++) {
            const float (&lev)[kAxisMaxLevels] = tab.lev[a];
            const float y0 = axis_symbol<B>(lev, axis_index<B>(label[0], a), a ? z[1] : z[0], sg);
            const float y1 = axis_symbol<B>(lev, axis_index<B>(label[1], a), a ? z[3] : z[2], sg);
            if (a) { y[1] = y0; y[3] = y1; } else { y[0] = y0; y[2] = y1; }
        }
        float *dst = sym + 2 * (f * (size_t)n_sym + 2 * (size_t)g);      // (not store_pair_il: through it this kernel compiles to other code)
        if (vec4) {
            *reinterpret_cast<float4 *>(dst) = make_float4(y[0], y[1], y[2], y[3]);
        } else {
            *reinterpret_cast<float2 *>(dst) = make_float2(y[0], y[1]);
            if (rem > M) *reinterpret_cast<float2 *>(dst + 2) = make_float2(y[2], y[3]);
        }
    }
}

template <int B, typename OT>
__global__ __launch_bounds__(256) void product_generate_il_kernel(AxisTab tab, IlTab il, const uint8_t *__restrict__ cw, int PB, OT *__restrict__ llr, int pairs, int lanes,
                                                                  size_t total, uint64_t seed, uint64_t first_frame, float sg, float inv, float qs) {
    constexpr int M = 2 * B;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)lanes;
        const int g = (int)(i - f * (size_t)lanes);
        OT *row = llr + f * (size_t)il.N;
        if (g < pairs) {
            const int32_t *src = il.pos + (size_t)(2 * M) * g;
            const int rem = il.n_tx - 2 * M * g;
            int32_t p0[M], p1[M];
            uint32_t label[2];
            float z[4], v0[M], v1[M];
            il_pair_positions<M>(src, rem, p0, p1);
            product_pair_draw_il<B>(cw + f * (size_t)PB, p0, p1, g, rem, seed, first_frame + f, label, z);
            // the 2 M entries are loaded again for the stores below (they hit the cache) and not kept in registers across the axis loop,
            // where 2^B distances are live: the compiler barrier keeps the two loads apart
            __asm__ volatile("" ::: "memory");
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

// ---- launchers.  transmit: pairs lanes per frame; generate: pairs + ceil(n_holes / 2M)
int mod_transmit_il_launch(hipStream_t st, const ModTab &tab, int m, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg,
                           float *d_sym) {
    const char *what = "ldpc_sim_transmit_il";
    return launched(what, dispatch_bits(what, m, [&](auto k) {
        constexpr int M = decltype(k)::value;
        const int n_sym = mod_symbols(il.n_tx, M), pairs = mod_pairs(n_sym);
        const size_t total = (size_t)batch * pairs;
        const int rc = check_items(what, total);
        if (rc == LDPC_OK)
            hipLaunchKernelGGL((mod_transmit_il_kernel<M>), grid_lanes(total), dim3(256), 0, st, tab, il, d_cw, PB, d_sym, n_sym, pairs, total, seed, first_frame, sg,
                               grant_pair_store(n_sym, d_sym, 16));
        return rc;
    }));
}

int product_transmit_il_launch(hipStream_t st, const AxisTab &tab, int b, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame,
                               float sg, float *d_sym) {
    const char *what = "ldpc_sim_transmit_il";
    return launched(what, dispatch_bits(what, b, [&](auto k) {
        constexpr int B = decltype(k)::value;
        const int n_sym = mod_symbols(il.n_tx, 2 * B), pairs = mod_pairs(n_sym);
        const size_t total = (size_t)batch * pairs;
        const int rc = check_items(what, total);
        if (rc == LDPC_OK)
            hipLaunchKernelGGL((product_transmit_il_kernel<B>), grid_lanes(total), dim3(256), 0, st, tab, il, d_cw, PB, d_sym, n_sym, pairs, total, seed, first_frame, sg,
                               grant_pair_store(n_sym, d_sym, 16));
        return rc;
    }));
}

int mod_generate_il_launch(hipStream_t st, const ModTab &tab, int m, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg,
                           float inv, void *d_llr, int fmt, float qscale) {
    const char *what = "ldpc_sim_generate_mod_il";
    return launched(what, dispatch_bits_fmt(what, m, fmt, [&](auto k, auto t) {
        constexpr int M = decltype(k)::value;
        typedef typename decltype(t)::type OT;
        const int pairs = mod_pairs(mod_symbols(il.n_tx, M)), lanes = mod_lanes(pairs, il.n_holes, 2 * M);
        const size_t total = (size_t)batch * lanes;
        const int rc = check_items(what, total);
        if (rc == LDPC_OK)
            hipLaunchKernelGGL((mod_generate_il_kernel<M, OT>), grid_lanes(total), dim3(256), 0, st, tab, il, d_cw, PB, (OT *)d_llr, pairs, lanes, total, seed, first_frame, sg, inv,
                               qscale);
        return rc;
    }));
}

int product_generate_il_launch(hipStream_t st, const AxisTab &tab, int b, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame,
                               float sg, float inv, void *d_llr, int fmt, float qscale) {
    const char *what = "ldpc_sim_generate_mod_il";
    return launched(what, dispatch_bits_fmt(what, b, fmt, [&](auto k, auto t) {
        constexpr int B = decltype(k)::value, M = 2 * B;
        typedef typename decltype(t)::type OT;
        const int pairs = mod_pairs(mod_symbols(il.n_tx, M)), lanes = mod_lanes(pairs, il.n_holes, 2 * M);
        const size_t total = (size_t)batch * lanes;
        const int rc = check_items(what, total);
        if (rc == LDPC_OK)
            hipLaunchKernelGGL((product_generate_il_kernel<B, OT>), grid_lanes(total), dim3(256), 0, st, tab, il, d_cw, PB, (OT *)d_llr, pairs, lanes, total, seed, first_frame, sg,
                               inv, qscale);
        return rc;
    }));
}

}  // namespace ldpc
