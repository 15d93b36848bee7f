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
#include "demap_product.h"
#include "interleaver.h"
#include "sim_noise.h"

namespace ldpc {

static unsigned il_grid1(size_t total) { return (unsigned)((total + 255) / 256); }

// pair g's place in the table: src = pos + M 2g, rem = n_tx - M 2g (> 0).  Symbol 2g + 1 is at src + M with rem - M, which is <= 0 from
// n_sym on (the second of the last pair when n_sym is odd): such a symbol has no entries, none are loaded and none looked at
template <int M>
__device__ __forceinline__ void il_pair_positions(const int32_t *__restrict__ src, int rem, int32_t (&p0)[M], int32_t (&p1)[M]) {
    il_positions<M>(src, p0);
#pragma unroll
    for (int j = 0; j < M; j++) p1[j] = 0;
    if (rem > M) il_positions<M>(src + M, p1);
}

// the two noisy symbols of pair g of frame f, as sim_mod.hip mod_pair with the labels gathered; a symbol from n_sym on is not made
template <int M>
__device__ __forceinline__ void mod_pair_il(const ModTab &tab, const uint8_t *__restrict__ row, const int32_t (&p0)[M], const int32_t (&p1)[M], int g, int rem,
                                            uint64_t seed, uint64_t frame, float sg, float (&y)[4]) {
    uint32_t r[4];
    float z[4];
    Philox::gen(seed, frame, (uint32_t)g, 2u, r);
    box_muller4(r, z);
    mod_symbol<M>(tab, il_label<M>(row, p0, rem), z[0], z[1], sg, y[0], y[1]);
    y[2] = 0.f; y[3] = 0.f;
    if (rem > M) mod_symbol<M>(tab, il_label<M>(row, p1, rem - M), z[2], z[3], sg, y[2], y[3]);
}

// vec4: n_sym even and a 16-byte aligned buffer -- every pair is whole and starts on a 16-byte boundary
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
        mod_pair_il<M>(tab, cw + f * (size_t)PB, p0, p1, g, rem, seed, first_frame + f, sg, y);
        float *dst = sym + 2 * (f * (size_t)n_sym + 2 * (size_t)g);
        if (vec4) {
            *reinterpret_cast<float4 *>(dst) = make_float4(y[0], y[1], y[2], y[3]);
        } else {
            *reinterpret_cast<float2 *>(dst) = make_float2(y[0], y[1]);
            if (rem > M) *reinterpret_cast<float2 *>(dst + 2) = make_float2(y[2], y[3]);
        }
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
            mod_pair_il<M>(tab, cw + f * (size_t)PB, p0, p1, g, rem, seed, first_frame + f, sg, y);
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
__device__ __forceinline__ void product_pair_draw_il(const uint8_t *__restrict__ row, const int32_t (&p0)[2 * B], const int32_t (&p1)[2 * B], int g, int rem,
                                                     uint64_t seed, uint64_t frame, uint32_t (&label)[2], float (&z)[4]) {
    uint32_t r[4];
    Philox::gen(seed, frame, (uint32_t)g, 2u, r);
    box_muller4(r, z);
    label[0] = il_label<2 * B>(row, p0, rem);
    label[1] = il_label<2 * B>(row, p1, rem - 2 * B);        // 0 for a symbol from n_sym on; what is computed for it is never stored
}

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
        float *dst = sym + 2 * (f * (size_t)n_sym + 2 * (size_t)g);
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

// ---- launchers
template <int M>
static int transmit_il_m(hipStream_t st, const ModTab &tab, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg, float *d_sym) {
    const int n_sym = (il.n_tx + M - 1) / M, pairs = (n_sym + 1) / 2;
    const size_t total = (size_t)batch * pairs;
    if (total > kIlMaxItems) return set_error(LDPC_EINVAL, "ldpc_sim_transmit_il: %zu items are more than one launch holds", total);
    const int vec4 = (n_sym % 2 == 0) && ((uintptr_t)d_sym % 16 == 0);
    hipLaunchKernelGGL((mod_transmit_il_kernel<M>), dim3(il_grid1(total)), dim3(256), 0, st, tab, il, d_cw, PB, d_sym, n_sym, pairs, total, seed, first_frame, sg, vec4);
    return LDPC_OK;
}

template <int B>
static int transmit_il_b(hipStream_t st, const AxisTab &tab, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg,
                         float *d_sym) {
    constexpr int M = 2 * B;
    const int n_sym = (il.n_tx + M - 1) / M, pairs = (n_sym + 1) / 2;
    const size_t total = (size_t)batch * pairs;
    if (total > kIlMaxItems) return set_error(LDPC_EINVAL, "ldpc_sim_transmit_il: %zu items are more than one launch holds", total);
    const int vec4 = (n_sym % 2 == 0) && ((uintptr_t)d_sym % 16 == 0);
    hipLaunchKernelGGL((product_transmit_il_kernel<B>), dim3(il_grid1(total)), dim3(256), 0, st, tab, il, d_cw, PB, d_sym, n_sym, pairs, total, seed, first_frame, sg, vec4);
    return LDPC_OK;
}

template <int M, typename OT>
static int generate_il_as(hipStream_t st, const ModTab &tab, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg, float inv,
                          void *d_llr, float qs) {
    const int n_sym = (il.n_tx + M - 1) / M, pairs = (n_sym + 1) / 2, lanes = pairs + (il.n_holes + 2 * M - 1) / (2 * M);
    const size_t total = (size_t)batch * lanes;
    if (total > kIlMaxItems) return set_error(LDPC_EINVAL, "ldpc_sim_generate_mod_il: %zu items are more than one launch holds", total);
    hipLaunchKernelGGL((mod_generate_il_kernel<M, OT>), dim3(il_grid1(total)), dim3(256), 0, st, tab, il, d_cw, PB, (OT *)d_llr, pairs, lanes, total, seed, first_frame, sg,
                       inv, qs);
    return LDPC_OK;
}

template <int B, typename OT>
static int generate_il_product_as(hipStream_t st, const AxisTab &tab, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg,
                                  float inv, void *d_llr, float qs) {
    constexpr int M = 2 * B;
    const int n_sym = (il.n_tx + M - 1) / M, pairs = (n_sym + 1) / 2, lanes = pairs + (il.n_holes + 2 * M - 1) / (2 * M);
    const size_t total = (size_t)batch * lanes;
    if (total > kIlMaxItems) return set_error(LDPC_EINVAL, "ldpc_sim_generate_mod_il: %zu items are more than one launch holds", total);
    hipLaunchKernelGGL((product_generate_il_kernel<B, OT>), dim3(il_grid1(total)), dim3(256), 0, st, tab, il, d_cw, PB, (OT *)d_llr, pairs, lanes, total, seed, first_frame, sg,
                       inv, qs);
    return LDPC_OK;
}

template <int M>
static int generate_il_m(hipStream_t st, const ModTab &tab, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg, float inv,
                         void *d_llr, int fmt, float qs) {
    if (fmt == MOD_LLR_I8) return generate_il_as<M, int8_t>(st, tab, il, batch, d_cw, PB, seed, first_frame, sg, inv, d_llr, qs);
    if (fmt == MOD_LLR_F16) return generate_il_as<M, __half>(st, tab, il, batch, d_cw, PB, seed, first_frame, sg, inv, d_llr, qs);
    return generate_il_as<M, float>(st, tab, il, batch, d_cw, PB, seed, first_frame, sg, inv, d_llr, qs);
}

template <int B>
static int generate_il_b(hipStream_t st, const AxisTab &tab, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg, float inv,
                         void *d_llr, int fmt, float qs) {
    if (fmt == MOD_LLR_I8) return generate_il_product_as<B, int8_t>(st, tab, il, batch, d_cw, PB, seed, first_frame, sg, inv, d_llr, qs);
    if (fmt == MOD_LLR_F16) return generate_il_product_as<B, __half>(st, tab, il, batch, d_cw, PB, seed, first_frame, sg, inv, d_llr, qs);
    return generate_il_product_as<B, float>(st, tab, il, batch, d_cw, PB, seed, first_frame, sg, inv, d_llr, qs);
}

#define LDPC_IL_SWITCH(n_, what_, CALL)                                    \
    int rc;                                                                \
    switch (n_) {                                                          \
        case 1: rc = CALL(1); break;                                       \
        case 2: rc = CALL(2); break;                                       \
        case 3: rc = CALL(3); break;                                       \
        case 4: rc = CALL(4); break;                                       \
        case 5: rc = CALL(5); break;                                       \
        case 6: rc = CALL(6); break;                                       \
        default: return set_error(LDPC_EINVAL, "%s: %d bits per symbol or axis", what_, n_); \
    }                                                                      \
    if (rc != LDPC_OK) return rc;                                          \
    hipError_t e = hipGetLastError();                                      \
    if (e != hipSuccess) return set_error(LDPC_EHIP, "%s: %s", what_, hipGetErrorString(e)); \
    return LDPC_OK;

int mod_transmit_il_launch(hipStream_t st, const ModTab &tab, int m, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg,
                           float *d_sym) {
#define LDPC_IL_T(M_) transmit_il_m<M_>(st, tab, il, batch, d_cw, PB, seed, first_frame, sg, d_sym)
    LDPC_IL_SWITCH(m, "ldpc_sim_transmit_il", LDPC_IL_T)
#undef LDPC_IL_T
}

int mod_generate_il_launch(hipStream_t st, const ModTab &tab, int m, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame, float sg,
                           float inv, void *d_llr, int fmt, float qscale) {
#define LDPC_IL_G(M_) generate_il_m<M_>(st, tab, il, batch, d_cw, PB, seed, first_frame, sg, inv, d_llr, fmt, qscale)
    LDPC_IL_SWITCH(m, "ldpc_sim_generate_mod_il", LDPC_IL_G)
#undef LDPC_IL_G
}

int product_transmit_il_launch(hipStream_t st, const AxisTab &tab, int b, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame,
                               float sg, float *d_sym) {
#define LDPC_IL_T(B_) transmit_il_b<B_>(st, tab, il, batch, d_cw, PB, seed, first_frame, sg, d_sym)
    LDPC_IL_SWITCH(b, "ldpc_sim_transmit_il", LDPC_IL_T)
#undef LDPC_IL_T
}

int product_generate_il_launch(hipStream_t st, const AxisTab &tab, int b, const IlTab &il, int batch, const uint8_t *d_cw, int PB, uint64_t seed, uint64_t first_frame,
                               float sg, float inv, void *d_llr, int fmt, float qscale) {
#define LDPC_IL_G(B_) generate_il_b<B_>(st, tab, il, batch, d_cw, PB, seed, first_frame, sg, inv, d_llr, fmt, qscale)
    LDPC_IL_SWITCH(b, "ldpc_sim_generate_mod_il", LDPC_IL_G)
#undef LDPC_IL_G
}

}  // namespace ldpc
