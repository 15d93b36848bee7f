// sim_mod_pair.h -- what a lane of the frame source's interleaved paths draws for its symbol pair: one copy for the AWGN kernels
// (sim_mod_il.hip) and the fading ones (sim_mod_fading.hip), which differ only in the sigma they hand in.  The pair's table entries are
// interleaver.h il_pair_positions'; the noise is sim_mod.hip's: ONE Philox call, counter (frame lo, frame hi, g, stream 2), feeds the
// four normals (z0, z1) -> I, Q of symbol 2g, (z2, z3) -> I, Q of 2g + 1.
#pragma once
#include "demap_product.h"
#include "interleaver.h"
#include "sim_noise.h"

#ifdef __HIPCC__
namespace ldpc {

// the two noisy symbols of pair g of frame f, as sim_mod.hip mod_pair with the labels gathered and a sigma per symbol (the AWGN kernels
// pass sg twice); a symbol from n_sym on is not made
template <int M>
__device__ __forceinline__ void mod_pair_il(const ModTab &tab, const uint8_t *__restrict__ row, const int32_t (&p0)[M], const int32_t (&p1)[M], int g, int rem,
                                            uint64_t seed, uint64_t frame, float sg0, float sg1, float (&y)[4]) {
    uint32_t r[4];
    float z[4];
    Philox::gen(seed, frame, (uint32_t)g, 2u, r);
    box_muller4(r, z);
    mod_symbol<M>(tab, il_label<M>(row, p0, rem), z[0], z[1], sg0, y[0], y[1]);
    y[2] = 0.f; y[3] = 0.f;
    if (rem > M) mod_symbol<M>(tab, il_label<M>(row, p1, rem - M), z[2], z[3], sg1, y[2], y[3]);
}

// the pair's samples to dst = the place of symbol 2g.  vec4 (n_sym even and a 16-byte aligned buffer: every pair is whole and starts on
// a 16-byte boundary): one store; otherwise one a symbol, the second only if it exists (rem > M)
template <int M>
__device__ __forceinline__ void store_pair_il(float *__restrict__ dst, const float (&y)[4], int rem, int vec4) {
    if (vec4) {
        *reinterpret_cast<float4 *>(dst) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
        *reinterpret_cast<float2 *>(dst) = make_float2(y[0], y[1]);
        if (rem > M) *reinterpret_cast<float2 *>(dst + 2) = make_float2(y[2], y[3]);
    }
}

// product constellations: the two labels and the four normals of the pair; the kernels turn them into symbols axis by axis
template <int B>
__device__ __forceinline__ void product_pair_draw_il(const uint8_t *__restrict__ row, const int32_t (&p0)[2 * B], const int32_t (&p1)[2 * B], int g, int rem,
                                                     uint64_t seed, uint64_t frame, uint32_t (&label)[2], float (&z)[4]) {
    uint32_t r[4];
    Philox::gen(seed, frame, (uint32_t)g, 2u, r);
    box_muller4(r, z);
    label[0] = il_label<2 * B>(row, p0, rem);
    label[1] = il_label<2 * B>(row, p1, rem - 2 * B);        // 0 for a symbol from n_sym on; what is computed for it is never stored
}

}  // namespace ldpc
#endif  // __HIPCC__
