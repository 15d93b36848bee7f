// fading.h -- the fading channel of include/ldpc_hip.h (ldpc_fading) and the per-symbol channel state of the demapper: the descriptor as
// a kernel argument and the device functions of the gain rule, one copy shared by the kernels of demap_csi.hip and sim_mod_fading.hip, so
// that the fused kernel equals ldpc_sim_transmit_il_fading + ldpc_demap_dev_il_csi bit for bit.  A coherent receiver with perfect channel
// knowledge is modelled: the samples are delivered equalised, and of the channel only the POWER gain a of a symbol appears -- its noise
// variance per real dimension is sigma^2 / a.  The rule is restated in tests/fading_spec.py.
#pragma once
#include "interleaver.h"
#include "sim_noise.h"

namespace ldpc {

// the descriptor as a kernel argument: mu = float32(sqrt(K / (K + 1))), sd = float32(sqrt(1 / (2 (K + 1)))), each computed in double on
// the host and rounded once
struct FadeArg {
    int block;      // symbols per fading block, >= 1
    float mu, sd;
};

// ldpc_demap_dev_il_csi: demap_il_launch / demap_il_product_launch (interleaver.h) with the LLRs of symbol s of frame f scaled by
// inv_s = fl(inv d_gain[f][s])
int demap_csi_launch(hipStream_t st, const ModTab &tab, int m, int rule, const IlTab &il, int batch, const float *d_sym, const float *d_gain, float inv, void *d_llr, int fmt,
                     float qscale);
int demap_csi_product_launch(hipStream_t st, const AxisTab &tab, int b, int rule, const IlTab &il, int batch, const float *d_sym, const float *d_gain, float inv, void *d_llr, int fmt,
                             float qscale);
// ldpc_demap_dev_il_apriori (demap_apriori.hip): demap_csi_launch for a table object with d_apriori [batch][N] float32, the bit knowledge in
// codeword order; d_gain may be null (a = 1)
int demap_apriori_launch(hipStream_t st, const ModTab &tab, int m, int rule, const IlTab &il, int batch, const float *d_sym, const float *d_gain, const float *d_apriori,
                         float inv, void *d_llr, int fmt, float qscale);
// ldpc_sim_transmit_il_fading / ldpc_sim_generate_mod_il_fading: as mod_transmit_il_launch / mod_generate_il_launch and their product
// forms; d_gain [batch][n_sym] may be null
int fading_transmit_launch(hipStream_t st, const ModTab &tab, int m, const IlTab &il, const FadeArg &fad, int batch, const uint8_t *d_cw, int PB, uint64_t seed,
                           uint64_t first_frame, float sg, float *d_sym, float *d_gain);
int fading_generate_launch(hipStream_t st, const ModTab &tab, int m, const IlTab &il, const FadeArg &fad, int batch, const uint8_t *d_cw, int PB, uint64_t seed,
                           uint64_t first_frame, float sg, float inv, void *d_llr, int fmt, float qscale, float *d_gain);
int fading_product_transmit_launch(hipStream_t st, const AxisTab &tab, int b, const IlTab &il, const FadeArg &fad, int batch, const uint8_t *d_cw, int PB, uint64_t seed,
                                   uint64_t first_frame, float sg, float *d_sym, float *d_gain);
int fading_product_generate_launch(hipStream_t st, const AxisTab &tab, int b, const IlTab &il, const FadeArg &fad, int batch, const uint8_t *d_cw, int PB, uint64_t seed,
                                   uint64_t first_frame, float sg, float inv, void *d_llr, int fmt, float qscale, float *d_gain);

#ifdef __HIPCC__
// the floor of a gain, 2^-20: a Box-Muller radius of 0 gives a = 0 for K = 0, and sg / sqrt(0) no finite sample
constexpr float kFadeFloor = 9.5367431640625e-07f;

// the gain of a block from its two normals: hI = fl(mu + fl(sd z0)), hQ = fl(sd z1), a = max(fl(fl(hI hI) + fl(hQ hQ)), 2^-20)
static __device__ __forceinline__ float fade_gain(const FadeArg &fad, float z0, float z1) {
    const float hI = fad.mu + fad.sd * z0, hQ = fad.sd * z1;
    const float a = hI * hI + hQ * hQ;
    return __builtin_fmaxf(a, kFadeFloor);
}

// the gains of symbols s0 and s0 + 1 of a frame (s0 even: a symbol pair of sim_mod_il.hip).  Symbol s lies in block q = s / block; block
// pair Q = blocks 2Q and 2Q + 1 takes one Philox call, counter (frame lo, frame hi, Q, stream 3), and box_muller4: (z0, z1) -> block 2Q,
// (z2, z3) -> block 2Q + 1.  ONE call serves both symbols for every block length: they lie in different blocks only if block divides
// s0 + 1, which is odd, so block is odd and q1 = (s0 + 1) / block is odd: q0 = q1 - 1 is even, the other half of the same block pair
static __device__ __forceinline__ void fade_pair_gains(const FadeArg &fad, uint64_t seed, uint64_t frame, int s0, float &a0, float &a1) {
    const uint32_t q0 = (uint32_t)s0 / (uint32_t)fad.block, q1 = ((uint32_t)s0 + 1u) / (uint32_t)fad.block;
    uint32_t r[4];
    float z[4];
    Philox::gen(seed, frame, q0 >> 1, 3u, r);
    box_muller4(r, z);
    a0 = (q0 & 1u) ? fade_gain(fad, z[2], z[3]) : fade_gain(fad, z[0], z[1]);
    a1 = (q1 & 1u) ? fade_gain(fad, z[2], z[3]) : fade_gain(fad, z[0], z[1]);
}

// the channel's sigma of a symbol: sg_s = fl(sg / fl(sqrt a)); a = 1 gives sg
static __device__ __forceinline__ float fade_sigma(float sg, float a) { return sg / sqrtf(a); }

// the demapper's scale of a symbol: inv_s = fl(inv a); a = 0 gives 0 (an erasure), a NaN gain NaN
static __device__ __forceinline__ float fade_inv(float inv, float a) { return inv * a; }
#endif  // __HIPCC__
}  // namespace ldpc
