// sim_noise.h -- the frame sources' randomness (sim.hip, sim_mod.hip): Philox4x32-10 and the four normals of one call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ldpc {

struct Philox {
    static __device__ __forceinline__ void round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
        const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
        uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
        uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
        uint32_t n0 = hi1 ^ c[1] ^ k0, n1 = lo1, n2 = hi0 ^ c[3] ^ k1, n3 = lo0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    }
    static __device__ __forceinline__ void gen(uint64_t seed, uint64_t frame, uint32_t idx, uint32_t stream, uint32_t (&out)[4]) {
        uint32_t c[4] = {(uint32_t)frame, (uint32_t)(frame >> 32), idx, stream};
        uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
        for (int r = 0; r < 10; r++) {
            round(c, k0, k1);
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
    }
};

// counter streams: 0 = message words, 1 = the BPSK source's noise (one call per four positions), 2 = the modulated path's noise (one
// call per symbol pair), 3 = fading gains (one call per pair of fading blocks: fading.h)
// Box-Muller on two pairs of 32-bit uniforms (u1 in (0,1]); both branches of each pair are used: z[0], z[1] = cos and sin branch
// of (r0, r1), z[2], z[3] of (r2, r3)
static __device__ __forceinline__ void box_muller4(const uint32_t (&r)[4], float (&z)[4]) {
    const float ua = ((float)r[0] + 1.0f) * 2.3283064365386963e-10f, ub = (float)r[1] * 2.3283064365386963e-10f;
    const float uc = ((float)r[2] + 1.0f) * 2.3283064365386963e-10f, ud = (float)r[3] * 2.3283064365386963e-10f;
    const float ra = sqrtf(-2.0f * logf(ua)), rc = sqrtf(-2.0f * logf(uc));
    float sa, ca, sc, cc;
    sincospif(2.0f * ub, &sa, &ca);
    sincospif(2.0f * ud, &sc, &cc);
    z[0] = ra * ca; z[1] = ra * sa; z[2] = rc * cc; z[3] = rc * sc;
}

}  // namespace ldpc
