// crc.hip -- CRC attach and check on the device (ldpc_crc_attach_dev, ldpc_crc_check_dev, ldpc_sim_crc_check) and the tally of detected
// and undetected errors (ldpc_sim_tally_crc).  The rule and its linear form: crc.h; restated in tests/crc_spec.py.
//
// The shape is sim_tally_kernel's (sim.hip): a wave owns a frame and its lanes stride over the frame's bits, so a wave instruction
// reads 64 consecutive bytes of the frame (256 with VEC, 8 of a packed row) and 64 (256) consecutive table entries: no lane walks a row.
// Lane i XORs ext[i] of every set bit i it sees, the 64 partial XORs are reduced across the wave by five __shfl_xor steps, after which
// every lane holds the frame's value: the CRC (attach: C0 ^ value, written by the first w lanes, one bit each) or the verdict (check:
// value == C0, written by lane 0).  No LDS, no atomic.  The frame is folded into blockIdx.x (four frames a workgroup), so no grid
// y-limit applies; the host side bounds batch * k by 2^32 - 256 and indexes with size_t all the same.
//
// PACKED rows are read ONE BIT A LANE as well: lane i takes byte i / 8 of the row (eight lanes share a byte, 64 lanes read 8
// consecutive bytes) and entry ext[i].  A lane per WORD would need entry 32 j + b in lane j for every bit b -- a 32-word stride across
// the wave, 64 cache lines an instruction -- or a second, transposed table; a lane per bit reads the one table the bytes format reads,
// consecutively, at the price of loading each data byte eight times from the same cache line.  The table (4 k bytes) is shared by all
// frames and stays in cache.
// VEC (bytes format, no position table, rows and base 4-byte aligned): a lane takes four consecutive bytes with one 4-byte load and
// their four entries with one 16-byte load.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "crc.h"

namespace ldpc {

static __device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v ^= __shfl_xor(v, o, 64);
    return v;
}

// the XOR of ext[i] over the set bits i < limit of frame row `row`
template <bool PACKED, bool VEC>
static __device__ __forceinline__ uint32_t crc_frame_xor(const CrcTab &t, const uint8_t *__restrict__ row, const int32_t *__restrict__ pos, int limit, int lane) {
    uint32_t acc = 0u;
    if constexpr (VEC) {
        for (int i = 4 * lane; i < limit; i += 256) {
            const uint32_t v = *reinterpret_cast<const uint32_t *>(row + i);          // bytes i .. i + 3 (the row holds them: its stride is a multiple of 4)
            const uint4 e = *reinterpret_cast<const uint4 *>(t.ext + i);              // ext is padded to a multiple of 4 entries
            acc ^= (0u - (v & 1u)) & e.x;
            acc ^= (0u - ((v >> 8) & (uint32_t)(i + 1 < limit))) & e.y;
            acc ^= (0u - ((v >> 16) & (uint32_t)(i + 2 < limit))) & e.z;
            acc ^= (0u - ((v >> 24) & (uint32_t)(i + 3 < limit))) & e.w;
        }
    } else {
        for (int i = lane; i < limit; i += 64) {
            const int p = pos ? pos[i] : i;
            const uint32_t b = PACKED ? ((uint32_t)row[p >> 3] >> (p & 7)) & 1u : row[p] & 1u;
            acc ^= (0u - b) & t.ext[i];
        }
    }
    return wave_xor(acc);
}

// in place: reads message bits 0 .. L - 1, writes bits L .. k - 1 (packed: the words from bit L on, payload bits kept, pad bits 0)
template <bool PACKED, bool VEC>
__global__ __launch_bounds__(256) void crc_attach_kernel(CrcTab t, uint8_t *msg, size_t stride, int batch) {
    const int lane = threadIdx.x & 63;
    const size_t f = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= (size_t)batch) return;
    uint8_t *row = msg + f * stride;
    const uint32_t crc = t.c0 ^ crc_frame_xor<PACKED, VEC>(t, row, nullptr, t.L, lane);
    if constexpr (PACKED) {
        // message bit L + j = crc bit w - 1 - j: the w-bit reversal of crc, placed at bit L.  It spans at most two words (w <= 32)
        const int w0 = t.L >> 5, sh = t.L & 31, nw = ((t.k + 31) >> 5) - w0;   // nw = 1 or 2
        if (lane < nw) {
            uint32_t *words = reinterpret_cast<uint32_t *>(row);
            const uint64_t field = (uint64_t)(__brev(crc) >> (32 - t.w)) << sh;
            uint32_t v = lane == 0 ? (uint32_t)field : (uint32_t)(field >> 32);
            if (lane == 0 && sh) v |= words[w0] & ((1u << sh) - 1u);
            words[w0 + lane] = v;
        }
    } else {
        if (lane < t.w) row[t.L + lane] = (uint8_t)((crc >> (t.w - 1 - lane)) & 1u);
    }
}

template <bool PACKED, bool VEC>
__global__ __launch_bounds__(256) void crc_check_kernel(CrcTab t, const uint8_t *__restrict__ src, size_t stride, const int32_t *__restrict__ pos,
                                                        uint8_t *__restrict__ ok, int batch) {
    const int lane = threadIdx.x & 63;
    const size_t f = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= (size_t)batch) return;
    const uint32_t x = crc_frame_xor<PACKED, VEC>(t, src + f * stride, pos, t.k, lane);
    if (lane == 0) ok[f] = (uint8_t)(x == t.c0);
}

// sim_tally_kernel with the frame's flag: tally[0..3] += {frames, ok, frames with a message-bit error, ok and in error}
__global__ __launch_bounds__(256) void crc_tally_kernel(const int32_t *__restrict__ msg_pos, int N, int k, int kwords, const uint32_t *__restrict__ msgw,
                                                        const uint8_t *__restrict__ bits, const uint8_t *__restrict__ ok, unsigned long long *tally, int batch) {
    const int lane = threadIdx.x & 63;
    const size_t f = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= (size_t)batch) return;
    unsigned errs = 0;
    for (int i = lane; i < k; i += 64) {
        const unsigned m = (msgw[f * kwords + (i >> 5)] >> (i & 31)) & 1u;
        errs += (bits[f * N + (msg_pos ? msg_pos[i] : i)] != m);
    }
    for (int o = 32; o > 0; o >>= 1) errs += __shfl_down(errs, o, 64);
    if (lane == 0) {
        const bool pass = ok[f] != 0;
        atomicAdd(&tally[0], 1ull);
        if (pass) atomicAdd(&tally[1], 1ull);
        if (errs) atomicAdd(&tally[2], 1ull);
        if (pass && errs) atomicAdd(&tally[3], 1ull);
    }
}

static int crc_launched(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "%s: %s", what, hipGetErrorString(e));
    return LDPC_OK;
}

int crc_attach_launch(hipStream_t st, const CrcTab &t, int batch, void *d_msg, bool packed) {
    const dim3 grid(((unsigned)batch + 3u) / 4u), block(256);
    uint8_t *msg = (uint8_t *)d_msg;
    if (packed) hipLaunchKernelGGL((crc_attach_kernel<true, false>), grid, block, 0, st, t, msg, (size_t)4 * ((t.k + 31) / 32), batch);
    else if (t.k % 4 == 0 && (uintptr_t)d_msg % 4 == 0) hipLaunchKernelGGL((crc_attach_kernel<false, true>), grid, block, 0, st, t, msg, (size_t)t.k, batch);
    else hipLaunchKernelGGL((crc_attach_kernel<false, false>), grid, block, 0, st, t, msg, (size_t)t.k, batch);
    return crc_launched("ldpc_crc_attach_dev");
}

int crc_check_launch(hipStream_t st, const CrcTab &t, int batch, const uint8_t *src, size_t stride, bool packed, const int32_t *pos, uint8_t *d_ok) {
    const dim3 grid(((unsigned)batch + 3u) / 4u), block(256);
    if (packed) hipLaunchKernelGGL((crc_check_kernel<true, false>), grid, block, 0, st, t, src, stride, pos, d_ok, batch);
    else if (!pos && stride % 4 == 0 && (uintptr_t)src % 4 == 0) hipLaunchKernelGGL((crc_check_kernel<false, true>), grid, block, 0, st, t, src, stride, pos, d_ok, batch);
    else hipLaunchKernelGGL((crc_check_kernel<false, false>), grid, block, 0, st, t, src, stride, pos, d_ok, batch);
    return crc_launched("crc_check");
}

int crc_tally_launch(hipStream_t st, const int32_t *msg_pos, int N, int k, int kwords, const uint32_t *msgw, int batch, const uint8_t *d_bits, const uint8_t *d_ok,
                     unsigned long long *d_tally) {
    hipLaunchKernelGGL(crc_tally_kernel, dim3(((unsigned)batch + 3u) / 4u), dim3(256), 0, st, msg_pos, N, k, kwords, msgw, d_bits, d_ok, d_tally, batch);
    return crc_launched("ldpc_sim_tally_crc");
}

}  // namespace ldpc
