// sim_systematic.hip -- the frame source's encoder from ANY parity-check matrix, through the systematic form of
// ldpc_csr_systematic_form (csrc/systematic.cc): message bit i sits at codeword position msg_pos[i], the parity positions hold the
// dense GF(2) product of the message with P.  Message and parity positions may interleave (codes/1920.1280.3.303: eight parity
// positions among the first 640 columns), so this stage emits the WHOLE codeword, packed in H's column order, and the unchanged
// sim_frame_kernel reads every position from it (SimSys, sim.h).
//
// LANE = FRAME, the layout of sim_parity_qc_kernel: a wave holds 64 frames x 16 codeword words in registers, and walks the
// message bits; for message bit i the 16 words of generator row i are the same for every lane -- a wave-uniform address, so they
// come by scalar loads through the constant cache and cost no VALU issue and no LDS bandwidth -- and the lanes whose message
// bit is set XOR them in under an EXEC mask: one v_xor per 32 parity bits.  The dense product of sim_frame_kernel (lane = four
// parity positions, AND + XOR per 32 MESSAGE bits and position) spends twice the VALU work on the same bits and reads its
// generator through the vector memory path.  A bit-sliced layout (32 frames a word, as sim_sparse.hip) would halve the XORs again
// for a P of density 1/2 but turns every one of them into a vector load of a scratch word; byte-indexed tables in LDS need
// 256 x 64 B per eight message bits and column group rebuilt or streamed per workgroup, and their lane-private row index makes
// every LDS read a gather with bank conflicts.  The four waves of a workgroup share frames and column group and split the message
// words; their partial words meet in LDS (XOR is associative: any split gives the same bits).  The only wait is that barrier.
#include "internal.h"
#include "sim.h"

namespace ldpc {

constexpr int kSysSplit = 4;
__global__ __launch_bounds__(64 * kSysSplit) void sim_systematic_codeword_kernel(const uint32_t *__restrict__ gwin, const uint32_t *__restrict__ msgw,
                                                                                  uint32_t *__restrict__ cw, int kwords, int w0, int cww, int batch) {
    __shared__ uint32_t part[kSysSplit - 1][16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f0 = blockIdx.x * 64, f = f0 + lane;
    const int cg = blockIdx.y;
    const bool live = f < batch;
    if (cg == 0) {   // the words before the window are message words as they stand: 64 frames x w0 words, coalesced along the words
        const int nf = min(64, batch - f0);
        for (int idx = threadIdx.x; idx < nf * w0; idx += 64 * kSysSplit) {
            const int fr = idx / w0, w = idx - fr * w0;
            cw[(size_t)(f0 + fr) * cww + w] = msgw[(size_t)(f0 + fr) * kwords + w];
        }
    }
    const int wchunk = (kwords + kSysSplit - 1) / kSysSplit;
    const int w_begin = __builtin_amdgcn_readfirstlane(wave * wchunk), w_end = min(kwords, w_begin + wchunk);
    const uint32_t *mw = msgw + (size_t)(live ? f : 0) * kwords;
    const uint32_t *t = gwin + (size_t)cg * kwords * (32 * 16);
    uint32_t acc[16];
#pragma unroll
    for (int c = 0; c < 16; c++) acc[c] = 0u;
    for (int w = w_begin; w < w_end; w++) {
        const uint32_t v = mw[w];
#pragma unroll
        for (int b0 = 0; b0 < 32; b0 += 4) {
            uint32_t T[4][16];       // four generator rows in flight (64 SGPRs): one wait per four masked regions
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int c = 0; c < 16; c++) T[q][c] = t[(size_t)(w * 32 + b0 + q) * 16 + c];   // uniform address: scalar loads
#pragma unroll
            for (int q = 0; q < 4; q++)
                if ((v >> (b0 + q)) & 1u) {          // the lanes (frames) whose message bit is set: EXEC mask, one v_xor per word
                    asm volatile("" ::: "memory");   // keeps this a real EXEC-masked region (otherwise: v_cndmask + v_xor per word)
#pragma unroll
                    for (int c = 0; c < 16; c++) acc[c] ^= T[q][c];
                }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int c = 0; c < 16; c++) part[wave - 1][c][lane] = acc[c];
    }
    __syncthreads();
    if (wave > 0 || !live) return;
#pragma unroll
    for (int c = 0; c < 16; c++) {
#pragma unroll
        for (int q = 0; q < kSysSplit - 1; q++) acc[c] ^= part[q][c][lane];
        const int wc = w0 + cg * 16 + c;
        if (wc < cww) cw[(size_t)f * cww + wc] = acc[c];
    }
}

// d_msg[frame][i] = message bit i: the message in msg_pos order is the message words unpacked
__global__ __launch_bounds__(256) void sim_systematic_msg_kernel(const uint32_t *__restrict__ msgw, uint8_t *__restrict__ msg_bytes, int kwords, int K, int batch) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)batch * K) return;
    const size_t f = idx / K;
    const int i = (int)(idx - f * K);
    msg_bytes[idx] = (uint8_t)((msgw[f * kwords + (i >> 5)] >> (i & 31)) & 1u);
}

// sim_tally_kernel with the message bits looked up at msg_pos; one wave per frame
__global__ __launch_bounds__(256) void sim_systematic_tally_kernel(const int32_t *__restrict__ msg_pos, int N, int K, int kwords, const uint32_t *__restrict__ msgw,
                                                                   const uint8_t *__restrict__ bits, const int32_t *__restrict__ iters, unsigned long long *tally,
                                                                   int batch) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= batch) return;
    unsigned errs = 0;
    for (int i = lane; i < K; i += 64) {
        const unsigned m = (msgw[(size_t)f * kwords + (i >> 5)] >> (i & 31)) & 1u;
        errs += (bits[(size_t)f * N + msg_pos[i]] != m);
    }
    for (int o = 32; o > 0; o >>= 1) errs += __shfl_down(errs, o, 64);
    if (lane == 0) {
        atomicAdd(&tally[0], 1ull);
        if (errs) atomicAdd(&tally[1], 1ull);
        if (errs) atomicAdd(&tally[2], (unsigned long long)errs);
        if (iters) atomicAdd(&tally[3], (unsigned long long)iters[f]);
    }
}

int sim_systematic_codeword(const SimSys &sy, const uint32_t *msgw, int kwords, uint32_t *cw, hipStream_t st, int batch) {
    hipLaunchKernelGGL(sim_systematic_codeword_kernel, dim3((batch + 63) / 64, sy.ncg), dim3(64 * kSysSplit), 0, st, sy.gwin, msgw, cw, kwords, sy.w0, sy.cww, batch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "sim_systematic_codeword: %s", hipGetErrorString(e));
    return LDPC_OK;
}

int sim_systematic_msg_bytes(const uint32_t *msgw, int kwords, int K, uint8_t *d_msg, hipStream_t st, int batch) {
    const size_t n = (size_t)batch * K;
    hipLaunchKernelGGL(sim_systematic_msg_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, msgw, d_msg, kwords, K, batch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "sim_systematic_msg_bytes: %s", hipGetErrorString(e));
    return LDPC_OK;
}

int sim_systematic_tally(const SimSys &sy, int N, int K, int kwords, const uint32_t *msgw, hipStream_t st, int batch, const uint8_t *d_bits,
                         const int32_t *d_iters, unsigned long long *d_tally) {
    hipLaunchKernelGGL(sim_systematic_tally_kernel, dim3((batch + 3) / 4), dim3(256), 0, st, sy.msg_pos, N, K, kwords, msgw, d_bits, d_iters, d_tally, batch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "sim_systematic_tally: %s", hipGetErrorString(e));
    return LDPC_OK;
}

}  // namespace ldpc
