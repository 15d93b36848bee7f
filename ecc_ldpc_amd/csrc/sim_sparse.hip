// sim_sparse.hip -- the frame source's encoder FROM H, for a parity-check matrix whose parity part is lower-triangular after a
// row permutation (DVB-S2-shaped IRA codes, codes/moon.7.13; the rule: ldpc_csr_triangular_order, include/ldpc_hip.h).
//
//   c[0..K) = msg;  for j = 0 .. M-1:  c[K+j] = XOR of c[col] over the other columns of row order[j]  (all of them < K + j)
//
// The solve is sequential in j (M up to 32 400), so the parallelism comes from the frames.  BIT-SLICED: one 32-bit word holds one
// position of 32 frames, scratch X[position][frame word] (position-major, FW = ceil(frames / 32) words per position).  In this
// layout the column indices of a row are wave-uniform (scalar loads), every bit gather is one coalesced load of 64 frame words,
// and a row update is a handful of v_xor.  Four kernels per chunk of at most 32 * fw_cap frames, all on the caller's stream:
//   in      32 x 32 bit transposes in registers: msgw[frame][word] -> X[0..K)           (msgw keeps its layout: tally, frame kernel)
//   msg     s_j = XOR of the message columns of row order[j] -> X[K + j]                (parallel over (j, frame word))
//   solve   lane = frame word, j ascending: p_j = s_j ^ (earlier parity bits of the row), in place.  p_{j-1} -- the whole
//           dependency chain of a staircase -- stays in a register; any other earlier parity bit is a word THIS lane stored
//           earlier in this kernel, read back through memory in program order: no barrier, no atomic, no fence, and nothing here
//           waits on another wave.  (Hence no __restrict__ / const on the pointer the solve reads and writes through.)
//   out     X[K..N) -> packed parw[frame][ceil(M/32)], the format sim_frame_kernel consumes
// Every loop bound is known to the host (M, row weights, FW).  Absent frames of a ragged last frame word are zero bits; nothing is
// written for frames >= batch.
#include "internal.h"
#include "sim.h"

namespace ldpc {

// a[i] bit b  <->  a[b] bit i  (LSB first), five rounds of masked block swaps; fully unrolled: a[] stays in registers
static __device__ __forceinline__ void transpose32(uint32_t (&a)[32]) {
    uint32_t m = 0x0000FFFFu;
#pragma unroll
    for (int j = 16; j != 0; j >>= 1, m ^= m << j) {
#pragma unroll
        for (int k = 0; k < 32; k = (k + j + 1) & ~j) {
            const uint32_t t = ((a[k] >> j) ^ a[k + j]) & m;
            a[k] ^= t << j;
            a[k + j] ^= t;
        }
    }
}

// thread = (message word w, frame word fw), fw fastest: the 32 stores of a thread are coalesced across the wave; its 32 loads
// (one per frame) are strided, every 64-byte line of msgw is used by the 16 threads of consecutive w
__global__ __launch_bounds__(256) void sim_sparse_in_kernel(const uint32_t *__restrict__ msgw, uint32_t *__restrict__ X, int kwords, int K, int FW, int batch) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)kwords * FW) return;
    const int fw = (int)(idx % FW), w = (int)(idx / FW);
    uint32_t a[32];
#pragma unroll
    for (int i = 0; i < 32; i++) {
        const int f = 32 * fw + i;
        a[i] = f < batch ? msgw[(size_t)f * kwords + w] : 0u;
    }
    transpose32(a);
#pragma unroll
    for (int b = 0; b < 32; b++)
        if (32 * w + b < K) X[(size_t)(32 * w + b) * FW + fw] = a[b];
}

// one wave = one row j (wave-uniform: its column list comes by scalar loads) x 64 frame words
__global__ __launch_bounds__(256) void sim_sparse_msg_kernel(const uint32_t *__restrict__ X, uint32_t *__restrict__ S, const int32_t *__restrict__ a_ptr,
                                                             const int32_t *__restrict__ a_col, int M, int FW, int tiles) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = (int)(blockIdx.x / tiles) * 4 + wave;
    const int fw = (int)(blockIdx.x % tiles) * 64 + (threadIdx.x & 63);
    if (j >= M || fw >= FW) return;
    uint32_t acc = 0u;
    for (int q = a_ptr[j]; q < a_ptr[j + 1]; q++) acc ^= X[(size_t)a_col[q] * FW + fw];
    S[(size_t)j * FW + fw] = acc;
}

// meta[j]: bit 31 = row order[j] holds parity bit j - 1 (taken from the register); low bits = where its other earlier parity
// bits start in far[] (they end where those of j + 1 start).  P = X + K * FW: on entry P[j] = s_j, on exit P[j] = p_j.
// kSolveAhead rows' s_j and meta words are loaded before the block's first store, so that one memory round trip covers the block
// (they are words no earlier row of the block writes: row j's word is written at step j only).
constexpr int kSolveAhead = 16;
__global__ __launch_bounds__(64) void sim_sparse_solve_kernel(uint32_t *P, const int32_t *__restrict__ meta, const int32_t *__restrict__ far, int M, int FW) {
    const int fw = blockIdx.x * 64 + threadIdx.x;
    if (fw >= FW) return;
    P += fw;
    uint32_t p = 0u;
    auto row = [&](int j, uint32_t s, int m0, int m1) {
        p = s ^ (m0 < 0 ? p : 0u);
        for (int q = m0 & 0x7fffffff; q < (m1 & 0x7fffffff); q++) p ^= P[(size_t)far[q] * FW];
        P[(size_t)j * FW] = p;
    };
    int j = 0;
    for (; j + kSolveAhead <= M; j += kSolveAhead) {
        uint32_t s[kSolveAhead];
        int mt[kSolveAhead + 1];
#pragma unroll
        for (int u = 0; u <= kSolveAhead; u++) mt[u] = meta[j + u];
#pragma unroll
        for (int u = 0; u < kSolveAhead; u++) s[u] = P[(size_t)(j + u) * FW];
#pragma unroll
        for (int u = 0; u < kSolveAhead; u++) row(j + u, s[u], mt[u], mt[u + 1]);
    }
    for (; j < M; j++) row(j, P[(size_t)j * FW], meta[j], meta[j + 1]);
}

// thread = (parity word pw, frame word fw), pw fastest: the 32 stores of a thread (one per frame) are coalesced across the
// wave; its 32 loads are strided, every 64-byte line of X is used by the 16 threads of consecutive fw
__global__ __launch_bounds__(256) void sim_sparse_out_kernel(const uint32_t *__restrict__ P, uint32_t *__restrict__ parw, int pwords, int M, int FW, int batch) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)pwords * FW) return;
    const int pw = (int)(idx % pwords), fw = (int)(idx / pwords);
    uint32_t a[32];
#pragma unroll
    for (int b = 0; b < 32; b++) {
        const int j = 32 * pw + b;
        a[b] = j < M ? P[(size_t)j * FW + fw] : 0u;
    }
    transpose32(a);
#pragma unroll
    for (int i = 0; i < 32; i++) {
        const int f = 32 * fw + i;
        if (f < batch) parw[(size_t)f * pwords + pw] = a[i];
    }
}

int sim_sparse_parity(const SimSparse &sp, const uint32_t *msgw, int kwords, uint32_t *parw, int pwords, hipStream_t st, int batch) {
    const int chunk = 32 * sp.fw_cap;   // the scratch holds this many frames: larger batches go through it in turns
    for (int f0 = 0; f0 < batch; f0 += chunk) {
        const int b = min(chunk, batch - f0), FW = (b + 31) / 32, tiles = (FW + 63) / 64;
        const uint32_t *mw = msgw + (size_t)f0 * kwords;
        uint32_t *P = sp.x + (size_t)sp.K * FW;
        hipLaunchKernelGGL(sim_sparse_in_kernel, dim3((unsigned)(((size_t)kwords * FW + 255) / 256)), dim3(256), 0, st, mw, sp.x, kwords, sp.K, FW, b);
        hipLaunchKernelGGL(sim_sparse_msg_kernel, dim3((unsigned)((sp.M + 3) / 4) * tiles), dim3(256), 0, st, sp.x, P, sp.a_ptr, sp.a_col, sp.M, FW, tiles);
        hipLaunchKernelGGL(sim_sparse_solve_kernel, dim3(tiles), dim3(64), 0, st, P, sp.b_meta, sp.b_far, sp.M, FW);
        hipLaunchKernelGGL(sim_sparse_out_kernel, dim3((unsigned)(((size_t)pwords * FW + 255) / 256)), dim3(256), 0, st, P, parw + (size_t)f0 * pwords, pwords,
                           sp.M, FW, b);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "sim_sparse_parity: %s", hipGetErrorString(e));
    return LDPC_OK;
}

}  // namespace ldpc
