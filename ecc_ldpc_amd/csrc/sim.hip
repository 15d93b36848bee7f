// sim.hip -- device-side frame source and error tally for the BER/throughput harness.
//
// The reference delegates this to the external tester (ecc-manifold's eccMain, main/Main.hs:41-48:
// message generation, encode, BPSK + AWGN, BER statistics; its source is not vendored, SURVEY.md
// section 8c), so the channel model is this build's own stated one:
//   message bits uniform; systematic encode  codeword = msg ++ take (c_length - k) (msg * G)
//   (src/ECC/Code/LDPC/Utils.hs:61, Reference/Orig.hs:25-26, Fast/Encoder.hs:26-63) -- G dense (sim_frame_kernel), quasi-cyclic
//   (sim_parity_qc_kernel), or none at all: all-zero codewords, or, for an H whose parity part is triangular after a row
//   permutation, the same codeword by back-substitution FROM H (sim_sparse.hip; no counterpart in the reference).  The last two
//   hand sim_frame_kernel packed parity words parw[frame][pwords].  ANY other H: a systematic form by GF(2) elimination, whose
//   message and parity positions may interleave (sim_systematic.hip) -- it hands over whole packed codewords, read with k = 0;
//   BPSK bit b -> 2b-1 (LLR > 0 <=> bit 1, `hard x = x > 0`); noise N(0, sigma^2),
//   sigma^2 = 1/(2 R 10^(EbN0/10)), R = k/n_tx; LLR = 2y/sigma^2; punctured tail LLR = 0
//   (Utils.hs:55 `unpuncture`).
// Randomness: Philox4x32-10 keyed by the 64-bit seed, counter = (global frame id, index / 4, stream),
// so a frame's content depends only on (seed, frame id): ranks generate disjoint frame ranges
// with no scatter.  Philox and the Box-Muller step live in sim_noise.h, shared with the modulated path (sim_mod.hip: any
// constellation of 2..64 points, complex AWGN on stream 2, max-log LLRs).
// The message words may also come from the caller (sim_load_messages: bytes or packed bits -> msgw; sim_generate then skips the draw and
// Philox keys the noise alone), and the codewords may leave packed (sim_pack_codeword_kernel); sim_extract_messages is the way back.
#include "internal.h"
#include "sim.h"
#include "sim_noise.h"
#include <hip/hip_fp16.h>
#include <algorithm>

namespace ldpc {

// message words: msgw[frame][w], bit i of word w = message bit 32*w + i
__global__ void sim_msg_kernel(uint32_t *msgw, int kwords, int k, uint64_t seed, uint64_t first_frame, int batch, int zero_msg) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)batch * kwords) return;
    int f = (int)(i / kwords), w = (int)(i % kwords);
    uint32_t r[4];
    Philox::gen(seed, first_frame + f, (uint32_t)w, 0u, r);
    uint32_t v = zero_msg ? 0u : r[0];
    int rem = k - 32 * w;
    if (rem < 32) v &= (rem <= 0) ? 0u : ((1u << rem) - 1u);
    msgw[i] = v;
}

// Quasi-cyclic encoder, the reference's formulation (Fast/Encoder.hs:42-63): the message is cut into sz-bit words v'[r],
// the parity word of block column c is  XOR_r mulWord(v'[r], g[r][c]),  mulWord(w1, w2) = XOR over the set bits n of w1 of
// rotateL(w2, n).  Here: LANE = FRAME, a wave = 64 frames x one group of 16/W block columns (W = sz/32 machine words per
// circulant).  The generator is never expanded: for n = 32a + b, word w of rotateL(g, n) is word (w - a) mod W of
// rotateL(g, b), so a table of the 32 bit-rotations of every circulant (scalar loads: 16 words per (r, b), the same for
// all lanes) is all that is read -- 32 x 12 x 32 x 4 words = 196 KB for jpl.4096 instead of the 786 KB dense k x p matrix,
// and it grows with k + p, not k * p.  Per message bit and parity word: one v_bitop3 (acc ^= mask & T), the mask (0 / -1
// from bit b of the lane's message word) shared by the 16/W columns of the group.
// The four waves of a workgroup share the 64 frames and the column group and split the block rows; their partial parity
// words meet in LDS (XOR is associative: any split gives the same bits).  4x the waves of a one-wave version: the scalar
// table loads of one wave hide behind the XORs of the others (jpl.4096, 65 536 frames: 0.91 -> see profiles/r03_encoder_rate.txt).
constexpr int kQcRowSplit = 4;
template <int W>
__global__ __launch_bounds__(64 * kQcRowSplit) void sim_parity_qc_kernel(const uint32_t *__restrict__ rot, int brows, int bcols, const uint32_t *__restrict__ msgw,
                                                                         uint32_t *__restrict__ parw, int kwords, int pwords, int batch) {
    constexpr int CB = 16 / W;
    __shared__ uint32_t part[kQcRowSplit - 1][16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.x * 64 + lane;
    const int cg = blockIdx.y;
    const bool live = f < batch;
    const int rchunk = (brows + kQcRowSplit - 1) / kQcRowSplit;
    const int r_begin = __builtin_amdgcn_readfirstlane(wave * rchunk), r_end = min(brows, r_begin + rchunk);
    const uint32_t *mw = msgw + (size_t)(live ? f : 0) * kwords;
    const uint32_t *t = rot + (size_t)cg * brows * (32 * 16);
    uint32_t acc[CB][W];
#pragma unroll
    for (int c = 0; c < CB; c++)
#pragma unroll
        for (int w = 0; w < W; w++) acc[c][w] = 0u;
    for (int r = r_begin; r < r_end; r++) {
        uint32_t v[W];
#pragma unroll
        for (int a = 0; a < W; a++) v[a] = mw[r * W + a];
#pragma unroll
        for (int b0 = 0; b0 < 32; b0 += 4) {
            uint32_t T[4][16];       // four rotations' worth of table in flight (64 SGPRs): one wait per 4 x W masked regions
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int i = 0; i < 16; i++) T[q][i] = t[(r * 32 + b0 + q) * 16 + i];   // uniform address: scalar loads
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int a = 0; a < W; a++)
                    if ((v[a] >> (b0 + q)) & 1u) {   // the lanes (frames) whose message bit 32a + b of this block row is set: EXEC mask, one v_xor per word
                        asm volatile("" ::: "memory");   // keeps this a real EXEC-masked region (otherwise: v_cndmask + v_xor per word)
#pragma unroll
                        for (int c = 0; c < CB; c++)
#pragma unroll
                            for (int w = 0; w < W; w++) acc[c][w] ^= T[q][c * W + ((w - a) & (W - 1))];
                    }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int c = 0; c < CB; c++)
#pragma unroll
            for (int w = 0; w < W; w++) part[wave - 1][c * W + w][lane] = acc[c][w];
    }
    __syncthreads();
    if (wave > 0 || !live) return;
#pragma unroll
    for (int c = 0; c < CB; c++)
#pragma unroll
        for (int w = 0; w < W; w++)
#pragma unroll
            for (int q = 0; q < kQcRowSplit - 1; q++) acc[c][w] ^= part[q][c * W + w][lane];
#pragma unroll
    for (int c = 0; c < CB; c++) {
        const int bc = cg * CB + c;
        if (bc < bcols) {
#pragma unroll
            for (int w = 0; w < W; w++) parw[(size_t)f * pwords + bc * W + w] = acc[c][w];
        }
    }
}

// one thread per (frame, group of four consecutive positions n = 4g .. 4g+3): ONE Philox call feeds both
// Box-Muller pairs (r0,r1 -> cos and sin branch, r2,r3 likewise), i.e. four normals -- the generator is bound by
// Philox's quarter-rate 32x32 multiplies, and the first version spent a whole call per sample.
// OT = float / __half: LLRs [batch][N]; OT = uint8_t: the codeword itself, bytes [batch][n_tx], no channel (the encoder alone)
template <typename OT, bool VEC>
__global__ __launch_bounds__(256) void sim_frame_kernel(SimDev s, const uint32_t *__restrict__ msgw, const uint32_t *__restrict__ parw, OT *__restrict__ llr,
                                                        uint8_t *__restrict__ msg_bytes, uint64_t seed, uint64_t first_frame,
                                                        int batch, float sigma, float llr_scale) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int f = blockIdx.y;
    const int n0 = 4 * g;
    if (n0 >= s.N || f >= batch) return;
    const uint32_t *mw = msgw + (size_t)f * s.kwords;
    constexpr bool kBytes = sizeof(OT) == 1;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (!kBytes && n0 < s.n_tx) {
        uint32_t r[4];
        Philox::gen(seed, first_frame + f, (uint32_t)g, 1u, r);
        box_muller4(r, z);   // (sim_noise.h)
    }
    // parity bits of the group: bit j = <msg, column j of G> over GF(2); a group that lies inside the parity part
    // on a 4-aligned column reads its four columns with one 16-byte load per message word
    uint32_t pacc[4] = {0u, 0u, 0u, 0u};
    if (s.gt && !parw && n0 + 3 >= s.k && n0 < s.n_tx) {
        const int j0 = n0 - s.k;
        if (j0 >= 0 && (j0 & 3) == 0) {
            const uint4 *col = reinterpret_cast<const uint4 *>(s.gt + j0);
            const size_t stride = (size_t)s.pp / 4;
            for (int w = 0; w < s.kwords; w++) {
                const uint32_t m = mw[w];
                const uint4 c = col[(size_t)w * stride];
                pacc[0] ^= m & c.x; pacc[1] ^= m & c.y; pacc[2] ^= m & c.z; pacc[3] ^= m & c.w;
            }
        } else {
            for (int w = 0; w < s.kwords; w++) {
                const uint32_t m = mw[w];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int j = j0 + i;
                    if (j >= 0 && j < s.pp) pacc[i] ^= m & s.gt[(size_t)w * s.pp + j];
                }
            }
        }
    }
    float out[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int n = n0 + i;
        out[i] = 0.f;
        if (n < s.n_tx) {
            uint32_t bit;
            if (n < s.k) {
                bit = (mw[n >> 5] >> (n & 31)) & 1u;
                if (msg_bytes) msg_bytes[(size_t)f * s.k + n] = (uint8_t)bit;
            } else if (parw) {
                const int j = n - s.k;         // packed by sim_parity_qc_kernel or sim_sparse_parity
                bit = (parw[(size_t)f * s.pwords + (j >> 5)] >> (j & 31)) & 1u;
            } else {
                bit = __popc(pacc[i]) & 1u;   // (no generator: pacc = 0, the all-zero codeword)
            }
            out[i] = llr_scale * ((bit ? 1.0f : -1.0f) + sigma * z[i]);
        } else if (n < s.k && msg_bytes) {
            msg_bytes[(size_t)f * s.k + n] = (uint8_t)((mw[n >> 5] >> (n & 31)) & 1u);
        }
    }
    if constexpr (kBytes) {
#pragma unroll
        for (int i = 0; i < 4; i++) if (n0 + i < s.n_tx) llr[(size_t)f * s.n_tx + n0 + i] = out[i] > 0.f ? 1 : 0;   // (sigma = 0: out = +-scale)
        return;
    }
    OT *dst = llr + (size_t)f * s.N + n0;
    if constexpr (kBytes) {
    } else if constexpr (sizeof(OT) == 2) {
        __half h[4];
#pragma unroll
        for (int i = 0; i < 4; i++) h[i] = __float2half_rn(fminf(fmaxf(out[i], -65504.f), 65504.f));  // = round_f16
        if constexpr (VEC) {
            *reinterpret_cast<uint2 *>(dst) = *reinterpret_cast<const uint2 *>(h);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) if (n0 + i < s.N) dst[i] = h[i];
        }
    } else {
        if constexpr (VEC) {
            *reinterpret_cast<float4 *>(dst) = make_float4(out[0], out[1], out[2], out[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) if (n0 + i < s.N) dst[i] = out[i];
        }
    }
}

// tally[0..3] += {frames, frame errors, message-bit errors, sum of iterations}; one wave per frame
__global__ __launch_bounds__(256) void sim_tally_kernel(SimDev s, const uint32_t *__restrict__ msgw, const uint8_t *__restrict__ bits,
                                                        const int32_t *__restrict__ iters, unsigned long long *tally, int batch) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= batch) return;
    unsigned errs = 0;
    for (int n = lane; n < s.k; n += 64) {
        unsigned m = (msgw[(size_t)f * s.kwords + (n >> 5)] >> (n & 31)) & 1u;
        errs += (bits[(size_t)f * s.N + n] != m);
    }
    for (int o = 32; o > 0; o >>= 1) errs += __shfl_down(errs, o, 64);
    if (lane == 0) {
        atomicAdd(&tally[0], 1ull);
        if (errs) atomicAdd(&tally[1], 1ull);
        if (errs) atomicAdd(&tally[2], (unsigned long long)errs);
        if (iters) atomicAdd(&tally[3], (unsigned long long)iters[f]);
    }
}

// frames per launch of the kernels whose frame is blockIdx.y (sim_frame_kernel, pack_bits_kernel): the 65 536 the device reports as its
// largest gridDim.y (hipDeviceAttributeMaxGridDimY; the runtime has been seen to run more, which nothing promises), so that a batch
// up to there is one launch as before; even, so that a slice starts on the alignment the first one has
constexpr int kFrameSlice = 65536;

// ---- caller-supplied messages (ldpc_sim_encode_messages, ldpc_sim_generate_from, ldpc_sim_extract_messages).  The three kernels
// index (frame, word) through one flat grid-stride loop over blockIdx.x: no batch limit of their own.
static unsigned sim_grid(size_t total) { return (unsigned)std::min<size_t>((total + 255) / 256, (size_t)1 << 20); }
// bit 0 of the four bytes of a word, LSB first
static __device__ __forceinline__ uint32_t bits4(uint32_t w) { return (w & 1u) | ((w >> 7) & 2u) | ((w >> 14) & 4u) | ((w >> 21) & 8u); }
static __device__ __forceinline__ uint32_t bits16(uint4 a) { return bits4(a.x) | (bits4(a.y) << 4) | (bits4(a.z) << 8) | (bits4(a.w) << 12); }

// message bytes [batch][k] (bit 0 of each) -> msgw[frame][w]: a lane makes one whole word from 32 consecutive bytes.  VEC: k % 16 == 0 and
// a 16-byte aligned buffer, so every word starts on a 16-byte boundary and holds 16 or 32 bits: one or two 16-byte loads
template <bool VEC>
__global__ __launch_bounds__(256) void sim_load_bytes_kernel(const uint8_t *__restrict__ src, uint32_t *__restrict__ msgw, int kwords, int k, size_t total) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t f = i / kwords;
        const int w = (int)(i - f * kwords);
        const uint8_t *row = src + f * k + 32 * w;
        const int rem = min(32, k - 32 * w);   // bits of this word, >= 1; the others stay 0
        uint32_t v = 0u;
        if constexpr (VEC) {
            v = bits16(*reinterpret_cast<const uint4 *>(row));
            if (rem == 32) v |= bits16(*reinterpret_cast<const uint4 *>(row + 16)) << 16;
        } else {
            for (int b = 0; b < rem; b++) v |= (uint32_t)(row[b] & 1u) << b;
        }
        msgw[i] = v;
    }
}

// packed message rows of kwords little-endian words ARE the message words, but for the bits >= k of the last one
__global__ __launch_bounds__(256) void sim_load_packed_kernel(const uint32_t *__restrict__ src, uint32_t *__restrict__ msgw, int kwords, int k, size_t total) {
    const uint32_t tail = (k & 31) ? ((1u << (k & 31)) - 1u) : 0xffffffffu;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        msgw[i] = src[i] & ((int)(i % kwords) == kwords - 1 ? tail : 0xffffffffu);
}

// packed codewords [batch][PB = ceil(n_tx / 8)] bytes: one lane = output word j of a frame, codeword bits 32 j .. 32 j + 31 =
// message bits below k, parity bits (parw, from bit 0) above: a message word, a parity word pair funnel-shifted by k % 32, or,
// for the one word that straddles k, both.  Cut at n_tx, pad bits 0.  k = 0: parw holds whole codewords.  words_ok: PB % 4 == 0 and a
// 4-byte aligned buffer, word stores; otherwise the bytes of the word one by one (rows need not start on a word then)
__global__ __launch_bounds__(256) void sim_pack_codeword_kernel(const uint32_t *__restrict__ msgw, const uint32_t *__restrict__ parw, uint8_t *__restrict__ out, int k,
                                                                int n_tx, int kwords, int pwords, int cwords, int PB, int words_ok, size_t total) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t f = i / cwords;
        const int j = (int)(i - f * cwords), n0 = 32 * j;
        uint32_t v;
        if (n0 + 32 <= k) {
            v = msgw[f * kwords + j];
        } else {
            const uint32_t *pw = parw + f * pwords;
            if (n0 >= k) {                       // (n0 < n_tx <= k + 32 pwords: q < pwords)
                const int q = (n0 - k) >> 5, sh = (n0 - k) & 31;
                const uint32_t lo = pw[q], hi = (sh && q + 1 < pwords) ? pw[q + 1] : 0u;
                v = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
            } else {
                const int r = k - n0;            // 1 .. 31 message bits, then parity bits from bit 0
                v = (msgw[f * kwords + j] & ((1u << r) - 1u)) | (pw[0] << r);
            }
        }
        const int rem = n_tx - n0;               // >= 1
        if (rem < 32) v &= (1u << rem) - 1u;
        if (words_ok) {
            reinterpret_cast<uint32_t *>(out)[i] = v;
        } else {
            uint8_t *dst = out + f * PB + 4 * j;
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (4 * j + b < PB) dst[b] = (uint8_t)(v >> (8 * b));
        }
    }
}

// decoded bytes [batch][N] -> the message in msg_pos order: PACKED = words of 32 bits (rows of kwords words, bits >= k zero), else bytes [batch][k]
template <bool PACKED>
__global__ __launch_bounds__(256) void sim_extract_kernel(const uint8_t *__restrict__ bits, int N, const int32_t *__restrict__ msg_pos, void *__restrict__ out, int kwords,
                                                          int k, size_t total) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        if constexpr (PACKED) {
            const size_t f = i / kwords;
            const int w = (int)(i - f * kwords), rem = min(32, k - 32 * w);
            const uint8_t *row = bits + f * N;
            uint32_t v = 0u;
            for (int b = 0; b < rem; b++) v |= (uint32_t)(row[msg_pos ? msg_pos[32 * w + b] : 32 * w + b] & 1u) << b;
            static_cast<uint32_t *>(out)[i] = v;
        } else {
            const size_t f = i / k;
            const int m = (int)(i - f * k);
            static_cast<uint8_t *>(out)[i] = bits[f * N + (msg_pos ? msg_pos[m] : m)] & 1u;
        }
    }
}

int sim_load_messages(hipStream_t st, const void *d_msg, int fmt, uint32_t *msgw, int kwords, int k, int batch) {
    const size_t total = (size_t)batch * kwords;
    const dim3 grid(sim_grid(total));
    if (fmt == 1) hipLaunchKernelGGL(sim_load_packed_kernel, grid, dim3(256), 0, st, (const uint32_t *)d_msg, msgw, kwords, k, total);
    else if (k % 16 == 0 && (uintptr_t)d_msg % 16 == 0) hipLaunchKernelGGL((sim_load_bytes_kernel<true>), grid, dim3(256), 0, st, (const uint8_t *)d_msg, msgw, kwords, k, total);
    else hipLaunchKernelGGL((sim_load_bytes_kernel<false>), grid, dim3(256), 0, st, (const uint8_t *)d_msg, msgw, kwords, k, total);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "sim_load_messages: %s", hipGetErrorString(e));
    return LDPC_OK;
}

int sim_extract_messages(hipStream_t st, const uint8_t *d_bits, int N, const int32_t *msg_pos, void *d_msg, int fmt, int kwords, int k, int batch) {
    if (fmt == 1) {
        const size_t total = (size_t)batch * kwords;
        hipLaunchKernelGGL((sim_extract_kernel<true>), dim3(sim_grid(total)), dim3(256), 0, st, d_bits, N, msg_pos, d_msg, kwords, k, total);
    } else {
        const size_t total = (size_t)batch * k;
        hipLaunchKernelGGL((sim_extract_kernel<false>), dim3(sim_grid(total)), dim3(256), 0, st, d_bits, N, msg_pos, d_msg, kwords, k, total);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "sim_extract_messages: %s", hipGetErrorString(e));
    return LDPC_OK;
}

int sim_generate(const SimDev &s0, const SimSparse *sp, const SimSys *sy, uint32_t *msgw, uint32_t *parw, hipStream_t st, uint64_t seed, uint64_t first_frame,
                 int batch, double ebn0_db, void *d_out, int out_fmt, uint8_t *d_msg0, bool msgw_ready) {
    // systematic form of any H: parw holds whole codewords in H's column order, so the frame kernel runs with k = 0 -- every position
    // takes its parw branch -- and the message bytes come from sim_systematic_msg_bytes
    SimDev s = s0;
    uint8_t *d_msg = d_msg0;
    if (sy) { s.k = 0; s.pwords = sy->cww; d_msg = nullptr; }
    const double R = (double)s0.k / (double)s0.n_tx;
    const double sigma2 = 1.0 / (2.0 * R * pow(10.0, ebn0_db / 10.0));
    size_t nw = (size_t)batch * s.kwords;
    if (!msgw_ready)
        hipLaunchKernelGGL(sim_msg_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, msgw, s.kwords, s0.k, seed, first_frame, batch, (s.gt || parw) ? 0 : 1);
    if (sy) {
        int rc = sim_systematic_codeword(*sy, msgw, s.kwords, parw, st, batch);
        if (rc == LDPC_OK && d_msg0) rc = sim_systematic_msg_bytes(msgw, s.kwords, s0.k, d_msg0, st, batch);
        if (rc != LDPC_OK) return rc;
    } else if (sp) {
        const int rc = sim_sparse_parity(*sp, msgw, s.kwords, parw, s.pwords, st, batch);
        if (rc != LDPC_OK) return rc;
    } else if (s.qc_rot) {
        const dim3 pg((batch + 63) / 64, s.qc_ncg);
#define LDPC_QC_PARITY(W_) hipLaunchKernelGGL((sim_parity_qc_kernel<W_>), pg, dim3(64 * kQcRowSplit), 0, st, s.qc_rot, s.qc_brows, s.qc_bcols, msgw, parw, s.kwords, s.pwords, batch)
        switch (s.qc_w) {
            case 1: LDPC_QC_PARITY(1); break;
            case 2: LDPC_QC_PARITY(2); break;
            case 4: LDPC_QC_PARITY(4); break;
            case 8: LDPC_QC_PARITY(8); break;
            default: return set_error(LDPC_EUNSUPPORTED, "quasi-cyclic encoder: circulant size %d", 32 * s.qc_w);
        }
#undef LDPC_QC_PARITY
    }
    if (out_fmt == 3) {   // packed codewords straight from the packed message and parity words (k = 0, systematic form: from the codeword words)
        if (!parw) return set_error(LDPC_EUNSUPPORTED, "sim_generate: packed codewords need packed parity words");
        const int cwords = (s.n_tx + 31) / 32, PB = (s.n_tx + 7) / 8;
        const size_t total = (size_t)batch * cwords;
        const int words_ok = (PB % 4 == 0) && ((uintptr_t)d_out % 4 == 0);
        hipLaunchKernelGGL(sim_pack_codeword_kernel, dim3(sim_grid(total)), dim3(256), 0, st, msgw, parw, (uint8_t *)d_out, s.k, s.n_tx, s.kwords, s.pwords, cwords, PB,
                           words_ok, total);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return set_error(LDPC_EHIP, "sim_generate: %s", hipGetErrorString(e));
        return LDPC_OK;
    }
    const int groups = ((out_fmt == 2 ? s.n_tx : s.N) + 3) / 4;
    const float sg = (float)sqrt(sigma2), sc = (float)(2.0 / sigma2);
    // 16-byte (f32) / 8-byte (fp16) vector stores when every row starts aligned: decided once, from the caller's pointer (an even
    // slice keeps every slice start aligned whenever the first one is)
    const bool vec = (s.N % 4 == 0) && ((uintptr_t)d_out % 16 == 0);
    // the frame is blockIdx.y (kFrameSlice): a larger batch goes in slices, all on the caller's stream.  The Philox counters are
    // functions of (frame id, group), so the slices write what one launch would
    const size_t row = out_fmt == 2 ? (size_t)s.n_tx : (size_t)s.N * (out_fmt == 1 ? 2 : 4);   // bytes of an output row
    for (int f0 = 0; f0 < batch; f0 += kFrameSlice) {
        const int b = std::min(kFrameSlice, batch - f0);
        const dim3 grid((groups + 255) / 256, b);
        const uint32_t *mw = msgw + (size_t)f0 * s.kwords;
        const uint32_t *pw = parw ? parw + (size_t)f0 * s.pwords : nullptr;
        uint8_t *dm = d_msg ? d_msg + (size_t)f0 * s.k : nullptr;
        void *out = (uint8_t *)d_out + (size_t)f0 * row;
        const uint64_t first = first_frame + (uint64_t)f0;
        if (out_fmt == 2) {
            hipLaunchKernelGGL((sim_frame_kernel<uint8_t, false>), grid, dim3(256), 0, st, s, mw, pw, (uint8_t *)out, dm, seed, first, b, 0.f, 1.f);
        } else if (out_fmt == 1) {
            if (vec) hipLaunchKernelGGL((sim_frame_kernel<__half, true>), grid, dim3(256), 0, st, s, mw, pw, (__half *)out, dm, seed, first, b, sg, sc);
            else hipLaunchKernelGGL((sim_frame_kernel<__half, false>), grid, dim3(256), 0, st, s, mw, pw, (__half *)out, dm, seed, first, b, sg, sc);
        } else {
            if (vec) hipLaunchKernelGGL((sim_frame_kernel<float, true>), grid, dim3(256), 0, st, s, mw, pw, (float *)out, dm, seed, first, b, sg, sc);
            else hipLaunchKernelGGL((sim_frame_kernel<float, false>), grid, dim3(256), 0, st, s, mw, pw, (float *)out, dm, seed, first, b, sg, sc);
        }
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "sim_generate: %s", hipGetErrorString(e));
    return LDPC_OK;
}

int sim_tally(const SimDev &s, const uint32_t *msgw, hipStream_t st, int batch, const uint8_t *d_bits, const int32_t *d_iters,
              unsigned long long *d_tally) {
    hipLaunchKernelGGL(sim_tally_kernel, dim3((batch + 3) / 4), dim3(256), 0, st, s, msgw, d_bits, d_iters, d_tally, batch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "sim_tally: %s", hipGetErrorString(e));
    return LDPC_OK;
}

// ---- packed result bits (ldpc_decode_batch_dev_packed): eight result bytes -> one byte, LSB first
__global__ __launch_bounds__(256) void pack_bits_kernel(const uint8_t *__restrict__ bits, uint8_t *__restrict__ packed, int batch, int N, int PB) {
    const int f = blockIdx.y;
    const uint8_t *src = bits + (size_t)f * N;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < PB; j += gridDim.x * blockDim.x) {
        uint32_t b = 0;
        if ((N & 7) == 0) {                                   // every frame starts on an 8-byte boundary of a 16-byte aligned buffer
            const uint2 v = *reinterpret_cast<const uint2 *>(src + 8 * (size_t)j);
            auto nib = [](uint32_t w) { return (w & 1u) | ((w >> 7) & 2u) | ((w >> 14) & 4u) | ((w >> 21) & 8u); };
            b = nib(v.x) | (nib(v.y) << 4);
        } else {
#pragma unroll
            for (int t = 0; t < 8; t++)
                if (8 * j + t < N) b |= (uint32_t)(src[8 * (size_t)j + t] & 1u) << t;
        }
        packed[(size_t)f * PB + j] = (uint8_t)b;
    }
}

int pack_bits(hipStream_t st, const uint8_t *d_bits, uint8_t *d_packed, int batch, int N) {
    const int PB = (N + 7) / 8;
    for (int f0 = 0; f0 < batch; f0 += kFrameSlice) {   // the frame is blockIdx.y: slices, as in sim_generate
        const int b = std::min(kFrameSlice, batch - f0);
        hipLaunchKernelGGL(pack_bits_kernel, dim3((PB + 255) / 256, b), dim3(256), 0, st, d_bits + (size_t)f0 * N, d_packed + (size_t)f0 * PB, b, N, PB);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "pack_bits: %s", hipGetErrorString(e));
    return LDPC_OK;
}

}  // namespace ldpc
