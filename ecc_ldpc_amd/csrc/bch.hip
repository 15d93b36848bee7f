// bch.hip -- BCH encode and bounded-distance decode on the device (ldpc_bch_encode_dev, ldpc_bch_decode_dev, ldpc_sim_bch_decode).
// The rule and its linear form: bch.h; restated in tests/bch_spec.py.
//
// The shape is crc.hip's: a wave owns a frame (four frames a 256-thread workgroup, the frame folded into blockIdx.x), its lanes stride
// over the frame's bits, and lane i XORs entry T[i] of every set bit i it sees.  An entry is W <= 8 words here, not one: the table is
// kept as W PLANES of n words, so that a wave instruction still reads 64 (256 with VEC) consecutive words of one plane, and the W
// partial words are reduced across the wave by __shfl_xor.  The instances are compiled for W = 1, 2, 4, 6, 8 (a table of fewer words is
// padded with zero planes), which keeps the accumulator in registers.
//   ENCODE  R over the k message bits is the parity: the first p lanes-strided bytes, or (packed) the words from bit k on, each put
//           together from 64 lanes' bits by a __ballot.
//   DECODE  R over all n bits; R == 0 is a wave-uniform branch that ends a clean frame with nerr = 0 -- after LDPC decoding almost every
//           frame, so this path sets the cost and nothing below is in it.  Otherwise, all inside the wave, with no LDS and no atomic:
//           1. S_j = R(alpha^j), j = 1 .. 2t, lane j - 1 its own: the XOR of alog[j b mod N0] over the <= p set bits b of R (independent loads);
//           2. Berlekamp-Massey in its inversionless form, lane c = coefficient c of Lambda and of B: the discrepancy is a wave XOR, the
//              shift by x^s a __shfl, and the products are shift-and-add in registers (m steps): a table product would put three
//              dependent loads into each of the 2t serial steps;
//           3. Chien search, lanes striding over the positions: Lambda at alpha^-d through the doubled antilog table and log Lambda_j
//              (read across the wave with a uniform lane index).  Roots are COUNTED first -- a __ballot per 64 positions, the q-th root
//              kept in lane q -- and only a count equal to L (with L <= t and deg Lambda = L) lets lanes < L flip their bits: a frame
//              that fails is never written.  Positions >= n are not searched: a root there leaves the count short.
//           Bytes: row[q] ^= 1.  Packed: decoded rows need not be word-aligned, so lanes that share a BYTE combine their masks across
//           the wave and one of them rewrites the byte.
#include <hip/hip_runtime.h>

#include "bch.h"

namespace ldpc {

static __device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v ^= __shfl_xor(v, o, 64);
    return v;
}

static __device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// R[0 .. W - 1], in every lane: the XOR of T[i] over the set bits i < limit of frame row `row`
template <int W, bool PACKED, bool VEC>
static __device__ __forceinline__ void bch_frame_xor(const BchTab &t, const uint8_t *__restrict__ row, const int32_t *__restrict__ pos, int limit, int lane, uint32_t (&R)[W]) {
#pragma unroll
    for (int w = 0; w < W; w++) R[w] = 0u;
    if constexpr (VEC) {
        for (int i = 4 * lane; i < limit; i += 256) {
            const uint32_t v = *reinterpret_cast<const uint32_t *>(row + i);          // bytes i .. i + 3 (the row holds them: its stride is a multiple of 4)
            const uint32_t m0 = 0u - (v & 1u), m1 = 0u - ((v >> 8) & (uint32_t)(i + 1 < limit)), m2 = 0u - ((v >> 16) & (uint32_t)(i + 2 < limit)),
                           m3 = 0u - ((v >> 24) & (uint32_t)(i + 3 < limit));
#pragma unroll
            for (int w = 0; w < W; w++) {
                const uint4 e = *reinterpret_cast<const uint4 *>(t.T + (size_t)w * t.n4 + i);   // a plane is padded to a multiple of 4 entries
                R[w] ^= (m0 & e.x) ^ (m1 & e.y) ^ (m2 & e.z) ^ (m3 & e.w);
            }
        }
    } else {
        for (int i = lane; i < limit; i += 64) {
            const int q = pos ? pos[i] : i;
            const uint32_t b = PACKED ? ((uint32_t)row[q >> 3] >> (q & 7)) & 1u : row[q] & 1u;
#pragma unroll
            for (int w = 0; w < W; w++) R[w] ^= (0u - b) & t.T[(size_t)w * t.n4 + i];
        }
    }
#pragma unroll
    for (int w = 0; w < W; w++) R[w] = wave_xor(R[w]);
}

// bit b of R, b in 0 .. 32 W - 1 (a chain of selects: R stays in registers)
template <int W>
static __device__ __forceinline__ uint32_t rem_bit(const uint32_t (&R)[W], int b) {
    uint32_t v = R[0];
#pragma unroll
    for (int w = 1; w < W; w++) v = (b >> 5) == w ? R[w] : v;
    return (v >> (b & 31)) & 1u;
}

// in place: reads row bits 0 .. k - 1, writes bits k .. n - 1 (packed: the words from bit k on, message bits kept, pad bits 0)
template <int W, bool PACKED, bool VEC>
__global__ __launch_bounds__(256) void bch_encode_kernel(BchTab t, uint8_t *rows, size_t stride, int batch) {
    const int lane = threadIdx.x & 63;
    const size_t f = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= (size_t)batch) return;
    uint8_t *row = rows + f * stride;
    uint32_t R[W];
    bch_frame_xor<W, PACKED, VEC>(t, row, nullptr, t.k, lane, R);
    if constexpr (PACKED) {
        // row bit k + j = bit p - 1 - j of R.  64 lanes' bits make two words at a time, from the word that holds bit k on
        uint32_t *words = reinterpret_cast<uint32_t *>(row);
        const int w0 = t.k >> 5, nwords = (t.n + 31) >> 5;
        const uint32_t keep = words[w0];
        for (int base = 32 * w0; base < 32 * nwords; base += 64) {
            const int i = base + lane;
            const uint32_t bit = i < t.k ? (keep >> (i & 31)) & 1u : i < t.n ? rem_bit<W>(R, t.p - 1 - (i - t.k)) : 0u;
            const unsigned long long mask = __ballot(bit != 0u);
            const int wi = (base >> 5) + lane;
            if (lane < 2 && wi < nwords) words[wi] = lane ? (uint32_t)(mask >> 32) : (uint32_t)mask;
        }
    } else {
        for (int j = lane; j < t.p; j += 64) row[t.k + j] = (uint8_t)rem_bit<W>(R, t.p - 1 - j);
    }
}

// a b in GF(2^m), shift and add
static __device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b, int m, uint32_t prim) {
    uint32_t r = 0u;
    for (int i = 0; i < m; i++) {
        r ^= (0u - ((b >> i) & 1u)) & a;
        a <<= 1;
        a ^= (0u - (a >> m)) & prim;
    }
    return r;
}

// the frame's remainder R != 0 -> the number of bits corrected in `row`, or -1 with the row untouched; the same value in every lane
template <int W, bool PACKED>
static __device__ __forceinline__ int bch_correct(const BchTab &t, const uint32_t (&R)[W], uint8_t *row, const int32_t *__restrict__ pos, int lane) {
    const int t2 = 2 * t.t, N0 = t.N0, m = t.m;
    const uint32_t prim = t.prim_poly;
    // 1. lane j - 1: S_j = R(alpha^j)
    uint32_t S = 0u;
#pragma unroll
    for (int w = 0; w < W; w++) {
        uint32_t word = uniform(R[w]);
        while (word) {
            const uint32_t b = (uint32_t)(__ffs((int)word) - 1 + 32 * w);
            word &= word - 1u;
            S ^= t.alog[((uint32_t)(lane + 1) * b) % (uint32_t)N0];
        }
    }
    if (lane >= t2) S = 0u;
    // 2. inversionless Berlekamp-Massey; lane c: coefficient c of Lambda (lam) and of B
    uint32_t lam = lane == 0, B = lane == 0, gamma = 1u;
    int L = 0, s = 1;
    for (int r = 0; r < t2; r++) {
        const int src = r - lane;
        uint32_t sv = __shfl(S, src & 63, 64);
        sv = src >= 0 ? sv : 0u;
        const uint32_t d = uniform(wave_xor(gf_mul(lam, sv, m, prim)));
        if (d) {
            uint32_t Bs = __shfl(B, (lane - s) & 63, 64);
            Bs = lane >= s ? Bs : 0u;
            const uint32_t next = gf_mul(lam, gamma, m, prim) ^ gf_mul(Bs, d, m, prim);
            if (2 * L <= r) {
                B = lam;
                L = r + 1 - L;
                gamma = d;
                s = 1;
            } else {
                s++;
            }
            lam = next;
        } else {
            s++;
        }
    }
    if (L > t.t) return -1;
    if (uniform(__shfl(lam, L, 64)) == 0u) return -1;                                 // deg Lambda < L
    // 3. Chien: count the roots first
    const uint32_t kZero = 0xffffffffu;
    const uint32_t ll = lam ? (uint32_t)t.log[lam] : kZero;                            // lam < 2^m: inside the table
    const uint32_t lam0 = uniform(lam);
    int count = 0, root = 0;
    for (int base = 0; base < t.n; base += 64) {
        const int d = base + lane;
        const bool valid = d < t.n;
        const uint32_t e = valid && d ? (uint32_t)(N0 - d) : 0u;                       // alpha^-d = alpha^(N0 - d)
        uint32_t acc = lam0, ej = 0u;
        for (int j = 1; j <= L; j++) {
            ej += e;
            ej -= ej >= (uint32_t)N0 ? (uint32_t)N0 : 0u;
            const uint32_t lj = (uint32_t)__builtin_amdgcn_readlane((int)ll, j);
            if (lj != kZero) acc ^= t.alog[lj + ej];                                  // lj, ej < N0: inside the doubled table
        }
        unsigned long long mask = __ballot(valid && acc == 0u);
        while (mask) {
            const int q = __ffsll((long long)mask) - 1;
            mask &= mask - 1ull;
            if (lane == count) root = base + q;
            count++;
        }
    }
    if (count != L) return -1;
    // lanes < L flip the bit of x^root: row bit n - 1 - root
    const bool mine = lane < L;
    const int i = mine ? t.n - 1 - root : 0;
    const int q = pos ? pos[i] : i;
    if constexpr (PACKED) {
        const int byte = mine ? q >> 3 : -1;
        uint32_t bits = 0u;
        bool first = true;
        for (int o = 0; o < L; o++) {
            const int ob = __shfl(byte, o, 64);
            const uint32_t om = 1u << (__shfl(q, o, 64) & 7);
            if (ob == byte) {
                bits ^= om;
                if (o < lane) first = false;
            }
        }
        if (mine && first) row[byte] ^= (uint8_t)bits;
    } else {
        if (mine) row[q] ^= 1u;
    }
    return L;
}

template <int W, bool PACKED, bool VEC>
__global__ __launch_bounds__(256) void bch_decode_kernel(BchTab t, uint8_t *rows, size_t stride, const int32_t *__restrict__ pos, int32_t *__restrict__ nerr, int batch) {
    const int lane = threadIdx.x & 63;
    const size_t f = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= (size_t)batch) return;
    uint8_t *row = rows + f * stride;
    uint32_t R[W];
    bch_frame_xor<W, PACKED, VEC>(t, row, pos, t.n, lane, R);
    uint32_t any = 0u;
#pragma unroll
    for (int w = 0; w < W; w++) any |= R[w];
    if (uniform(any) == 0u) {                                                         // a codeword: the frame is done
        if (lane == 0) nerr[f] = 0;
        return;
    }
    const int e = bch_correct<W, PACKED>(t, R, row, pos, lane);
    if (lane == 0) nerr[f] = e;
}

static int bch_launched(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "%s: %s", what, hipGetErrorString(e));
    return LDPC_OK;
}

template <int W>
static void bch_encode_w(hipStream_t st, const BchTab &t, int batch, uint8_t *rows, bool packed) {
    const dim3 grid(((unsigned)batch + 3u) / 4u), block(256);
    if (packed) hipLaunchKernelGGL((bch_encode_kernel<W, true, false>), grid, block, 0, st, t, rows, (size_t)4 * ((t.n + 31) / 32), batch);
    else if (t.n % 4 == 0 && (uintptr_t)rows % 4 == 0) hipLaunchKernelGGL((bch_encode_kernel<W, false, true>), grid, block, 0, st, t, rows, (size_t)t.n, batch);
    else hipLaunchKernelGGL((bch_encode_kernel<W, false, false>), grid, block, 0, st, t, rows, (size_t)t.n, batch);
}

template <int W>
static void bch_decode_w(hipStream_t st, const BchTab &t, int batch, uint8_t *rows, size_t stride, bool packed, const int32_t *pos, int32_t *d_nerr) {
    const dim3 grid(((unsigned)batch + 3u) / 4u), block(256);
    if (packed) hipLaunchKernelGGL((bch_decode_kernel<W, true, false>), grid, block, 0, st, t, rows, stride, pos, d_nerr, batch);
    else if (!pos && stride % 4 == 0 && (uintptr_t)rows % 4 == 0) hipLaunchKernelGGL((bch_decode_kernel<W, false, true>), grid, block, 0, st, t, rows, stride, pos, d_nerr, batch);
    else hipLaunchKernelGGL((bch_decode_kernel<W, false, false>), grid, block, 0, st, t, rows, stride, pos, d_nerr, batch);
}

int bch_encode_launch(hipStream_t st, const BchTab &t, int W, int batch, void *d_rows, bool packed) {
    uint8_t *rows = (uint8_t *)d_rows;
    switch (W) {
        case 1: bch_encode_w<1>(st, t, batch, rows, packed); break;
        case 2: bch_encode_w<2>(st, t, batch, rows, packed); break;
        case 4: bch_encode_w<4>(st, t, batch, rows, packed); break;
        case 6: bch_encode_w<6>(st, t, batch, rows, packed); break;
        case 8: bch_encode_w<8>(st, t, batch, rows, packed); break;
        default: return set_error(LDPC_EUNSUPPORTED, "ldpc_bch_encode_dev: no instance for %d table words", W);
    }
    return bch_launched("ldpc_bch_encode_dev");
}

int bch_decode_launch(hipStream_t st, const BchTab &t, int W, int batch, uint8_t *rows, size_t stride, bool packed, const int32_t *pos, int32_t *d_nerr) {
    switch (W) {
        case 1: bch_decode_w<1>(st, t, batch, rows, stride, packed, pos, d_nerr); break;
        case 2: bch_decode_w<2>(st, t, batch, rows, stride, packed, pos, d_nerr); break;
        case 4: bch_decode_w<4>(st, t, batch, rows, stride, packed, pos, d_nerr); break;
        case 6: bch_decode_w<6>(st, t, batch, rows, stride, packed, pos, d_nerr); break;
        case 8: bch_decode_w<8>(st, t, batch, rows, stride, packed, pos, d_nerr); break;
        default: return set_error(LDPC_EUNSUPPORTED, "bch_decode: no instance for %d table words", W);
    }
    return bch_launched("bch_decode");
}

}  // namespace ldpc
