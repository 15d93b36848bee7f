// demap_apriori.hip -- the soft demapper WITH A-PRIORI INPUT, writing through a bit interleaver (ldpc_demap_dev_il_apriori): demap_csi.hip's
// table kernel with bit knowledge, for the receiver that iterates between demapper and decoder (BICM-ID).  d_apriori [batch][N] float32 in
// CODEWORD order holds what the decoder said about every bit (its extrinsic output: ldpc_decode_batch_dev_soft), LLR = log P(1) / P(0).
// The rule is restated in tests/demap_apriori_spec.py; all float32, one operation at a time, nothing fused:
//   d_p    the squared distances of demap.h demap_llrs; inv_s = fl(inv a) of fading.h (no gains: inv)
//   a_p    the sum of La_j over the set label bits j of p, MSB first, left to right: a_0 = +0, a_p = a_q + La_j with j the least significant
//          set bit of p and q = p without it; one set bit: La_j itself
//   u_p    fl(a_p - fl(d_p inv_s));  U1_j / U0_j = max of u_p over the labels whose bit j is 1 / 0
//   max-log   LLR_j = fl(fl(U1_j - U0_j) - La_j): the EXTRINSIC value -- the bit's own knowledge is taken out again
//   log-MAP   fl(logmap_llr(fl(U1_j - U0_j), s0, s1) - La_j), s_v = the sum over the subset, in label order, of exp(u_p - U_v): the
//             convention of demap.h logmap_llr, a zero correction leaves the max-log term as it is
// LANE = SYMBOL, as demap_csi.hip: the lane gathers its m a-priori values through the same m table entries it stores through, so a
// punctured position's a-priori value is never read; the pad bits of a ragged last symbol have La = 0.  Every element of d_llr is written
// exactly once (0 at the holes, by the lanes after the symbols), no memset.
// The constellation is read from LDS (demap_apriori_kernel).  Cost: 2^m points a symbol, each one add (a_p: the sums of a label's prefix are shared, the compiler sees p as a constant), one
// multiply, one subtract and m max.  Log-MAP is the two-pass form of demap_llrs_logmap: the u_p are computed again for the exponentials
// -- the same float32 operations, hence the same values -- where keeping 2^m of them would hold 64 registers across the second pass.
// Product objects are refused by the entry point (api.cc): their Gray-like per-axis labels gain little from iteration.
#include "demap_product.h"
#include "fading.h"
#include "mod_dispatch.h"

namespace ldpc {

// a_p for a label p that is a constant after unrolling
template <int M>
__device__ __forceinline__ float apriori_sum(int p, const float (&la)[M]) {
    float acc = 0.f;
    bool any = false;
#pragma unroll
    for (int j = 0; j < M; j++) {
        if ((p >> (M - 1 - j)) & 1) {
            acc = any ? acc + la[j] : la[j];
            any = true;
        }
    }
    return acc;
}

// u_p.  pts: the constellation in LDS (demap_apriori_kernel says why)
template <int M>
__device__ __forceinline__ float apriori_metric(const float2 *pts, int p, float yI, float yQ, float inv_s, const float (&la)[M]) {
    const float2 c = pts[p];
    const float dx = yI - c.x, dy = yQ - c.y;
    const float d = dx * dx + dy * dy;
    return apriori_sum<M>(p, la) - d * inv_s;
}

template <int M, int RULE>
__device__ __forceinline__ void demap_llrs_apriori(const float2 *pts, float yI, float yQ, float inv_s, const float (&la)[M], float (&llr)[M]) {
    float u0[M], u1[M];
#pragma unroll
    for (int p = 0; p < (1 << M); p++) {
        const float u = apriori_metric<M>(pts, p, yI, yQ, inv_s, la);
#pragma unroll
        for (int j = 0; j < M; j++) {
            const int bit = (p >> (M - 1 - j)) & 1;
            if (bit) u1[j] = (p == (1 << (M - 1 - j))) ? u : __builtin_fmaxf(u1[j], u);
            else u0[j] = (p == 0) ? u : __builtin_fmaxf(u0[j], u);
        }
    }
    if constexpr (RULE == DEMAP_LOGMAP && M > 1) {
        float s0[M], s1[M];
#pragma unroll
        for (int p = 0; p < (1 << M); p++) {
            const float u = apriori_metric<M>(pts, p, yI, yQ, inv_s, la);
#pragma unroll
            for (int j = 0; j < M; j++) {
                const int bit = (p >> (M - 1 - j)) & 1;
                const float e = __expf(bit ? u - u1[j] : u - u0[j]);
                if (bit) s1[j] = (p == (1 << (M - 1 - j))) ? e : s1[j] + e;
                else s0[j] = (p == 0) ? e : s0[j] + e;
            }
        }
#pragma unroll
        for (int j = 0; j < M; j++) llr[j] = logmap_llr(u1[j] - u0[j], s0[j], s1[j]) - la[j];
    } else {                                              // (m = 1: one point a subset, both sums are exp(0))
#pragma unroll
        for (int j = 0; j < M; j++) llr[j] = (u1[j] - u0[j]) - la[j];
    }
}

// THE TABLE IN LDS.  The other demappers read the constellation from the kernel arguments through scalar loads.  Here a point's
// metric also holds a sum of per-lane values, the walk keeps more alive, and the scheduler issued the scalar loads of all 2^m points ahead of
// it: 128 coordinates at m = 6, more than the scalar registers hold -- they spilled, in the max-log instance too, and chunking the walk
// behind values hidden from the optimiser (demap_rm.hip) moved the spills without ending them.  So the workgroup copies the 2^m points
// into LDS once (512 bytes at the most) and every lane reads point p at the same address: a broadcast, 8 bytes into two vector registers
// that live for one point.  No scalar register holds a coordinate.
template <int M, typename OT, int RULE>
__global__ __launch_bounds__(256) void demap_apriori_kernel(ModTab tab, IlTab il, const float *__restrict__ sym, const float *__restrict__ gain,
                                                            const float *__restrict__ apriori, OT *__restrict__ llr, int n_sym, int lanes, size_t total, float inv, float qs) {
    __shared__ float2 pts[1 << M];
    if (threadIdx.x < (1 << M)) pts[threadIdx.x] = make_float2(tab.pt[threadIdx.x][0], tab.pt[threadIdx.x][1]);
    __syncthreads();      // (every thread of the workgroup: the guard comes after it)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)lanes;
        const int s = (int)(i - f * (size_t)lanes);
        OT *row = llr + f * (size_t)il.N;
        if (s < n_sym) {
            const size_t at = f * (size_t)n_sym + s;
            const float2 y = *reinterpret_cast<const float2 *>(sym + 2 * at);
            const float inv_s = gain ? fade_inv(inv, gain[at]) : inv;
            const float *la_row = apriori + f * (size_t)il.N;
            const int rem = il.n_tx - M * s;
            float v[M], la[M];
            int32_t p[M];
            il_positions<M>(il.pos + (size_t)M * s, p);
#pragma unroll
            for (int j = 0; j < M; j++) la[j] = j < rem ? la_row[p[j]] : 0.f;      // (a pad bit's table entry is 0: not read as a position)
            demap_llrs_apriori<M, RULE>(pts, y.x, y.y, inv_s, la, v);
            il_store<M, OT>(row, p, rem, v, qs);
        } else {
            il_store_holes<M, OT>(row, il, M * (s - n_sym), qs);
        }
    }
}

int demap_apriori_launch(hipStream_t st, const ModTab &tab, int m, int rule, const IlTab &il, int batch, const float *d_sym, const float *d_gain, const float *d_apriori,
                         float inv, void *d_llr, int fmt, float qscale) {
    const char *what = "ldpc_demap_dev_il_apriori";
    return launched(what, dispatch_rule_bits_fmt(what, rule, m, fmt, [&](auto r, auto k, auto t) {
        constexpr int M = decltype(k)::value, RULE = decltype(r)::value;
        typedef typename decltype(t)::type OT;
        const int n_sym = mod_symbols(il.n_tx, M), lanes = mod_lanes(n_sym, il.n_holes, M);
        const size_t total = (size_t)batch * lanes;
        const int rc = check_items(what, total);
        if (rc == LDPC_OK)
            hipLaunchKernelGGL((demap_apriori_kernel<M, OT, RULE>), grid_lanes(total), dim3(256), 0, st, tab, il, d_sym, d_gain, d_apriori, (OT *)d_llr, n_sym, lanes, total, inv,
                               qscale);
        return rc;
    }));
}

}  // namespace ldpc
