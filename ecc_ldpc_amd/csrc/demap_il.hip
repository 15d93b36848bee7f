// demap_il.hip -- the max-log soft demapper writing through a bit interleaver (ldpc_demap_dev_il), and the table alone
// (ldpc_interleave_bits_dev, ldpc_deinterleave_llr_dev).  I/Q samples [batch][n_sym][2] -> LLRs [batch][N] in the decoders' input formats,
// one pass, no memset before it: every element of a row is written exactly once.  The LLR rule is the device functions of demap.h and
// demap_product.h, the ones demap_kernel and demap_product_kernel call, so with the identity table the output is ldpc_demap_dev's bit for
// bit; the table's rule and its device functions: interleaver.h; restated in tests/interleaver_spec.py.
// LANE = SYMBOL: lane s < n_sym of a frame reads the m table entries of its symbol (contiguous: vector loads where m allows) and stores
// its m LLRs at those codeword positions, element by element.  With a block table of m columns the lanes of a wave store consecutive
// elements for each bit index j, so the stores coalesce per j; a random table scatters them.  The lanes from n_sym on take the hole list
// (the punctured positions, sorted), m holes a lane, and store zeros.
// ONE ITEM A LANE, no grid-stride loop, for the reason demap_product.hip gives.
// The LLR rule (demap.h DEMAP_MAXLOG / DEMAP_LOGMAP) is a template argument of the two demapper kernels.
#include "demap_product.h"
#include "interleaver.h"
#include "mod_dispatch.h"

namespace ldpc {

template <int M, typename OT, int RULE>
__global__ __launch_bounds__(256) void demap_il_kernel(ModTab tab, IlTab il, const float *__restrict__ sym, OT *__restrict__ llr, int n_sym, int lanes, size_t total,
                                                       float inv, float qs) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)lanes;
        const int s = (int)(i - f * (size_t)lanes);
        OT *row = llr + f * (size_t)il.N;
        if (s < n_sym) {
            const float2 y = *reinterpret_cast<const float2 *>(sym + 2 * (f * (size_t)n_sym + s));
            float v[M];
            int32_t p[M];
            demap_llrs_by<M, RULE>(tab, y.x, y.y, inv, v);
            il_positions<M>(il.pos + (size_t)M * s, p);
            il_store<M, OT>(row, p, il.n_tx - M * s, v, qs);
        } else {
            il_store_holes<M, OT>(row, il, M * (s - n_sym), qs);
        }
    }
}

template <int B, typename OT, int RULE>
__global__ __launch_bounds__(256) void demap_il_product_kernel(AxisTab tab, IlTab il, const float *__restrict__ sym, OT *__restrict__ llr, int n_sym, int lanes,
                                                               size_t total, float inv, float qs) {
    constexpr int M = 2 * B;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const size_t f = i / (size_t)lanes;
        const int s = (int)(i - f * (size_t)lanes);
        OT *row = llr + f * (size_t)il.N;
        if (s < n_sym) {
            const float2 y = *reinterpret_cast<const float2 *>(sym + 2 * (f * (size_t)n_sym + s));
            float v[M];
            int32_t p[M];
            // the axes one after the other, in a loop of two turns that is NOT unrolled (sim_mod_product.hip): 2^B distances and 2^B
            // levels live at a time, where the scheduler otherwise interleaves the two axes and doubles the registers
#pragma unroll 1
            for (int a = 0; a < 2; a++) {
                float r[B];
                axis_llrs_by<B, RULE>(tab.lev[a], a ? y.y : y.x, inv, r);
#pragma unroll
                for (int j = 0; j < B; j++) {
                    if (a) v[B + j] = r[j]; else v[j] = r[j];
                }
            }
            il_positions<M>(il.pos + (size_t)M * s, p);
            il_store<M, OT>(row, p, il.n_tx - M * s, v, qs);
        } else {
            il_store_holes<M, OT>(row, il, M * (s - n_sym), qs);
        }
    }
}

int demap_il_launch(hipStream_t st, const ModTab &tab, int m, int rule, const IlTab &il, int batch, const float *d_sym, float inv, void *d_llr, int fmt, float qscale) {
    const char *what = "ldpc_demap_dev_il";
    return launched(what, dispatch_rule_bits_fmt(what, rule, m, fmt, [&](auto r, auto k, auto t) {
        constexpr int M = decltype(k)::value, RULE = decltype(r)::value;
        typedef typename decltype(t)::type OT;
        const int n_sym = mod_symbols(il.n_tx, M), lanes = mod_lanes(n_sym, il.n_holes, M);
        const size_t total = (size_t)batch * lanes;
        const int rc = check_items(what, total);
        if (rc == LDPC_OK) hipLaunchKernelGGL((demap_il_kernel<M, OT, RULE>), grid_lanes(total), dim3(256), 0, st, tab, il, d_sym, (OT *)d_llr, n_sym, lanes, total, inv, qscale);
        return rc;
    }));
}

int demap_il_product_launch(hipStream_t st, const AxisTab &tab, int b, int rule, const IlTab &il, int batch, const float *d_sym, float inv, void *d_llr, int fmt, float qscale) {
    const char *what = "ldpc_demap_dev_il";
    return launched(what, dispatch_rule_bits_fmt(what, rule, b, fmt, [&](auto r, auto k, auto t) {
        constexpr int B = decltype(k)::value, M = 2 * B, RULE = decltype(r)::value;
        typedef typename decltype(t)::type OT;
        const int n_sym = mod_symbols(il.n_tx, M), lanes = mod_lanes(n_sym, il.n_holes, M);
        const size_t total = (size_t)batch * lanes;
        const int rc = check_items(what, total);
        if (rc == LDPC_OK) hipLaunchKernelGGL((demap_il_product_kernel<B, OT, RULE>), grid_lanes(total), dim3(256), 0, st, tab, il, d_sym, (OT *)d_llr, n_sym, lanes, total, inv, qscale);
        return rc;
    }));
}

// ---- the table alone
// bit p of a codeword row: bit 0 of byte p, or bit p % 8 of byte p / 8
template <bool PACKED>
__device__ __forceinline__ uint32_t il_bit(const uint8_t *__restrict__ row, int p) {
    return PACKED ? ((uint32_t)row[p >> 3] >> (p & 7)) & 1u : (uint32_t)row[p] & 1u;
}

// LANE = OUTPUT BYTE: one transmitted bit (bytes out), or eight of them (packed out; the pad bits of a row's last byte are 0)
template <bool INP, bool OUTP>
__global__ __launch_bounds__(256) void interleave_bits_kernel(IlTab il, const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int in_row, int out_row, size_t total) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t f = i / (size_t)out_row;
        const int e = (int)(i - f * (size_t)out_row);
        const uint8_t *row = in + f * (size_t)in_row;
        if constexpr (!OUTP) {
            out[i] = (uint8_t)il_bit<INP>(row, il.pos[e]);
        } else {
            uint32_t byte = 0u;
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (8 * e + j < il.n_tx) byte |= il_bit<INP>(row, il.pos[8 * e + j]) << j;
            out[i] = (uint8_t)byte;
        }
    }
}

// LANE = OUTPUT ELEMENT in list order: lane r < n_tx of a frame moves transmitted element r to position pos[r], lane n_tx + h writes 0
// (all bits clear: +0 in float32 and fp16, 0 in int8) at hole h.  The reads are consecutive, the writes follow the table
template <typename T>
__global__ __launch_bounds__(256) void deinterleave_kernel(IlTab il, const T *__restrict__ in, T *__restrict__ out, size_t total) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t f = i / (size_t)il.N;
        const int r = (int)(i - f * (size_t)il.N);
        T *row = out + f * (size_t)il.N;
        if (r < il.n_tx) row[il.pos[r]] = in[f * (size_t)il.n_tx + r];
        else row[il.holes[r - il.n_tx]] = (T)0;
    }
}

int interleave_bits_launch(hipStream_t st, const IlTab &il, int batch, const uint8_t *d_in, bool in_packed, uint8_t *d_out, bool out_packed) {
    const int in_row = in_packed ? (il.N + 7) / 8 : il.N, out_row = out_packed ? (il.n_tx + 7) / 8 : il.n_tx;
    const size_t total = (size_t)batch * out_row;
    const dim3 grid = grid_stride(total);
    if (in_packed && out_packed) hipLaunchKernelGGL((interleave_bits_kernel<true, true>), grid, dim3(256), 0, st, il, d_in, d_out, in_row, out_row, total);
    else if (in_packed) hipLaunchKernelGGL((interleave_bits_kernel<true, false>), grid, dim3(256), 0, st, il, d_in, d_out, in_row, out_row, total);
    else if (out_packed) hipLaunchKernelGGL((interleave_bits_kernel<false, true>), grid, dim3(256), 0, st, il, d_in, d_out, in_row, out_row, total);
    else hipLaunchKernelGGL((interleave_bits_kernel<false, false>), grid, dim3(256), 0, st, il, d_in, d_out, in_row, out_row, total);
    return launched("ldpc_interleave_bits_dev");
}

int deinterleave_llr_launch(hipStream_t st, const IlTab &il, int batch, const void *d_in, void *d_out, int elem) {
    const size_t total = (size_t)batch * il.N;
    const dim3 grid = grid_stride(total);
    if (elem == 4) hipLaunchKernelGGL((deinterleave_kernel<uint32_t>), grid, dim3(256), 0, st, il, (const uint32_t *)d_in, (uint32_t *)d_out, total);
    else if (elem == 2) hipLaunchKernelGGL((deinterleave_kernel<uint16_t>), grid, dim3(256), 0, st, il, (const uint16_t *)d_in, (uint16_t *)d_out, total);
    else hipLaunchKernelGGL((deinterleave_kernel<uint8_t>), grid, dim3(256), 0, st, il, (const uint8_t *)d_in, (uint8_t *)d_out, total);
    return launched("ldpc_deinterleave_llr_dev");
}

}  // namespace ldpc
