// sim.h -- frame source / tally (sim.hip) interface
#pragma once
#include "internal.h"
namespace ldpc {
struct SimDev {
    int N, k, n_tx, kwords, pp;
    const uint32_t *gt;  // dense generator, [kwords][pp]: word w of column j of G (packed over message bits) at w*pp + j; pp = p
                         // rounded up to a multiple of 4 (16-byte rows); null = no dense table
    // quasi-cyclic generator (Fast/Encoder.hs:26-63): rotation table for sim_parity_qc_kernel, null = none.
    //   qc_rot[cg][r][b][16]: for column group cg (16/W block columns, W = sz/32 words per circulant), block row r and bit
    //   rotation b = 0..31, the W words of rotl(g[r][c], b) for each column c of the group (missing columns: zero)
    const uint32_t *qc_rot;
    int qc_w, qc_brows, qc_bcols, qc_ncg, pwords;   // pwords: packed parity words per frame (qc_bcols * qc_w; encoder from H: ceil(M / 32))
};
// encoder from H (sim_sparse.hip): the rows of H in the order of ldpc_csr_triangular_order, row j ending in column K + j
struct SimSparse {
    int M, K;
    const int32_t *a_ptr, *a_col;    // [M + 1], [..]: the message columns (< K) of row j
    const int32_t *b_meta, *b_far;   // [M + 1], [..]: bit 31 of b_meta[j] = the row holds parity bit j - 1; its low bits = where the row's
                                     // other earlier parity bits (as parity indices < j - 1) start in b_far
    uint32_t *x;                     // bit-sliced scratch [N][fw_cap]: word fw of position n = that bit of frames 32 fw .. 32 fw + 31
    int fw_cap;                      // frame words the scratch holds per position
};
int sim_sparse_parity(const SimSparse &sp, const uint32_t *msgw, int kwords, uint32_t *parw, int pwords, hipStream_t st, int batch);
// systematic form of any H (sim_systematic.hip): the codeword packed in H's column order, cww = ceil(N / 32) words per frame.
// Words 0..w0-1 hold message positions only and ARE the message words (every column before the first parity position is a message
// position, in order); words w0..cww-1 are the GF(2) product of the message with the window generator
//   gwin[cg][i][16]: for column group cg (16 codeword words from w0 + 16 cg) and message bit i < 32 kwords, those words of the
//   codeword of the unit message e_i (its own position and its parity bits; zero beyond the codeword and for i >= K)
struct SimSys {
    const uint32_t *gwin;
    int ncg, w0, cww;
    const int32_t *msg_pos;          // [K] ascending: where message bit i sits in the codeword
};
int sim_systematic_codeword(const SimSys &sy, const uint32_t *msgw, int kwords, uint32_t *cw, hipStream_t st, int batch);
int sim_systematic_msg_bytes(const uint32_t *msgw, int kwords, int K, uint8_t *d_msg, hipStream_t st, int batch);
int sim_systematic_tally(const SimSys &sy, int N, int K, int kwords, const uint32_t *msgw, hipStream_t st, int batch, const uint8_t *d_bits,
                         const int32_t *d_iters, unsigned long long *d_tally);
// parw: scratch for the packed parity words [batch][pwords] (quasi-cyclic encoder, encoder from H) or the packed codewords
// [batch][cww] (systematic form); null otherwise.  sp / sy: null unless the source encodes from H that way
// msgw_ready: the message words are already in msgw (sim_load_messages): no message is drawn, seed and first_frame key the noise only
int sim_generate(const SimDev &s, const SimSparse *sp, const SimSys *sy, uint32_t *msgw, uint32_t *parw, hipStream_t st, uint64_t seed, uint64_t first_frame, int batch,
                 double ebn0_db, void *d_out, int out_fmt, uint8_t *d_msg,    // out_fmt: 0 = f32 LLRs [batch][N], 1 = fp16 LLRs, 2 = codeword bytes [batch][n_tx],
                 bool msgw_ready = false);                                    // 3 = packed codewords [batch][ceil(n_tx / 8)] (sources with parw only)
// caller-supplied messages (include/ldpc_hip.h ldpc_bit_format; fmt 0: bytes [batch][k], 1: packed rows of kwords words) -> msgw, bits >= k zero
int sim_load_messages(hipStream_t st, const void *d_msg, int fmt, uint32_t *msgw, int kwords, int k, int batch);
// d_msg (same two formats) <- bits[frame][msg_pos[i]] of decoded bytes [batch][N]; msg_pos null = positions 0..k-1
int sim_extract_messages(hipStream_t st, const uint8_t *d_bits, int N, const int32_t *msg_pos, void *d_msg, int fmt, int kwords, int k, int batch);
int sim_tally(const SimDev &s, const uint32_t *msgw, hipStream_t st, int batch, const uint8_t *d_bits, const int32_t *d_iters,
              unsigned long long *d_tally);
// hard bits, one byte each [batch][N] -> packed [batch][ceil(N/8)], bit i of a frame in byte i / 8 at bit i % 8
int pack_bits(hipStream_t st, const uint8_t *d_bits, uint8_t *d_packed, int batch, int N);
}  // namespace ldpc
