// demap_product.hip -- ldpc_demap_dev for product constellations (demap.h AxisTab, b = 1..6 bits an axis, up to 4096-QAM): I/Q samples
// [batch][n_sym][2] -> LLRs [batch][N], one pass.  The rule and its device functions: demap_product.h; restated in
// tests/product_modulation_spec.py, which the kernel reproduces bit for bit.
// LANE = SLOT, as demap.hip: slot s of a frame is output elements m s .. m s + m - 1, m = 2 b: the b LLRs of the I coordinate, then the b
// of the Q coordinate.  A lane works its two axes one after the other, so 2^b distances are live at a time, and the two level tables ride
// in the kernel arguments (scalar loads).  A slot's m elements are contiguous: they go out in 16 / 8 / 4-byte vector stores where the row
// alignment allows it (demap_product.h store_slot_pieces).
// ONE SLOT A LANE, no grid-stride loop: inside a loop the compiler hoists the 128 level loads (and, in sim_mod_product.hip, the Philox key
// schedule) out of it as loop invariants and then spills those scalar registers; without one they are loaded where they are used.
// The kernel and its launcher are templated on the LLR rule and live in demap_product_kernel.h; this file holds the max-log instances
// (the ones it held before the rule existed) and the dispatch by rule; the log-MAP instances are demap_product_logmap.hip's.
#include "demap_product_kernel.h"

namespace ldpc {

int demap_product_launch(hipStream_t st, const AxisTab &tab, int b, int rule, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, int fmt, float qscale) {
    if (rule == DEMAP_LOGMAP) return demap_product_logmap_launch(st, tab, b, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale);
    return demap_product_launch_r<DEMAP_MAXLOG>(st, tab, b, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale);
}

}  // namespace ldpc
