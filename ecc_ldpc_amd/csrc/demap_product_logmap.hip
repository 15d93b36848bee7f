// demap_product_logmap.hip -- the log-MAP instances of ldpc_demap_dev's kernel for product constellations (demap_product_kernel.h,
// demap_product.h axis_llrs_logmap): a translation unit of their own, so that the max-log instances of demap_product.hip stay the set
// they were.  Two axes of b 2^b exponentials each a sample; no scratch and no spilled register (build.py checks it).
#include "demap_product_kernel.h"

namespace ldpc {

int demap_product_logmap_launch(hipStream_t st, const AxisTab &tab, int b, int batch, int n_tx, int N, const float *d_sym, float inv, void *d_llr, int fmt, float qscale) {
    return demap_product_launch_r<DEMAP_LOGMAP>(st, tab, b, batch, n_tx, N, d_sym, inv, d_llr, fmt, qscale);
}

}  // namespace ldpc
