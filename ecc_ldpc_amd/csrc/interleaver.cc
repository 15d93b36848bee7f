// interleaver.cc -- the host side of the bit interleaver (include/ldpc_hip.h ldpc_interleaver): the checks of a position table, its hole
// list, and the block rule.  Nothing here touches a device (ldpc_interleaver_create_on, which copies the table there, is in api.cc).
// Restated in tests/interleaver_spec.py.
#include <limits.h>

#include <new>

#include "interleaver.h"

using ldpc::set_error;

namespace ldpc {

int interleaver_check(const char *what, int n_tx, int N, const int32_t *pos, std::vector<int32_t> &holes) {
    if (!pos) return set_error(LDPC_EINVAL, "%s: null table", what);
    if (n_tx < 1 || n_tx > N) return set_error(LDPC_EINVAL, "%s: n_tx = %d outside 1..N = %d", what, n_tx, N);
    std::vector<uint8_t> seen;
    try { seen.assign((size_t)N, 0); holes.clear(); holes.reserve((size_t)(N - n_tx)); } catch (const std::bad_alloc &) { return set_error(LDPC_ENOMEM, "out of host memory"); }
    for (int t = 0; t < n_tx; t++) {
        const int32_t p = pos[t];
        if (p < 0 || p >= N) return set_error(LDPC_EINVAL, "%s: pos[%d] = %d outside 0..%d", what, t, p, N - 1);
        if (seen[p]) return set_error(LDPC_EINVAL, "%s: pos[%d] = %d repeats an earlier entry", what, t, p);
        seen[p] = 1;
    }
    for (int n = 0; n < N; n++)
        if (!seen[n]) holes.push_back(n);
    return LDPC_OK;
}

}  // namespace ldpc

extern "C" {

int ldpc_interleaver_block_positions(int rows, int cols, const int32_t *twist, const int32_t *order, int32_t *pos) {
    if (rows < 1 || cols < 1 || (long long)rows * (long long)cols > (long long)INT_MAX)
        return set_error(LDPC_EINVAL, "ldpc_interleaver_block_positions: rows = %d, cols = %d: both must be >= 1 and rows * cols must fit an int", rows, cols);
    if (!pos) return set_error(LDPC_EINVAL, "ldpc_interleaver_block_positions: null output");
    if (twist)
        for (int c = 0; c < cols; c++)
            if (twist[c] < 0 || twist[c] >= rows) return set_error(LDPC_EINVAL, "ldpc_interleaver_block_positions: twist[%d] = %d outside 0..%d", c, twist[c], rows - 1);
    if (order) {
        std::vector<uint8_t> seen;
        try { seen.assign((size_t)cols, 0); } catch (const std::bad_alloc &) { return set_error(LDPC_ENOMEM, "out of host memory"); }
        for (int j = 0; j < cols; j++) {
            if (order[j] < 0 || order[j] >= cols || seen[order[j]])
                return set_error(LDPC_EINVAL, "ldpc_interleaver_block_positions: order is not a permutation of 0..%d (order[%d] = %d)", cols - 1, j, order[j]);
            seen[order[j]] = 1;
        }
    }
    // codeword bit c rows + u sits in column c at row (u + twist[c]) mod rows; the matrix is read row by row, the columns in `order`
    for (int r = 0; r < rows; r++)
        for (int j = 0; j < cols; j++) {
            const int c = order ? order[j] : j, tw = twist ? twist[c] : 0;
            int u = r - tw;
            if (u < 0) u += rows;
            pos[(size_t)r * cols + j] = c * rows + u;
        }
    return LDPC_OK;
}

int ldpc_interleaver_dims(const ldpc_interleaver *il, int *n_tx, int *N) {
    if (!il) return set_error(LDPC_EINVAL, "null interleaver");
    if (n_tx) *n_tx = il->n_tx;
    if (N) *N = il->N;
    return LDPC_OK;
}

int ldpc_interleaver_positions(const ldpc_interleaver *il, int32_t *pos) {
    if (!il) return set_error(LDPC_EINVAL, "null interleaver");
    for (int t = 0; pos && t < il->n_tx; t++) pos[t] = il->pos[t];
    return il->n_tx;
}

}  // extern "C"
