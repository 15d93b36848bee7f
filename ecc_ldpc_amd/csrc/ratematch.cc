// ratematch.cc -- the host side of the rate-matching table (include/ldpc_hip.h ldpc_ratematch): the checks of a position table whose
// entries may repeat, its inverse in CSR form, and the circular-buffer rule.  Nothing here touches a device (ldpc_ratematch_create_on,
// which copies the table there, is in api.cc).  Restated in tests/ratematch_spec.py.
#include <new>

#include "ratematch.h"

using ldpc::set_error;

namespace ldpc {

int ratematch_check(const char *what, int E, int N, const int32_t *pos) {
    if (!pos) return set_error(LDPC_EINVAL, "%s: null table", what);
    if (N < 1) return set_error(LDPC_EINVAL, "%s: N = %d (must be >= 1)", what, N);
    if (E < 1 || E > kRmMaxE) return set_error(LDPC_EINVAL, "%s: E = %d outside 1..%d", what, E, kRmMaxE);
    for (int t = 0; t < E; t++)
        if (pos[t] < 0 || pos[t] >= N) return set_error(LDPC_EINVAL, "%s: pos[%d] = %d outside 0..%d", what, t, pos[t], N - 1);
    return LDPC_OK;
}

// a counting sort by position: the t are placed in increasing order, so every position's list is ascending
int ratematch_invert(int E, int N, const int32_t *pos, std::vector<int32_t> &inv_ptr, std::vector<int32_t> &inv_t) {
    std::vector<int32_t> at;
    try { inv_ptr.assign((size_t)N + 1, 0); inv_t.assign((size_t)E, 0); at.resize((size_t)N); } catch (const std::bad_alloc &) { return set_error(LDPC_ENOMEM, "out of host memory"); }
    for (int t = 0; t < E; t++) inv_ptr[(size_t)pos[t] + 1]++;
    for (int c = 0; c < N; c++) inv_ptr[(size_t)c + 1] += inv_ptr[c];
    for (int c = 0; c < N; c++) at[c] = inv_ptr[c];
    for (int t = 0; t < E; t++) inv_t[(size_t)at[pos[t]]++] = t;
    return LDPC_OK;
}

}  // namespace ldpc

extern "C" {

int ldpc_ratematch_circular_positions(int n_buf, const int32_t *buf, int start, int E, int32_t *pos) {
    if (n_buf < 1 || E < 1) return set_error(LDPC_EINVAL, "ldpc_ratematch_circular_positions: n_buf = %d, E = %d: both must be >= 1", n_buf, E);
    if (start < 0 || start >= n_buf) return set_error(LDPC_EINVAL, "ldpc_ratematch_circular_positions: start = %d outside 0..%d", start, n_buf - 1);
    if (!pos) return set_error(LDPC_EINVAL, "ldpc_ratematch_circular_positions: null output");
    int at = start;                                        // (start + t) mod n_buf, without the sum that could pass an int
    for (int t = 0; t < E; t++) {
        pos[t] = buf ? buf[at] : at;
        if (++at == n_buf) at = 0;
    }
    return LDPC_OK;
}

int ldpc_ratematch_dims(const ldpc_ratematch *rm, int *E, int *N) {
    if (!rm) return set_error(LDPC_EINVAL, "null ratematch");
    if (E) *E = rm->E;
    if (N) *N = rm->N;
    return LDPC_OK;
}

int ldpc_ratematch_positions(const ldpc_ratematch *rm, int32_t *pos) {
    if (!rm) return set_error(LDPC_EINVAL, "null ratematch");
    for (int t = 0; pos && t < rm->E; t++) pos[t] = rm->pos[t];
    return rm->E;
}

int ldpc_ratematch_fanin(const ldpc_ratematch *rm, int32_t *count) {
    if (!rm || !count) return set_error(LDPC_EINVAL, "ldpc_ratematch_fanin: null argument");
    for (int c = 0; c < rm->N; c++) count[c] = rm->inv_ptr[(size_t)c + 1] - rm->inv_ptr[c];
    return LDPC_OK;
}

}  // extern "C"
