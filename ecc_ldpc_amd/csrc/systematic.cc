// systematic.cc -- a systematic form of ANY parity-check matrix (ldpc_csr_systematic_form, include/ldpc_hip.h): which columns
// carry the message, which the parity bits, and the K x rank matrix P that gives the parity bits from the message.
//
// The rule is greedy from the right: column c is a parity position iff it is not in the span of the parity positions > c.
// Written with the columns REVERSED (bit q of a row = column N - 1 - q) those are the pivot columns of the reduced row echelon
// form -- a column gets a pivot iff it is independent of the columns before it -- so one Gauss-Jordan elimination on rows packed
// into 64-bit words answers everything: the pivot row of parity position p reads  c[p] = XOR of c[n] over its other set
// columns n, all of them message positions.  Redundant and empty rows reduce to zero rows; a zero column never gets a pivot.
// Cost: rank * M bit tests and at most rank * M row XORs of N / 64 words.
#include "systematic.h"

#include <algorithm>
#include <new>

#include "../../include/ldpc_hip.h"

namespace ldpc {

static int fail(std::string &err, int code, const std::string &msg) {
    err = msg;
    return code;
}

int systematic_form(const char *who, int M, int N, const int32_t *row_ptr, const int32_t *col_idx, SystematicForm &out, std::string &err) {
    const std::string w(who);
    if (M <= 0 || N <= 0 || !row_ptr || !col_idx || row_ptr[0] != 0)
        return fail(err, LDPC_EINVAL, w + ": bad arguments (M=" + std::to_string(M) + " N=" + std::to_string(N) + ")");
    for (int m = 0; m < M; m++) {
        if (row_ptr[m + 1] < row_ptr[m]) return fail(err, LDPC_EINVAL, w + ": row_ptr decreases at row " + std::to_string(m));
        for (int q = row_ptr[m]; q < row_ptr[m + 1]; q++)
            if (col_idx[q] < 0 || col_idx[q] >= N || (q > row_ptr[m] && col_idx[q] <= col_idx[q - 1]))
                return fail(err, LDPC_EINVAL, w + ": row " + std::to_string(m) + ": columns not strictly ascending inside [0, " + std::to_string(N) + ")");
    }
    if ((long long)M * N > kSystematicMaxCells)
        return fail(err, LDPC_EUNSUPPORTED, w + ": M * N = " + std::to_string((long long)M * N) + " is above the elimination's limit of 2^28 = " +
                                                std::to_string(kSystematicMaxCells) + "; an accumulator-shaped H of this size encodes by back-substitution (ldpc_sim_create_sparse_on)");
    try {
        const size_t W = ((size_t)N + 63) / 64;
        std::vector<uint64_t> A((size_t)M * W, 0ull);
        for (int m = 0; m < M; m++)
            for (int e = row_ptr[m]; e < row_ptr[m + 1]; e++) {
                const int q = N - 1 - col_idx[e];
                A[(size_t)m * W + (q >> 6)] |= 1ull << (q & 63);
            }
        std::vector<int32_t> piv;   // reversed pivot columns, ascending; the pivot row of piv[t] is row t
        int rank = 0;
        for (int q = 0; q < N && rank < M; q++) {
            const size_t w0 = (size_t)q >> 6;
            const uint64_t bit = 1ull << (q & 63);
            int p = rank;
            while (p < M && !(A[(size_t)p * W + w0] & bit)) p++;
            if (p == M) continue;
            if (p != rank) std::swap_ranges(&A[(size_t)p * W + w0], &A[(size_t)p * W + W], &A[(size_t)rank * W + w0]);   // (rows >= rank are zero before word w0)
            const uint64_t *src = &A[(size_t)rank * W];
            for (int i = 0; i < M; i++) {
                uint64_t *dst = &A[(size_t)i * W];
                if (i == rank || !(dst[w0] & bit)) continue;
                for (size_t x = w0; x < W; x++) dst[x] ^= src[x];   // (the pivot row is zero in every column before its pivot)
            }
            piv.push_back(q);
            rank++;
        }
        const int K = N - rank;
        if (K <= 0) return fail(err, LDPC_EUNSUPPORTED, w + ": rank " + std::to_string(rank) + " = N: no message bits");
        out.K = K; out.rank = rank; out.pw64 = (rank + 63) / 64;
        out.par_pos.resize((size_t)rank);
        for (int j = 0; j < rank; j++) out.par_pos[j] = N - 1 - piv[rank - 1 - j];
        out.msg_pos.clear();
        for (int n = 0, j = 0; n < N; n++) {
            if (j < rank && out.par_pos[j] == n) j++;
            else out.msg_pos.push_back(n);
        }
        out.P.assign((size_t)K * out.pw64, 0ull);
        for (int j = 0; j < rank; j++) {
            const uint64_t *row = &A[(size_t)(rank - 1 - j) * W];
            for (int i = 0; i < K; i++) {
                const int q = N - 1 - out.msg_pos[i];
                if ((row[q >> 6] >> (q & 63)) & 1ull) out.P[(size_t)i * out.pw64 + (j >> 6)] |= 1ull << (j & 63);
            }
        }
    } catch (const std::bad_alloc &) { return fail(err, LDPC_ENOMEM, "out of host memory"); }
    return LDPC_OK;
}

}  // namespace ldpc
