// systematic.h -- a systematic form of any parity-check matrix by GF(2) elimination (systematic.cc).  Plain C++: no HIP header,
// so that a stand-alone host program can build it (and run it under a sanitizer) without the rest of the library.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

namespace ldpc {

// the largest M * N the elimination takes (include/ldpc_hip.h, ldpc_csr_systematic_form)
constexpr long long kSystematicMaxCells = 1ll << 28;

// The rule of ldpc_csr_systematic_form: columns visited from N - 1 down to 0, a column is a parity position iff it is not in the
// span of the parity positions chosen before it.  msg_pos [K] and par_pos [rank] ascend.  P packed by rows:
//   bit j of row i (word i * pw64 + j / 64, bit j % 64) = P[i][j]:   c[par_pos[j]] = XOR_i m[i] P[i][j]
struct SystematicForm {
    int K = 0, rank = 0, pw64 = 0;
    std::vector<int32_t> msg_pos, par_pos;
    std::vector<uint64_t> P;
};

// -> LDPC_OK, or LDPC_EINVAL (malformed CSR) / LDPC_EUNSUPPORTED (M * N above the limit, no message bits) / LDPC_ENOMEM with the
// reason in err; `who` starts that message
int systematic_form(const char *who, int M, int N, const int32_t *row_ptr, const int32_t *col_idx, SystematicForm &out, std::string &err);

}  // namespace ldpc
