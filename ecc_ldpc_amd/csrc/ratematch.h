// ratematch.h -- the rate-matching table of include/ldpc_hip.h (ldpc_ratematch): a position table between codeword order and transmitted
// order whose entries MAY REPEAT.  Transmitted bit t is codeword bit pos[t], t = 0 .. E - 1, pos any map into 0 .. N - 1, E below, at or
// above N; the codeword positions no pos[t] names are not sent in this round.  The receive side adds the LLRs of all transmitted bits
// that name a position, and optionally the soft buffer of earlier rounds (HARQ), in ONE defined order: the object holds the INVERSE of
// the table in CSR form, inv_t[inv_ptr[c] .. inv_ptr[c + 1]) = the t with pos[t] = c, ascending, and the kernels of demap_rm.hip GATHER
// through it, one lane per codeword element.  The injective table stays the interleaver (interleaver.h), whose scatter kernels are
// untouched.  The host side (validation, the inversion, the circular rule): ratematch.cc.  The transmit side reads pos alone, through
// the interleaver's kernels (rm_as_il).  The rule is restated in tests/ratematch_spec.py.
#pragma once
#include "interleaver.h"

namespace ldpc {

// the table as a kernel argument (device pointers)
struct RmTab {
    const int32_t *pos;       // [E + kIlPad], the pad 0 as the interleaver's
    const int32_t *inv_ptr;   // [N + 1], inv_ptr[0] = 0, inv_ptr[N] = E
    const int32_t *inv_t;     // [E]: the transmitted indices by codeword position, ascending inside a position
    int E, N;
};

// E + kIlPad table entries are indexed with an int, so E may be no larger than this; the launchers, which work ONE item a lane, further
// refuse batch * max(E, N) above kLaneMaxItems
constexpr int kRmMaxE = 0x7fffffff - kIlPad;

// pos [E] maps into 0 .. N - 1, 1 <= E <= kRmMaxE, N >= 1: LDPC_OK, or LDPC_EINVAL
int ratematch_check(const char *what, int E, int N, const int32_t *pos);
// the inverse of a checked table in CSR form (a counting sort, so every list is ascending): LDPC_OK, or LDPC_ENOMEM
int ratematch_invert(int E, int N, const int32_t *pos, std::vector<int32_t> &inv_ptr, std::vector<int32_t> &inv_t);

// what the kernels that read pos alone need (sim_mod_il.hip, sim_mod_fading.hip, demap_il.hip interleave_bits_kernel): the table as an
// interleaver's with n_tx = E and no hole list.  Those kernels never assume an injection: they gather
static inline IlTab rm_as_il(const RmTab &rm) { return IlTab{rm.pos, nullptr, rm.E, rm.N, 0}; }

// ldpc_demap_dev_rm: d_llr [batch][N] <- (accumulate: +=) per position the left-to-right float32 sum of the LLRs of d_sym
// [batch][ceil(E / m)][2] whose transmitted bits name it; d_gain [batch][n_sym] or null; inv = float32(1 / (2 sigma^2))
int demap_rm_launch(hipStream_t st, const ModTab &tab, int m, int rule, const RmTab &rm, int batch, const float *d_sym, const float *d_gain, float inv, void *d_llr, int fmt,
                    float qscale, bool accumulate);
int demap_rm_product_launch(hipStream_t st, const AxisTab &tab, int b, int rule, const RmTab &rm, int batch, const float *d_sym, const float *d_gain, float inv, void *d_llr,
                            int fmt, float qscale, bool accumulate);
// ldpc_ratematch_llr_dev: the same with the LLR of transmitted bit t loaded from d_llr_tx [batch][E] float32
int ratematch_llr_launch(hipStream_t st, const RmTab &rm, int batch, const float *d_llr_tx, void *d_llr, int fmt, float qscale, bool accumulate);

}  // namespace ldpc

// (host) the object behind include/ldpc_hip.h ldpc_ratematch
struct ldpc_ratematch {
    int E = 0, N = 0, device = -1;
    int max_pos = 0;                           // the largest entry: the frame source's path needs it below its n_tx
    std::vector<int32_t> pos;                  // [E]
    std::vector<int32_t> inv_ptr, inv_t;       // [N + 1], [E]
    int32_t *d_tab = nullptr;                  // one allocation: pos [E] | pad [kIlPad, rounded up to 4 entries] | inv_ptr [N + 1, rounded up] | inv_t [E]
    ldpc::RmTab tab{};
};
