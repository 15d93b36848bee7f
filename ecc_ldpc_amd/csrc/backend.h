// backend.h -- the one decoder a context owns (host side).  Every kernel family implements this interface in its own
// translation unit and owns its own buffers; make_backend (select.cc) decides which family and instance a context gets.
//
// One backend's decode never runs twice at once on the device: the host-pointer entry points (api.cc decode_host) start each
// chunk's decode after the previous chunk's has ended, whichever slot stream it is on, and device-pointer callers order their
// streams (include/ldpc_hip.h).  So a backend may keep mutable device state across launches: fused_csr.hip's and
// layered_lds.hip's work counters, the HBM state of flood.hip and layered_qc.hip.
#pragma once
#include "internal.h"

namespace ldpc {

struct Backend {
    int path = LDPC_PATH_FUSED;   // what ldpc_ctx_path reports: LDPC_PATH_FUSED (state on-chip) or LDPC_PATH_FLOOD (state in HBM)
    KernelTimer *timer = nullptr; // the context's event bracket around the dominant kernel (set by the context after creation)
    // the dominant kernel's name and geometry (ldpc_ctx_kernel_name / _geometry): set at creation, or by the first decode launch of
    // families whose instance depends on the call
    LaunchInfo info;
    virtual ~Backend() {}
    // d_llr [batch][N] of element type llr_fmt (LLR_F32 / LLR_F64 / LLR_F16; LLR_I8 reaches LDPC_I8 contexts only: api.cc decode_dev);
    // device outputs, all but d_bits may be null
    virtual int decode(hipStream_t st, int max_iters, int batch, const void *d_llr, int llr_fmt, uint8_t *d_bits, int32_t *d_iters,
                       uint8_t *d_conv, double *d_final, double *d_trace) = 0;
    // decode() with the soft output of ldpc_decode_batch_dev_soft (validated by api.cc): d_soft [batch][N] of element type soft_fmt
    // (LDPC_LLR_*), soft_kind LDPC_SOFT_POSTERIOR / _EXTRINSIC.  Served by csrc/layered_csr.hip alone; every other family answers
    // LDPC_EUNSUPPORTED with its own name
    virtual int decode_soft(hipStream_t, int, int, const void *, int, uint8_t *, int32_t *, uint8_t *, void *, int, float, int) {
        return set_error(LDPC_EUNSUPPORTED, "no soft output from %s: ldpc_decode_batch_dev_soft is served by the on-chip layered min-sum kernel for any H "
                         "(ldpc::layered_csr_kernel: min-sum, LDPC_SCHED_LAYERED, dtype LDPC_F16, LDPC_F32 or LDPC_I8, with or without a check-node rule)", kernel_name());
    }
    // A DECODE STATE (ldpc_decode_state, api.cc): per frame slot, the check-to-variable messages -- as the row records of the family that
    // serves it -- and the sum of check messages per column.  decode_state_bytes: the device bytes of one slot's records and of its sums
    // (api.cc allocates slots x each; a zero fill is a reset slot).  decode_continue: decode_soft() that starts from slots first .. first +
    // batch - 1 of that memory and leaves the new state there (ldpc_decode_batch_dev_continue, validated by api.cc); d_soft may be null.
    // Served by csrc/layered_csr.hip alone; every other family answers both with LDPC_EUNSUPPORTED and its own name
    virtual int decode_state_bytes(size_t *, size_t *) { return no_decode_state(); }
    virtual int decode_continue(hipStream_t, void *, void *, int, int, int, const void *, int, uint8_t *, int32_t *, uint8_t *, void *, int, float, int) {
        return no_decode_state();
    }
    int no_decode_state() const {
        return set_error(LDPC_EUNSUPPORTED, "no decode state on %s: ldpc_decode_state_create and ldpc_decode_batch_dev_continue are served by the on-chip layered "
                         "min-sum kernel for any H (ldpc::layered_csr_kernel: min-sum, LDPC_SCHED_LAYERED, dtype LDPC_F16, LDPC_F32 or LDPC_I8, with or without a "
                         "check-node rule)", kernel_name());
    }
    // one teacher-forced iteration from given (lam, ne) in f64 (ldpc_debug_step), or LDPC_EUNSUPPORTED with the reason
    virtual int step(hipStream_t st, int batch, const double *d_orig, const double *d_lam, const double *d_ne, double *d_ne_out,
                     double *d_lam_out, uint8_t *d_syn) = 0;
    virtual const char *kernel_name() const { return info.name; }
    // whether decode() reads every channel LLR from memory exactly once (then the LLRs may sit in page-locked HOST memory and be
    // read over PCIe by the kernel itself: api.cc zero-copy path)
    virtual bool reads_llr_once(int max_iters) const = 0;
};

// A min-sum check-node rule other than the library's 3/4 (ldpc_ctx_config cn_scale / cn_offset, validated by api.cc):
// |msg'| = max(scale * min - offset, 0) in float cells; a / 16 and b quantiser steps in the integers of an LDPC_I8 context
// (a = clip(rint(16 scale), 1, 16), b = rint(offset * llr_qscale)).  Served by csrc/layered_csr.hip alone.
// kind LDPC_CN_AMINSTAR (ldpc_ctx_config cn_rule): the A-min* row of layered_csr_kernel<D, MinStar<LT>> instead -- float cells only, the
// other members are not read.
struct CnRule { float scale, offset; int a, b; int kind = LDPC_CN_MINSUM; };

// The decoder for a validated context configuration (api.cc ldpc_ctx_create_cfg), on the calling thread's current device, whose
// graph tables are `tabs`.  nullptr + set_error when no kernel serves the configuration or creating it failed.  llr_qscale: the
// quantiser's scale of an LDPC_I8 context.  rule: null for the 3/4 every kernel computes with, else the context's check-node rule.
Backend *make_backend(const ldpc_code &c, const ldpc_code_dev &tabs, int variant, int dtype, int schedule, int sum_order, int path,
                      int max_batch, float llr_qscale = 0.f, const CnRule *rule = nullptr);

// null when the row-layered schedule's layers are the block rows of the code's QC description, else why not
const char *layers_why_not(const ldpc_code &c);

// batch-major flood path for any H (flood.hip), flooding or layered schedule; pairs4: see FloodDev
Backend *flood_create(const ldpc_code &c, const ldpc_code_dev &tabs, int variant, int dtype, int schedule, int sum_order, int pairs4,
                      int max_batch);

}  // namespace ldpc
