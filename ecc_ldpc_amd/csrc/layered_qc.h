// layered_qc.h -- quasi-cyclic decoders with one workgroup per frame and the state (or its records) in HBM: the constructors and
// the conditions make_backend (select.cc) checks before calling them
#pragma once
#include "backend.h"

namespace ldpc {
// layered_qc.hip.  flooding = 0: the layered schedule (layers = block rows); 1: the reference's flooding schedule with the same mapping
const char *layered_qc_why_not(const ldpc_code &c, int variant, int dtype, int flooding);
Backend *layered_qc_create(const ldpc_code &c, int variant, int dtype, int max_batch, int flooding);
// layered_lds.hip: lam on-chip as fp16, row records streamed from HBM -- layered min-sum with LDPC_F16 lam storage on QC codes whose
// frame fits LDS in fp16
const char *layered_lds_why_not(const ldpc_code &c, int variant, int dtype);
Backend *layered_lds_create(const ldpc_code &c, int max_batch);
// layered_csr.hip: the same for ANY H (column table in device memory, the code's layers merged into barrier steps) -- min-sum with
// lam stored as fp16 (LDPC_F16, 2 N bytes of LDS) or as f32 (LDPC_F32, 4 N bytes: N <= 40 952; with the non-finite veto), or the
// int8 fixed-point decoder (LDPC_I8, N bytes; llr_qscale: its quantiser's scale); lam never leaves the chip, so the context reports
// LDPC_PATH_FUSED.  rule: a check-node rule other than the 3/4 (backend.h CnRule; layered_csr_kernel<D, Ruled<LT>>, or <D, MinStar<LT>> for kind LDPC_CN_AMINSTAR), null for the 3/4
const char *layered_csr_why_not(const ldpc_code &c, int variant, int dtype);
Backend *layered_csr_create(const ldpc_code &c, int dtype, int max_batch, float llr_qscale = 0.f, const CnRule *rule = nullptr);
}  // namespace ldpc
