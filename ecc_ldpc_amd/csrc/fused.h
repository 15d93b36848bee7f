// fused.h -- the fused on-chip decoders (LDPC_PATH_FUSED): one launch decodes a batch, all BP state stays in LDS/registers
// between iterations.  Constructors and the conditions make_backend (select.cc) checks before calling them.
#pragma once
#include "backend.h"

namespace ldpc {
// built-in instances for quasi-cyclic codes with compile-time tables (fused.hip)
enum FusedKind {
    FUSED_SPLIT,         // fused_split.hip    four waves per frame, block rows split between wave pairs (f32)
    FUSED_MSG,           // fused_msg.hip      per-edge-message two-wave kernel, table-driven (f32, f64)
    FUSED_PK16,          // fused_pk16.hip     LDPC_F16PK: packed fp16 arithmetic, two frames per lane
    FUSED_LAYERED,       // fused_layered.hip  LDPC_SCHED_LAYERED on-chip (f32)
    FUSED_LAYERED_PK16,  // fused_layered.hip  the same in packed fp16
};
// dtype: the compute type; static_id: the compiled-in rotation table (fused_msg_static_id; 0 = none); round16: an LDPC_F16 context
// (its LLRs count as stored in fp16)
Backend *fused_qc_create(const ldpc_code &c, int variant, int dtype, FusedKind kind, int static_id, int round16);
// the same kernels specialised at run time for any single-circulant QC code (jit.cc; kind: JitKind)
Backend *fused_jit_create(const ldpc_code &c, int variant, int dtype, int kind, int round16);
// generic on-chip kernel for any H whose frame fits in LDS (fused_csr.hip)
const char *fused_csr_why_not(const ldpc_code &c, int variant, int dtype);
Backend *fused_csr_create(const ldpc_code &c, int variant, int dtype, int round16);
}  // namespace ldpc
