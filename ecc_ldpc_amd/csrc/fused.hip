// fused.hip -- host side of the fused on-chip decoders for quasi-cyclic codes (LDPC_PATH_FUSED): the built-in instances
// (fused_split.hip, fused_msg.hip, fused_pk16.hip, fused_layered.hip) and the run-time specialised ones (jit.cc).  One launch
// decodes a batch; a frame's entire BP state stays on-chip for all iterations (lam in LDS, check->variable messages in VGPRs or
// LDS).  Which of them a context gets: make_backend (select.cc).
// (Round 1 also kept a compressed-record kernel here -- the reference's MinSum2/`omit` semigroup, Utils.hs:133-144, as
//  three registers per row; rebuilding messages twice per turn cost ~32 of its ~76 VALU clk per edge and it was removed
//  in round 2; DESIGN.md section 3.1 has its numbers.)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fused.h"
#include "ldpc_math.h"
#include "fused_common.h"
#include "jit.h"

namespace ldpc {

// ------------------------------------------------------------------ built-in instances
struct FusedState : Backend {
    FusedKind kind = FUSED_MSG;
    int variant = 0, dtype = 0, sz = 0;   // dtype: the COMPUTE type (f32/f64; LDPC_F16PK for the packed kinds)
    int round16 = 0;          // LDPC_F16 context: fp16 channel LLRs, f32 state (nothing else of a fused decode lives in HBM)
    int static_id = 0;        // compiled-in rotation table matching this code (0 = none: table-driven kernel)
    uint32_t *d_tab = nullptr;   // graph table of the per-edge-message kernel (FUSED_SPLIT / FUSED_MSG)

    ~FusedState() override { (void)hipFree(d_tab); }
    int decode(hipStream_t st, int max_iters, int batch, const void *d_llr, int llr_fmt, uint8_t *d_bits, int32_t *d_iters,
               uint8_t *d_conv, double *d_final, double *d_trace) override;
    int step(hipStream_t st, int batch, const double *d_orig, const double *d_lam, const double *d_ne, double *d_ne_out,
             double *d_lam_out, uint8_t *d_syn) override;
    // (without template arguments before the first launch, with the instance-selecting ones after it)
    const char *kernel_name() const override {
        static const char *const names[] = {"fused_split_kernel", "fused_msg_kernel", "fused_pk16_kernel", "fused_layered_kernel", "fused_layered_pk16_kernel"};
        return info.name[0] ? info.name : names[kind];
    }
    bool reads_llr_once(int max_iters) const override { return kind != FUSED_MSG && (kind != FUSED_SPLIT || max_iters <= kSplitMaxIters); }
};

Backend *fused_qc_create(const ldpc_code &c, int variant, int dtype, FusedKind kind, int static_id, int round16) {
    FusedState *s = new (std::nothrow) FusedState();
    if (!s) { set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    s->kind = kind; s->variant = variant; s->dtype = dtype; s->sz = c.sz; s->static_id = static_id; s->round16 = round16;
    if (kind != FUSED_SPLIT && kind != FUSED_MSG) return s;
    // per-edge messages: {rotation offset, block-column offset} of every circulant in bytes of this kernel's LDS layout
    const int es = dtype == LDPC_F64 ? 8 : 4;
    const int cpw = c.sz >= 64 ? 1 : 64 / c.sz, V = c.sz * cpw;
    std::vector<uint32_t> tab;
    for (int br = 0; br < c.block_rows; br++)
        for (int bc = 0; bc < c.block_cols; bc++) {
            int off = c.offsets[(size_t)br * c.block_cols + bc];
            if (off < 0) continue;
            uint32_t lo = (uint32_t)(off * cpw * es), hi = (uint32_t)(bc * V * es);
            if (lo > 0xffffu || hi > 0xffffu) { delete s; set_error(LDPC_EUNSUPPORTED, "graph table field overflow"); return nullptr; }
            tab.push_back(lo | (hi << 16));
        }
    hipError_t e = hipMalloc((void **)&s->d_tab, tab.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(s->d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_error(LDPC_EHIP, "fused_create: %s", hipGetErrorString(e)); delete s; return nullptr; }
    return s;
}

int FusedState::decode(hipStream_t st, int max_iters, int batch, const void *d_llr, int llr_fmt, uint8_t *d_bits, int32_t *d_iters,
                       uint8_t *d_conv, double *d_final, double *d_trace) {
    FusedArgs a{};
    a.tab = d_tab; a.llr = d_llr; a.llr_fmt = llr_fmt; a.llr_round16 = round16; a.bits = d_bits; a.iters = d_iters; a.conv = d_conv;
    a.final_lam = d_final; a.trace = d_trace; a.batch = batch; a.max_iters = max_iters; a.step_mode = 0;
    // (the built-in split, packed-fp16 and layered kernels pack a frame's result into one register: 9 bits for the turn it converged at)
    switch (kind) {
        case FUSED_LAYERED:
        case FUSED_LAYERED_PK16:
            if (max_iters > kSplitMaxIters) return set_error(LDPC_EUNSUPPORTED, "on-chip layered kernel: at most %d sweeps (a frame's result is packed into one register)", kSplitMaxIters);
            return kind == FUSED_LAYERED_PK16 ? fused_layered_pk16_launch(sz, st, a, timer, &info) : fused_layered_launch(sz, st, a, timer, &info);
        case FUSED_PK16:
            if (max_iters > kSplitMaxIters) return set_error(LDPC_EUNSUPPORTED, "LDPC_F16PK: at most %d iterations (a frame's result is packed into one register)", kSplitMaxIters);
            return fused_pk16_launch(sz, st, a, timer, &info);
        case FUSED_SPLIT:
            if (max_iters <= kSplitMaxIters) return fused_split_launch(variant, sz, st, a, timer, &info);
            [[fallthrough]];   // (more turns: the two-wave kernel)
        default:
            return fused_msg_launch(variant, dtype, sz, static_id, st, a, timer, &info);
    }
}

static const char kLayeredNoStep[] = "the on-chip layered kernel has no teacher-forced step (use path = LDPC_PATH_FLOOD: the same arithmetic, state in HBM)";
static const char kPk16NoStep[] = "LDPC_F16PK has no teacher-forced step (its state is not the reference's: use ldpc_decode_trace)";

// per-edge messages: the state goes in and out as it is
static FusedArgs step_args(int batch, const double *d_orig, const double *d_lam, const double *d_ne, double *d_ne_out, double *d_lam_out,
                           uint8_t *d_syn) {
    FusedArgs a{};
    a.llr = d_orig; a.llr_fmt = LLR_F64; a.llr_round16 = 0; a.batch = batch; a.max_iters = 1; a.step_mode = 1;
    a.st_lam = d_lam; a.st_ne_in = d_ne; a.st_ne_out = d_ne_out; a.final_lam = d_lam_out; a.st_syn = d_syn;
    return a;
}

int FusedState::step(hipStream_t st, int batch, const double *d_orig, const double *d_lam, const double *d_ne, double *d_ne_out,
                     double *d_lam_out, uint8_t *d_syn) {
    if (kind == FUSED_LAYERED || kind == FUSED_LAYERED_PK16) return set_error(LDPC_EUNSUPPORTED, "%s", kLayeredNoStep);
    if (kind == FUSED_PK16) return set_error(LDPC_EUNSUPPORTED, "%s", kPk16NoStep);
    FusedArgs a = step_args(batch, d_orig, d_lam, d_ne, d_ne_out, d_lam_out, d_syn);
    a.tab = d_tab;
    if (kind == FUSED_SPLIT) return fused_split_launch(variant, sz, st, a, nullptr, nullptr);
    return fused_msg_launch(variant, dtype, sz, static_id, st, a, nullptr, nullptr);
}

// ------------------------------------------------------------------ run-time specialised instances (jit.cc)
struct JitState : Backend {
    JitKernel *jit = nullptr;
    int kind = JIT_SPLIT, round16 = 0;

    ~JitState() override { jit_destroy(jit); }
    int launch(hipStream_t st, FusedArgs &a) {
        const int grid = (a.batch + jit->frames_per_wg - 1) / jit->frames_per_wg;
        void *params[] = {&a};
        if (timer && !a.step_mode) timer->begin(st);
        hipError_t e = hipModuleLaunchKernel(jit->fn, (unsigned)grid, 1, 1, (unsigned)jit->threads, 1, 1, 0, st, params, nullptr);
        if (timer && !a.step_mode) timer->end(st);
        if (e != hipSuccess) return set_error(LDPC_EHIP, "launch of %s: %s", jit->name.c_str(), hipGetErrorString(e));
        return LDPC_OK;
    }
    // (run-time instances: no limit on max_iters)
    int decode(hipStream_t st, int max_iters, int batch, const void *d_llr, int llr_fmt, uint8_t *d_bits, int32_t *d_iters,
               uint8_t *d_conv, double *d_final, double *d_trace) override {
        FusedArgs a{};
        a.llr = d_llr; a.llr_fmt = llr_fmt; a.llr_round16 = round16; a.bits = d_bits; a.iters = d_iters; a.conv = d_conv;
        a.final_lam = d_final; a.trace = d_trace; a.batch = batch; a.max_iters = max_iters; a.step_mode = 0;
        return launch(st, a);
    }
    int step(hipStream_t st, int batch, const double *d_orig, const double *d_lam, const double *d_ne, double *d_ne_out,
             double *d_lam_out, uint8_t *d_syn) override {
        if (kind == JIT_LAYERED || kind == JIT_LAYERED_PK16) return set_error(LDPC_EUNSUPPORTED, "%s", kLayeredNoStep);
        if (kind == JIT_PK16) return set_error(LDPC_EUNSUPPORTED, "%s", kPk16NoStep);
        FusedArgs a = step_args(batch, d_orig, d_lam, d_ne, d_ne_out, d_lam_out, d_syn);
        return launch(st, a);
    }
    bool reads_llr_once(int) const override { return true; }
};

Backend *fused_jit_create(const ldpc_code &c, int variant, int dtype, int kind, int round16) {
    JitKernel *k = jit_split_create(c, variant, dtype, kind);
    if (!k) return nullptr;
    JitState *s = new (std::nothrow) JitState();
    if (!s) { jit_destroy(k); set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    s->jit = k; s->kind = kind; s->round16 = round16;
    snprintf(s->info.name, sizeof(s->info.name), "%s", k->name.c_str());
    s->info.threads = k->threads; s->info.frames_per_wg = k->frames_per_wg;
    return s;
}

}  // namespace ldpc
