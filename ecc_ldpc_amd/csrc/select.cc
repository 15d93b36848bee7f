// select.cc -- which decoder a context gets.  make_backend walks the preference ladder below and returns the first candidate the
// configuration allows and that builds; every kernel family is a Backend (backend.h) in its own translation unit.
//
// On-chip, state in LDS/registers (LDPC_PATH_FUSED; LDPC_PATH_AUTO whenever such a kernel exists).  Flooding schedule, in order of
// preference for a quasi-cyclic code:
//   (1) fused_split.hip   built-in instances of the four-wave split kernel for the shipped matrices (compile-time tables)
//   (2) jit.cc            the same kernel specialised at run time for any other single-circulant QC code
//   (3) fused_msg.hip     two-wave per-edge-message kernel, table-driven (AR4JA block structure; f64 parity mode;
//                         what runs when run-time compilation is off or unavailable)
//   (4) fused_csr.hip     generic on-chip kernel for any H whose frame fits in LDS
// LDPC_F16PK: fused_pk16.hip's built-in instances, else jit.cc.  Layered schedule: fused_layered.hip's built-in instances, else
// jit.cc -- and when that compilation fails under LDPC_PATH_AUTO, the frame-per-workgroup kernels below.
// State in HBM (LDPC_PATH_FLOOD; LDPC_PATH_AUTO otherwise):
//   (5) layered_lds.hip   layered min-sum with fp16 lam storage whose frame fits LDS: lam on-chip, row records streamed
//   (6) layered_qc.hip    QC codes, either schedule: one workgroup per frame
//   (7) flood.hip         any H, batch-major (lane = frame): flooding and layered schedules, fp16 storage, the parity modes
// Layered min-sum where none of the above serves it (reported as FUSED):
//   (8) layered_csr.hip   any H whose frame fits LDS: lam on-chip, row records streamed, layers merged into barrier steps
//                         - lam as fp16 (LDPC_F16, N <= 65 535): LDPC_PATH_AUTO or LDPC_PATH_FUSED
//                         - lam as f32 (LDPC_F32, N <= 40 952): LDPC_PATH_FUSED only.  LDPC_PATH_AUTO keeps such a context on (7): that
//                           routing follows a measurement of this instance against flood.hip's layered kernel on the same frames and
//                           layers (tools/layered_csr_rate.py --lam f32), it does not precede it
//                         - lam as int8 (LDPC_I8, the fixed-point decoder): the only kernel of that dtype, so it is taken ahead of the
//                           ladder, on any code (a QC code as its CSR form, with the layers it has): LDPC_PATH_AUTO or LDPC_PATH_FUSED
//                         - a check-node rule other than the 3/4 (cn_scale / cn_offset; LDPC_F16, LDPC_F32 or LDPC_I8): only this family
//                           has instances that read one (layered_csr_kernel<D, Ruled<LT>>), so such a context is routed here ahead of the ladder
//                           too, a QC code as its CSR form: LDPC_PATH_AUTO or LDPC_PATH_FUSED
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "backend.h"
#include "fused.h"
#include "fused_common.h"
#include "jit.h"
#include "layered_qc.h"

namespace ldpc {

const char *layers_why_not(const ldpc_code &c) {
    bool same = (int)c.layer_ptr.size() == c.block_rows + 1;
    for (int br = 0; same && br <= c.block_rows; br++) same = c.layer_ptr[br] == br * c.sz;
    return same ? nullptr : "layers were replaced: not the block rows";
}

int jit_kind_of(int dtype, int schedule) {
    if (schedule == LDPC_SCHED_LAYERED) return dtype == LDPC_F16PK ? JIT_LAYERED_PK16 : JIT_LAYERED;
    return dtype == LDPC_F16PK ? JIT_PK16 : JIT_SPLIT;
}

// ------------------------------------------------------------------ built-in QC instances
static bool plan_matches_ar4ja45(const ldpc_code &c) {
    if (c.sz <= 0 || c.block_rows != PlanAR4JA45::NBR || c.block_cols != PlanAR4JA45::NBC) return false;
    for (int br = 0; br < c.block_rows; br++) {
        int d = 0;
        for (int bc = 0; bc < c.block_cols; bc++) d += c.offsets[(size_t)br * c.block_cols + bc] >= 0;
        if (d != PlanAR4JA45::deg(br)) return false;
    }
    return true;
}

// the compiled-in rotation table matching the code's circulants, in block-row order (0 = none)
static int builtin_static_id(const ldpc_code &c) {
    std::vector<uint16_t> rot; std::vector<uint8_t> bcv;
    for (int br = 0; br < c.block_rows; br++)
        for (int bc = 0; bc < c.block_cols; bc++) {
            int off = c.offsets[(size_t)br * c.block_cols + bc];
            if (off >= 0) { rot.push_back((uint16_t)off); bcv.push_back((uint8_t)bc); }
        }
    return fused_msg_static_id(c.sz, rot.data(), bcv.data(), (int)rot.size());
}

static bool pk16_builtin(const ldpc_code &c, int variant) {
    return c.sz > 0 && plan_matches_ar4ja45(c) && fused_pk16_has(variant, c.sz, builtin_static_id(c));
}
static bool layered_builtin(const ldpc_code &c, int variant, int dtype) {
    return plan_matches_ar4ja45(c) && fused_layered_has(variant, dtype, c.sz, builtin_static_id(c));
}

// LDPC_F16PK: the built-in instances (compile-time tables of the shipped AR4JA matrices), any other single-circulant QC code
// through the run-time compiler (jit.cc JIT_PK16)
static const char *pk16_why_not(const ldpc_code &c, int variant) {
    if (variant != LDPC_MINSUM) return "the packed-fp16 kernel implements min-sum";
    if (c.sz == 0) return "the packed-fp16 kernel takes quasi-cyclic codes (built-in instances for codes/jpl.1024.4.5 and codes/jpl.4096.4.5, run-time specialised ones for any other single-circulant .q)";
    if (pk16_builtin(c, variant)) return nullptr;
    return jit_split_why_not(c, variant, LDPC_F16PK, JIT_PK16);
}

static const char *fused_layered_why_not(const ldpc_code &c, int variant, int dtype) {
    if (variant != LDPC_MINSUM) return "the on-chip layered kernel implements min-sum";
    if (dtype != LDPC_F32 && dtype != LDPC_F16 && dtype != LDPC_F16PK) return "the on-chip layered kernels compute in f32 or packed fp16";
    if (c.sz == 0) return "the on-chip layered kernels take quasi-cyclic codes";
    if (const char *l = layers_why_not(c)) return l;
    const char *e = getenv("LDPC_LAYERED_FUSED");
    if (e && !strcmp(e, "0")) return "disabled (LDPC_LAYERED_FUSED=0)";
    if (layered_builtin(c, variant, dtype)) return nullptr;
    // any other single-circulant QC code: the same bodies specialised at run time
    return jit_split_why_not(c, variant, dtype == LDPC_F16PK ? LDPC_F16PK : LDPC_F32, jit_kind_of(dtype, LDPC_SCHED_LAYERED));
}

static const char *plan_why_not(const ldpc_code &c, int variant, int dtype) {
    if (variant == LDPC_TANH && dtype != LDPC_F32) return "the fused tanh kernel exists for f32 only (f64 tanh: flood path)";
    if (dtype != LDPC_F32 && dtype != LDPC_F64) return "fused kernels exist for f32 and f64";
    if (c.sz == 0) return "code was not created from a quasi-cyclic description";
    if (!(c.sz == 32 || c.sz == 64 || c.sz == 128)) return "circulant size must be 32, 64 or 128";
    if (!plan_matches_ar4ja45(c)) return "block structure is not the AR4JA rate-4/5 plan (12x44 blocks, row weights 3,3,3,3,18x8)";
    return nullptr;
}
// LDPC_F16 = "fp16 storage in HBM, f32 arithmetic".  The only thing a fused decode keeps in HBM is the channel
// LLRs, so a fused F16 context is the f32 kernel fed fp16-rounded LLRs.
static inline int compute_dtype(int dtype) { return dtype == LDPC_F16 ? LDPC_F32 : dtype; }

// a fused (on-chip) kernel for the flooding schedule exists if the code matches a compiled QC plan, or failing that if a frame
// fits in LDS
static const char *fused_why_not(const ldpc_code &c, int variant, int dtype) {
    if (dtype == LDPC_F16PK) return pk16_why_not(c, variant);
    dtype = compute_dtype(dtype);
    const char *p = plan_why_not(c, variant, dtype);
    if (!p) return nullptr;
    const char *j = jit_split_why_not(c, variant, dtype);
    if (!j) return nullptr;
    const char *g = fused_csr_why_not(c, variant, dtype);
    if (!g) return nullptr;
    static thread_local char buf[600];
    snprintf(buf, sizeof(buf), "built-in QC kernel: %s; run-time specialised QC kernel: %s; generic on-chip kernel: %s", p, j, g);
    return buf;
}

// ------------------------------------------------------------------ the ladder
// on-chip, flooding schedule (fused_why_not is null)
static Backend *onchip_flooding(const ldpc_code &c, int variant, int dtype) {
    if (dtype == LDPC_F16PK) {
        if (pk16_builtin(c, variant)) return fused_qc_create(c, variant, LDPC_F16PK, FUSED_PK16, 0, 0);
        return fused_jit_create(c, variant, LDPC_F16PK, jit_kind_of(dtype, LDPC_SCHED_FLOODING), 0);
    }
    const int round16 = dtype == LDPC_F16;
    dtype = compute_dtype(dtype);
    const char *table = getenv("LDPC_FUSED_TABLE");    // =dyn: the table-driven kernel (not the run-time compiler either)
    const char *kernel = getenv("LDPC_FUSED_KERNEL");  // =msg: the two-wave kernel where the four-wave split kernel exists
    const bool dyn = table && !strcmp(table, "dyn"), msg_only = kernel && !strcmp(kernel, "msg");
    const char *plan = plan_why_not(c, variant, dtype);
    const int static_id = plan || dyn ? 0 : builtin_static_id(c);
    // (1) a built-in instance with compile-time tables (the shipped matrices), or an A/B switch naming a built-in kernel; else (2)
    // the split kernel specialised at run time -- unless that cannot be built (compiler missing, shape out of range), in which
    // case (3) the table-driven two-wave kernel if the block structure is the AR4JA plan, else (4) the generic on-chip kernel
    const bool builtin = !plan && ((dtype == LDPC_F32 && (dyn || static_id != 0)) || msg_only);
    if (!builtin && jit_split_why_not(c, variant, dtype) == nullptr) {
        if (Backend *b = fused_jit_create(c, variant, dtype, jit_kind_of(dtype, LDPC_SCHED_FLOODING), round16)) return b;
        fprintf(stderr, "[libldpc_hip] run-time specialisation failed (%s); using a table-driven kernel\n", ldpc_last_error());
    }
    if (plan) {
        if (fused_csr_why_not(c, variant, dtype) != nullptr) {
            const char *why = fused_why_not(c, variant, dtype);
            set_error(LDPC_EUNSUPPORTED, "no fused kernel could be built for this code (%s)", why ? why : "run-time compilation failed");
            return nullptr;
        }
        return fused_csr_create(c, variant, dtype, round16);
    }
    if (!fused_msg_has(variant, dtype, c.sz)) { set_error(LDPC_EUNSUPPORTED, "no fused kernel"); return nullptr; }
    const bool split = fused_split_has(variant, dtype, c.sz, static_id) && !msg_only;
    return fused_qc_create(c, variant, dtype, split ? FUSED_SPLIT : FUSED_MSG, static_id, round16);
}

// on-chip, layered schedule (fused_layered_why_not is null)
static Backend *onchip_layered(const ldpc_code &c, int variant, int dtype) {
    const bool pk16 = dtype == LDPC_F16PK;
    const int round16 = dtype == LDPC_F16;
    if (layered_builtin(c, variant, dtype))
        return fused_qc_create(c, variant, pk16 ? LDPC_F16PK : LDPC_F32, pk16 ? FUSED_LAYERED_PK16 : FUSED_LAYERED, 0, round16);
    return fused_jit_create(c, variant, pk16 ? LDPC_F16PK : LDPC_F32, jit_kind_of(dtype, LDPC_SCHED_LAYERED), round16);
}

// state in HBM, one workgroup per frame (layered_qc_why_not is null)
static Backend *frame_per_workgroup(const ldpc_code &c, int variant, int dtype, int max_batch, int flooding) {
    if (!flooding && layered_lds_why_not(c, variant, dtype) == nullptr) return layered_lds_create(c, max_batch);
    return layered_qc_create(c, variant, dtype, max_batch, flooding);
}

Backend *make_backend(const ldpc_code &c, const ldpc_code_dev &tabs, int variant, int dtype, int schedule, int sum_order, int path,
                      int max_batch, float llr_qscale, const CnRule *rule) {
    if (rule && rule->kind == LDPC_CN_AMINSTAR) {     // the A-min* row: the same family's MinStar instances, float cells only
        const char *why = dtype == LDPC_I8 ? "LDPC_I8 (an integer A-min* does not exist: LDPC_F16 or LDPC_F32 only)"
                          : schedule != LDPC_SCHED_LAYERED ? "the flooding schedule (LDPC_SCHED_LAYERED only)"
                          : variant != LDPC_MINSUM || sum_order != LDPC_SUM_REFERENCE ? "any variant but LDPC_MINSUM (the tanh rule and the parity modes have a check-node rule of their own)"
                          : dtype != LDPC_F16 && dtype != LDPC_F32 ? "this dtype (LDPC_F16 or LDPC_F32 only)"
                          : path == LDPC_PATH_FLOOD ? "LDPC_PATH_FLOOD (lam is kept on-chip: LDPC_PATH_AUTO or LDPC_PATH_FUSED)"
                          : layered_csr_why_not(c, variant, dtype);
        if (why) { set_error(LDPC_EUNSUPPORTED, "cn_rule = LDPC_CN_AMINSTAR (the A-min* check-node rule) does not serve this request: %s", why); return nullptr; }
        return layered_csr_create(c, dtype, max_batch, 0.f, rule);
    }
    if (rule) {     // a check-node rule other than the 3/4: layered min-sum in csrc/layered_csr.hip (layered_csr_kernel<D, Ruled<LT>>), nothing else
        const char *why = schedule != LDPC_SCHED_LAYERED ? "the flooding schedule (its kernels compute 3/4 min, always; LDPC_SCHED_LAYERED only)"
                          : variant != LDPC_MINSUM || sum_order != LDPC_SUM_REFERENCE ? "any rule but min-sum (the tanh rule and the parity modes have no scale or offset)"
                          : dtype != LDPC_F16 && dtype != LDPC_F32 && dtype != LDPC_I8 ? "this dtype (LDPC_F16, LDPC_F32 or LDPC_I8 only)"
                          : path == LDPC_PATH_FLOOD ? "LDPC_PATH_FLOOD (lam is kept on-chip: LDPC_PATH_AUTO or LDPC_PATH_FUSED)"
                          : layered_csr_why_not(c, variant, dtype);
        if (why) { set_error(LDPC_EUNSUPPORTED, "a check-node rule (cn_scale / cn_offset) other than 3/4 min does not serve this request: %s", why); return nullptr; }
        return layered_csr_create(c, dtype, max_batch, dtype == LDPC_I8 ? llr_qscale : 0.f, rule);
    }
    if (dtype == LDPC_I8) {     // the int8 fixed-point decoder: layered min-sum in csrc/layered_csr.hip, nothing else
        const char *why = schedule != LDPC_SCHED_LAYERED ? "the flooding schedule (LDPC_SCHED_LAYERED only)"
                          : variant != LDPC_MINSUM || sum_order != LDPC_SUM_REFERENCE ? "any rule but min-sum"
                          : path == LDPC_PATH_FLOOD ? "LDPC_PATH_FLOOD (lam is kept on-chip: LDPC_PATH_AUTO or LDPC_PATH_FUSED)"
                          : layered_csr_why_not(c, variant, dtype);
        if (why) { set_error(LDPC_EUNSUPPORTED, "LDPC_I8 (int8 fixed-point layered min-sum) does not serve this request: %s", why); return nullptr; }
        return layered_csr_create(c, dtype, max_batch, llr_qscale);
    }
    if (dtype == LDPC_F16PK && (variant != LDPC_MINSUM || path == LDPC_PATH_FLOOD)) {
        set_error(LDPC_EUNSUPPORTED, "LDPC_F16PK (packed fp16 arithmetic, two frames per lane) exists for min-sum on the on-chip path");
        return nullptr;
    }
    const bool layered = schedule == LDPC_SCHED_LAYERED;
    // (the parity modes exist on the flood path only: the context configuration rejects them with LDPC_PATH_FUSED or the layered schedule)
    const bool parity = variant == LDPC_TANH_CM || variant == LDPC_TANH_CUDA32 || sum_order != LDPC_SUM_REFERENCE;
    // why no on-chip kernel serves this context (null: one does)
    const char *onchip_why = layered ? fused_layered_why_not(c, variant, dtype) : parity ? "parity mode" : fused_why_not(c, variant, dtype);
    const char *csr_why = "";   // why the on-chip layered kernel for any H does not serve this context ("" = not considered)
    if (layered) {
        // (8) layered_csr.hip, lam on-chip for ANY H; its fp16-lam instances -- only where no kernel above serves the request: no on-chip QC kernel,
        // and under LDPC_PATH_AUTO no HBM kernel of a QC code either (an explicit LDPC_PATH_FLOOD keeps the state in HBM and is refused)
        if (dtype == LDPC_F16 && onchip_why && path != LDPC_PATH_FLOOD && (path == LDPC_PATH_FUSED || layered_qc_why_not(c, variant, dtype, 0) != nullptr)) {
            csr_why = layered_csr_why_not(c, variant, dtype);
            if (!csr_why) return layered_csr_create(c, dtype, max_batch);
        }
        // its f32-lam instances: on an explicit LDPC_PATH_FUSED only, and only where no on-chip QC kernel exists for the request (a QC code
        // whose on-chip kernel fails to compile still fails under LDPC_PATH_FUSED); LDPC_PATH_AUTO is not re-routed (see the ladder above)
        if (dtype == LDPC_F32 && onchip_why && path == LDPC_PATH_FUSED) {
            csr_why = layered_csr_why_not(c, variant, dtype);
            if (!csr_why) return layered_csr_create(c, dtype, max_batch);
        }
        if (dtype == LDPC_F16 && (onchip_why || path == LDPC_PATH_FLOOD)) {
            // from HBM: lam stored in fp16 for the frame-per-workgroup min-sum record kernel of QC codes (r03); nothing else
            const char *why = layered_qc_why_not(c, variant, dtype, 0);
            if (why) {
                if (*csr_why) set_error(LDPC_EUNSUPPORTED, "the layered schedule with fp16 storage: from HBM: %s; on-chip kernel for any H: %s", why, csr_why);
                else set_error(LDPC_EUNSUPPORTED, "the layered schedule from HBM with fp16 storage: %s", why);
                return nullptr;
            }
        }
        if (c.max_row_deg > 32) { set_error(LDPC_EUNSUPPORTED, "layered schedule: check rows above weight 32 (this code has %d)", c.max_row_deg); return nullptr; }
    }
    if ((path == LDPC_PATH_FUSED || dtype == LDPC_F16PK) && onchip_why) {
        if (layered && *csr_why) set_error(LDPC_EUNSUPPORTED, "no on-chip kernel for the layered schedule on this code / rule / type (%s; on-chip kernel for any H: %s); LDPC_PATH_FLOOD keeps the state in HBM", onchip_why, csr_why);
        else if (layered) set_error(LDPC_EUNSUPPORTED, "no on-chip kernel for the layered schedule on this code / rule / type (%s); LDPC_PATH_FLOOD keeps the state in HBM", onchip_why);
        else set_error(LDPC_EUNSUPPORTED, "no fused kernel for this code/variant/dtype (%s)", onchip_why);
        return nullptr;
    }
    // LDPC_PATH_AUTO takes the on-chip kernel wherever one exists: measured r01 (jpl.4096, 16384 frames): min-sum fused 10.0 vs flood
    // 0.85 Gbit/s; tanh fused 2.09 vs flood 0.73 (before the branch-free phi the fused tanh kernel spilled ~560 VGPRs and lost to
    // flood: 0.53 vs 0.68)
    if (path == LDPC_PATH_FUSED || (path == LDPC_PATH_AUTO && !onchip_why)) {
        Backend *b = layered ? onchip_layered(c, variant, dtype) : onchip_flooding(c, variant, dtype);
        if (b || !layered || path != LDPC_PATH_AUTO || dtype == LDPC_F16PK || layered_qc_why_not(c, variant, dtype, 0) != nullptr) return b;
        // the on-chip layered kernel of this code is compiled at run time and that failed (no compiler on this host, or it rejected the
        // instance): under LDPC_PATH_AUTO the context keeps its state in HBM instead, as onchip_flooding falls back to its table-driven
        // kernels for the flooding schedule
        fprintf(stderr, "libldpc_hip: on-chip layered kernel unavailable (%s); the context runs the layered schedule from HBM\n", ldpc_last_error());
        return frame_per_workgroup(c, variant, dtype, max_batch, 0);
    }
    // ONE predicate for both paths: rows of weight <= 4 take the pair-product form of the tanh rule exactly when the on-chip path of
    // this code is the generic kernel (whose DMAX = 4 instance is written that way) -- a plain graph, or a QC description the
    // split family does not take (circulant size below 16, LDPC_JIT=0, ...).  Such a QC code then also runs its flood path on the
    // batch-major kernels, which know the form; a QC code of the split family uses the chained form everywhere (flood_qc_kernel too).
    const int pairs4 = (variant == LDPC_TANH && dtype != LDPC_F64 && c.max_row_deg <= 4 &&
                        (c.sz == 0 || jit_split_why_not(c, variant, LDPC_F32) != nullptr)) ? 1 : 0;
    // QC code, either schedule: one workgroup per frame, state in HBM (a frame stops when ITS rule fires); any other H, fp16
    // storage and the arraylet-cm parity mode: the batch-major kernels
    const int flooding = layered ? 0 : 1;
    if (sum_order == LDPC_SUM_REFERENCE && variant != LDPC_TANH_CUDA32 && !(pairs4 && flooding) && layered_qc_why_not(c, variant, dtype, flooding) == nullptr)
        return frame_per_workgroup(c, variant, dtype, max_batch, flooding);
    return flood_create(c, tabs, variant, dtype, schedule, sum_order, pairs4, max_batch);
}

}  // namespace ldpc
