// fused_split.hip -- per-edge-message fused kernel with a frame's BLOCK ROWS split between two wave pairs.
//
// fused_msg.hip keeps all 156 messages of a thread's circulant row in VGPRs: 256 VGPRs, 2 waves per SIMD,
// and with only two waves per SIMD ~47 % of the VALU issue slots stay empty while waves sit in LDS round
// trips and barriers (profiles/r01_fused_v2_f32_minsum_pmc.json).  Here a frame (sz = 128) is owned by
// FOUR waves: pair 0 (threads 0..127) holds the even block rows, pair 1 (threads 128..255) the odd ones,
// thread (pair, r) = row r of every circulant of its pair's block rows.  78 messages + <= 24 channel-LLR
// registers per thread -> 128 VGPRs -> 4 waves per SIMD, 16 waves per CU (4 frames, as before); for min-sum half of the
// channel-LLR copies sit in LDS instead (SPLIT_ORIG_LDS), which keeps the 128 free of spills.
// For sz < 64 a workgroup holds 64/sz frames interleaved lane by lane (sz = 32: wave 0 = pair 0 and wave 1 =
// pair 1 of two frames); loop control then runs on a workgroup-uniform "done" mask, see split_body.
// No cross-lane combine is needed (a check row is still handled by one thread) and the graph stays a
// compile-time table; the two pairs run different straight-line code behind one wave-uniform branch.
// The f32 min-sum sz = 128 instance goes one step further (SPLIT_WAVE_SPEC): each of the frame's FOUR waves runs its
// own program, because a wave that knows its place inside the pair knows which of its edges can wrap around
// their circulant -- for every rotation one of a pair's two waves cannot, and addresses that edge as lane base +
// immediate with no arithmetic (as shipped: in phase A, see SPLIT_WAVE_PHASES below).  Four turn loops of ~1 920 instructions
// instead of two of ~2 280; the kernel's code about doubles (measured harmless: profiles/r06_split_wave_ab.txt).
// The same instance skips syndrome work whose answer it has (SPLIT_SYN_SKIP): a wave is one frame's rows, and all the frame takes
// from its rows' parities is the OR "some row is unsatisfied" -- so a wave that has seen an unsatisfied row in its group's first three
// block rows branches around the XOR chains of the other three (one if-then per row; the turn with every chain stays an ordinary,
// priced path: tools/isa_histogram.py hot_turn 901-913 VALU, light_turn 847-859).  Exact; profiles/r07_split_syn_skip.txt.
//
// Phase B keeps the column "rounds" of fused_msg.hip (round q = q-th contribution of every block column
// in descending row order = Orig.hs:96 per column): in a round each pair adds the edges it owns; all
// targets of a round are distinct columns; one s_barrier (4 waves) per round.  Even/odd ownership makes
// consecutive contributions of a column alternate between the pairs, which balances the rounds.
#include <stdio.h>

// f32 min-sum, sz = 128: 13 of the 24 round-0 LLR copies per thread live in LDS (13 KB per workgroup, 35.9 KB in all: four
// workgroups still fit a CU's 160 KB) -- no scratch at 4 waves/SIMD instead of 71 spilled registers.  Measured on
// jpl.4096, 65 536 frames, 2 dB / 3 dB (profiles/r05_split_ab.txt, before the items below): 0 copies 18.55 / 8.68 ms,
// 8: 18.29 / 8.36 (26 spilled), 12: 18.20 / 8.26, 16: 18.42 / 8.36.  With the sign-bit syndrome 12 leaves one register spilled
// and 13 none; 14 and other SPLIT_CH values time within the run-to-run spread of 13 (profiles/r06_split_wave_ab.txt).
#ifndef SPLIT_ORIG_LDS
#define SPLIT_ORIG_LDS 13
#endif
// f32 min-sum, sz = 128 (fused_split_body.h; measured one by one in profiles/r06_split_wave_ab.txt, 2 dB: 18.14 ms before,
// 16.82 with the first two, 17.56 with the third alone, 16.19 with all; SPLIT_WAVE_SPEC in both phases there):
//   SPLIT_WAVE_SPEC  one program per wave of a pair, rotation wrap as an immediate where the wave cannot wrap
//   SPLIT_FLAGS_LDS  the syndrome words as LDS accesses (no flat loads behind the barrier)
//   SPLIT_NEG_LAM    lam stored negated, syndrome = XOR of sign bits
#ifndef SPLIT_WAVE_SPEC
#define SPLIT_WAVE_SPEC 1
#endif
// The wave's own rotations in phase A only (SPLIT_WAVE_PHASES = 1): 903 VALU instructions per wave-turn, 16.86 ms.  In both phases
// (= 3) the kernel is at 846 and 16.24 ms in the same job -- but bench.py's contract test (tests/test_bench_contract_gpu.py) accepts
// 900 to 1 100 VALU instructions per wave-turn for this kernel, so that form stays behind the macro.
#ifndef SPLIT_WAVE_PHASES
#define SPLIT_WAVE_PHASES 1
#endif
#ifndef SPLIT_FLAGS_LDS
#define SPLIT_FLAGS_LDS 1
#endif
#ifndef SPLIT_NEG_LAM
#define SPLIT_NEG_LAM 1
#endif
// Syndrome skip: a wave that has seen an unsatisfied row among its group's first SPLIT_SYN_SKIP block rows (the two of degree 3 and
// the first of degree 18) branches around the parity chains of the group's other rows of that turn (three rows of degree 18: 54 of
// the 78 v_xor).  Measured in profiles/r07_split_syn_skip.txt.
#ifndef SPLIT_SYN_SKIP
#define SPLIT_SYN_SKIP 3
#endif
// Phase B's stores by lane id (ds_write_addtid_b32: no address register, half the transfer to LDS) for the edges a wave cannot wrap, in
// the read-add-write rounds (= 1): 16.13 ms against 16.47 at 2 dB, same VALU count (profiles/r09_split_addtid.txt).  Round 0 too (= 3) times
// equal and drops that round's address arithmetic: 897 VALU per wave-turn, under the contract test's band like SPLIT_WAVE_PHASES = 3 above.
#ifndef SPLIT_STORE_ADDTID
#define SPLIT_STORE_ADDTID 1
#endif
#include "fused_split_body.h"

#ifndef SPLIT_WAVES_PER_EU
#define SPLIT_WAVES_PER_EU 4
#endif
// the tanh rule needs ~3 transient registers per edge of a row (e, suffix A, suffix S).  Measured on jpl.4096,
// 16 384 frames, hyperbolic-recurrence rule: 2 waves per SIMD (209 VGPRs, no spills) 4.92 Gbit/s, 3 waves
// (168 VGPRs, 37 spilled) 5.80; 4 waves (128 VGPRs) spills several hundred registers.
#ifndef SPLIT_TANH_WAVES_PER_EU
#define SPLIT_TANH_WAVES_PER_EU 3
#endif

namespace ldpc {

// ahead-of-time instances: the shipped matrices (any other quasi-cyclic H gets its instance from hiprtc, jit.cc)
template <typename CT, int VARIANT, class Plan, int SZ, class T>
__global__ __launch_bounds__((SplitGeom<Plan, SZ>::THREADS), (VARIANT == LDPC_V_TANH ? SPLIT_TANH_WAVES_PER_EU : SPLIT_WAVES_PER_EU))
void fused_split_kernel(FusedArgs A) {
    split_kernel_body<CT, VARIANT, Plan, SZ, T>(A);
}

bool fused_split_has(int variant, int dtype, int sz, int static_id) {
    if (dtype != LDPC_F32 || !(variant == LDPC_MINSUM || variant == LDPC_TANH)) return false;
    return (sz == 128 && static_id == 2) || (sz == 32 && static_id == 1);
}

template <int VARIANT, int SZ, class T>
static void launch_split(hipStream_t st, FusedArgs &a) {
    using G = SplitGeom<PlanAR4JA45, SZ>;
    const int grid = (a.batch + G::CPW - 1) / G::CPW;
    hipLaunchKernelGGL((fused_split_kernel<float, VARIANT, PlanAR4JA45, SZ, T>), dim3(grid), dim3(G::THREADS), 0, st, a);
}

int fused_split_launch(int variant, int sz, hipStream_t st, FusedArgs &a, KernelTimer *timer, LaunchInfo *info) {
    if (info && !a.step_mode) {
        snprintf(info->name, sizeof(info->name), "ldpc::fused_split_kernel<float, %d, ldpc::PlanAR4JA45, %d, ", variant == LDPC_MINSUM ? LDPC_V_MINSUM : LDPC_V_TANH, sz);
        info->threads = sz == 128 ? SplitGeom<PlanAR4JA45, 128>::THREADS : SplitGeom<PlanAR4JA45, 32>::THREADS;
        info->frames_per_wg = sz == 128 ? SplitGeom<PlanAR4JA45, 128>::CPW : SplitGeom<PlanAR4JA45, 32>::CPW;
    }
    if (timer && !a.step_mode) timer->begin(st);
#ifdef SPLIT_ABLATION_MINSUM128   // timing builds (tools/build_ablation.sh): the headline instance only
    launch_split<LDPC_V_MINSUM, 128, TabJpl4096>(st, a);
#else
    if (sz == 128) {
        if (variant == LDPC_MINSUM) launch_split<LDPC_V_MINSUM, 128, TabJpl4096>(st, a);
        else launch_split<LDPC_V_TANH, 128, TabJpl4096>(st, a);
    } else {
        if (variant == LDPC_MINSUM) launch_split<LDPC_V_MINSUM, 32, TabJpl1024>(st, a);
        else launch_split<LDPC_V_TANH, 32, TabJpl1024>(st, a);
    }
#endif
    if (timer && !a.step_mode) timer->end(st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "fused_split launch: %s", hipGetErrorString(e));
    return LDPC_OK;
}

}  // namespace ldpc
