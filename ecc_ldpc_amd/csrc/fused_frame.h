// fused_frame.h -- the frame plumbing the four on-chip quasi-cyclic kernel bodies share (split_body in fused_split_body.h, pk::body in
// fused_pk16_body.h, lay::body and laypk::body in fused_layered_body.h).  Those bodies differ in how a check row is computed and
// scheduled; what surrounds the rows is here, once: the workgroup's geometry and LDS layout, which wave group runs which program,
// where a lane's frame(s) live in memory, the per-frame OR over the workgroup, what an LDS word means as a lam (LamCell*), and the
// loops over a lane's own columns that carry lam and hard bits out of the kernel (snapshot at convergence, trace row, result).
// Everything is a __forceinline__ template and every instance compiles to the instructions it had with the pieces written out in
// its body (profiles/r08_frame_plumbing_isa.txt).  That is also why the CONTROL FLOW around these pieces -- which frames stop, the
// `done` mask, the non-finite veto, iters / conv -- stays in the bodies: wrapped into functions it changed the register allocation
// of the instances (same file).  Device code only, like the body headers (jit.cc embeds this text too).
#pragma once
#include "fused_rows.h"

namespace ldpc {

// Geometry and LDS layout of a workgroup: NP wave groups of VT threads around one block column of V positions (QcGeom), ES bytes
// per lam cell.  LDS = lam (block column after block column, rounded up to 16 bytes), one flag word per wave, then -- the layered
// kernels with rows split between two groups -- an exchange area of EXCHANGE_WORDS x 2 groups x VT dwords that starts at EX0.
// (jit.cc fused_jit_plan restates an upper bound of lds_bytes() on the host side.)
template <class Plan, int SZ, int ES = 4> struct SplitGeom {
    static constexpr int CPW = QcGeom<SZ>::CPW, V = QcGeom<SZ>::V, VT = QcGeom<SZ>::VT, THREADS = Plan::NP * VT, NW = THREADS / 64;
    static constexpr int N = Plan::NBC * SZ, NBCP = (Plan::NBC + Plan::NP - 1) / Plan::NP;   // a frame's columns; block columns a group fills, at most
    static constexpr uint32_t vmask = V * ES - 1;
    static constexpr int LAM_BYTES = (Plan::NBC * V * ES + 15) / 16 * 16;
    static constexpr uint32_t EX0 = LAM_BYTES + 4 * NW + 12, EXW = 2 * VT * 4, EXG = VT * 4;   // exchange area: [word][group][VT]
    static constexpr int lds_bytes(int exchange_words = 0) { return LAM_BYTES + 4 * NW + (exchange_words ? 16 + exchange_words * 2 * VT * 4 : 0); }
    static_assert(THREADS <= 1024, "a frame's wave groups must fit one workgroup");
};

// every wave group runs its own straight-line program (same loop structure, same barriers): f(integral_constant P) in group P
template <class Plan, int VT, class F>
__device__ __forceinline__ void in_own_group(uint32_t tid, F &&f) {
    const uint32_t group = __builtin_amdgcn_readfirstlane(tid / VT);  // wave-uniform (VT is a multiple of 64)
    static_for<0, Plan::NP>([&](auto pc) {
        if (group == (uint32_t)decltype(pc)::value) f(pc);
    });
}

// f(integral_constant bc) for the block columns group P fills: bc % NP == P
template <class Plan, int P, class F>
__device__ __forceinline__ void own_columns(F &&f) {
    static_for<0, Plan::NBC>([&](auto bcc) {
        if constexpr ((decltype(bcc)::value % Plan::NP) == P) f(bcc);
    });
}

// Where a lane is, from its LDS byte offset p inside a block column.  Only p lives across the iteration loop; everything else about
// the lane's place is recomputed from it where needed, so that it does not occupy registers next to the messages.  FPL frames per
// lane: frame0 (+ 1 in the high half of a packed-fp16 word).
template <int ES, int CPW, int N, int FPL> struct Where {
    uint32_t sub, r0; long long frame0; bool valid[FPL]; size_t fN[FPL];
    __device__ __forceinline__ Where(uint32_t p, int batch) {
        asm volatile("" : "+v"(p));            // keep the compiler from carrying these over from an earlier Where
        const uint32_t lane = p / ES;          // position inside the group
        sub = lane % CPW;                      // slot inside the workgroup (slots interleave lane by lane)
        r0 = lane / CPW;                       // circulant row / own column inside a block
        frame0 = ((long long)blockIdx.x * CPW + sub) * FPL;
#pragma unroll   // lanes of a frame past the batch shadow frame 0 and store nothing
        for (int h = 0; h < FPL; h++) { valid[h] = frame0 + h < batch; fN[h] = (size_t)(valid[h] ? frame0 + h : 0) * N; }
    }
};

// Workgroup-wide OR, per frame, of a lane flag: lane_flag(h) for the lane's frame h.  -> bit FPL * s + h = some lane of slot s
// raised it for frame h.  One word per wave into `flags` (a volatile pointer or SynFlags<>), barrier, OR over the NW words.
// BARRIER_AFTER: the flags may be rewritten at once (without it the caller has a barrier before they are written next).
template <int CPW, int NW, int FPL, bool BARRIER_AFTER, class Flags, class LaneFlag>
__device__ __forceinline__ uint32_t frames_with(const Flags &flags, uint32_t tid, LaneFlag lane_flag) {
    uint32_t wbits = 0;
#pragma unroll
    for (int h = 0; h < FPL; h++) {
        const unsigned long long ub = __ballot(lane_flag(h));
#pragma unroll
        for (int s2 = 0; s2 < CPW; s2++) {
            unsigned long long m = 0;
            for (int i = 0; i < 64; i += CPW) m |= 1ull << i;
            wbits |= ((ub & (m << s2)) != 0ull) ? (1u << (FPL * s2 + h)) : 0u;
        }
    }
    if ((tid & 63) == 0) flags[tid >> 6] = wbits;
    __syncthreads();
    uint32_t f = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) f |= flags[w];
    f = __builtin_amdgcn_readfirstlane(f);
    if constexpr (BARRIER_AFTER) __syncthreads();
    return f;
}

// ---- what an LDS word holds for a lam: hard(word, h) and value(word, h) of the lane's frame h, and channel<FMT>(A, gi) = the
// channel LLR gi as the kernel takes it in (the lam of a frame that did not converge)
template <typename CT, bool NEG> struct LamCell {      // lam itself, or 0 - lam (NEG: fused_split_body.h SPLIT_NEG_LAM)
    using word = CT;
    static constexpr int FPL = 1;
    static __device__ __forceinline__ CT stored(CT x) { return NEG ? CT(0) - x : x; }   // lam -> word and back
    static __device__ __forceinline__ bool hard(CT w, int) { return NEG ? w < CT(0) : w > CT(0); }
    static __device__ __forceinline__ double value(CT w, int) { return (double)stored(w); }
    template <int FMT> static __device__ __forceinline__ double channel(const FusedArgs &A, size_t gi) {
        return (double)maybe_round_f16<CT>(load_llr_as<CT, FMT>(A.llr, gi), A.llr_round16);
    }
};
// the f32 cell of the on-chip layered kernel (fused_layered_body.h lay::body): its LDPC_F16 rounding is still the plain saturation
// (ldpc_math.h round_f16_sat: a NaN comes out as -65504) -- that kernel is not under rule 1 and rule 3 of include/ldpc_hip.h yet
struct LamCellLay : LamCell<float, false> {
    template <int FMT> static __device__ __forceinline__ double channel(const FusedArgs &A, size_t gi) {
        const float v = load_llr_as<float, FMT>(A.llr, gi);
        return (double)(A.llr_round16 ? round_f16_sat(v) : v);
    }
};
// NANZ: a NaN channel LLR is taken in as +0, an erasure (include/ldpc_hip.h, non-finite channel LLRs, rule 1): the layered kernel.  The
// flooding kernel (fused_pk16_body.h) still has the plain saturation, under which fmaxf(NaN, -M) = -M makes a NaN the LLR -16384: with
// the erasure form in its prologue that kernel lost 3 % although its turn loop, registers and spills were unchanged (DESIGN.md sections 4, 7).
template <bool NANZ> struct LamCellPk16T {   // two frames: L = -lam as fp16 in the low / high half (fused_pk16_body.h)
    using word = uint32_t;
    static constexpr int FPL = 2;
    static constexpr float LLR16_MAX = 16384.0f;
    // -(x) of a channel LLR as fp16 bits, saturated at +-LLR16_MAX, a zero as +0.  NANZ, without a compare: fmaxf(NaN, -M) = -M and
    // fminf(NaN, M) = M, so the median of {max(x, -M), min(x, M), 0} is 0 for a NaN, x itself inside +-M and +-M outside
    static __device__ __forceinline__ uint32_t neg_llr16(float x) {
        float v;
        if constexpr (NANZ) v = __builtin_amdgcn_fmed3f(fmaxf(x, -LLR16_MAX), fminf(x, LLR16_MAX), 0.0f);
        else v = fminf(fmaxf(x, -LLR16_MAX), LLR16_MAX);
        const _Float16 h = (_Float16)(0.0f - v);          // 0 - (+-0) = +0; the f32 negation is exact, the conversion rounds to nearest even
        uint16_t b;
        __builtin_memcpy(&b, &h, 2);
        return b == 0x8000u ? 0u : (uint32_t)b;           // (a value that underflows to -0 in fp16)
    }
    static __device__ __forceinline__ bool hard(uint32_t w, int h) { return (w >> (15 + 16 * h)) & 1u; }   // lam > 0 = sign bit of L
    static __device__ __forceinline__ double value(uint32_t w, int h) {
        const uint16_t b = (uint16_t)(h ? w >> 16 : w & 0xffffu);
        _Float16 v;
        __builtin_memcpy(&v, &b, 2);
        return -(double)(float)v;
    }
    template <int FMT> static __device__ __forceinline__ double channel(const FusedArgs &A, size_t gi) {
        return value(neg_llr16(load_llr_as<float, FMT>(A.llr, gi)), 0);
    }
};
using LamCellPk16 = LamCellPk16T<true>;
using LamCellPk16Sat = LamCellPk16T<false>;

// The plumbing of wave group P of a workgroup whose lam cells are Cell's.  lds: the workgroup's LDS; p4: the lane's byte offset
// inside a block column; w: where the lane is; h: which of the lane's FPL frames.  FULL: the `done` mask with every frame finished
// (bit FPL * slot + h).
template <class Plan, int SZ, int P, class Cell> struct Frame : SplitGeom<Plan, SZ, sizeof(typename Cell::word)> {
    using G = SplitGeom<Plan, SZ, sizeof(typename Cell::word)>;
    using word = typename Cell::word;
    static constexpr int FPL = Cell::FPL, ES = sizeof(word);
    static constexpr uint32_t FULL = (1u << (FPL * G::CPW)) - 1;
    using W = Where<ES, G::CPW, G::N, FPL>;

    template <int BC> static __device__ __forceinline__ word own(const char *lds, uint32_t p4) { return lds_ld<word>(lds, p4 + (BC * G::V * ES)); }   // the lane's cell of block column BC

    // ---- a frame that stops now by the rule (the lane's frame h): hard(lam) of the lane's own columns into the bits of its result ...
    template <class Bits>
    static __device__ __forceinline__ void hard_bits(const char *lds, uint32_t p4, int h, Bits &bits) {
        own_columns<Plan, P>([&](auto bcc) {
            constexpr int bc = decltype(bcc)::value;
            bits.set(bc / Plan::NP, Cell::hard(own<bc>(lds, p4), h));
        });
    }
    // ... and lam itself, if it is wanted
    static __device__ __forceinline__ void store_lam(const FusedArgs &A, const char *lds, uint32_t p4, const W &w, int h) {
        own_columns<Plan, P>([&](auto bcc) {
            constexpr int bc = decltype(bcc)::value;
            A.final_lam[w.fN[h] + bc * SZ + w.r0] = Cell::value(own<bc>(lds, p4), h);
        });
    }
    // row n of the trace of the lane's frame h
    static __device__ __forceinline__ void trace_frame(const FusedArgs &A, const char *lds, uint32_t p4, const W &w, int h, int n) {
        own_columns<Plan, P>([&](auto bcc) {
            constexpr int bc = decltype(bcc)::value;
            A.trace[((size_t)(w.frame0 + h) * (A.max_iters + 1) + n) * G::N + bc * SZ + w.r0] = Cell::value(own<bc>(lds, p4), h);
        });
    }
    // ---- result of the lane's frame h: hard(lam at convergence) for a frame that stopped by the rule, hard(channel LLR) otherwise
    template <class Res>
    static __device__ __forceinline__ void store_bits(const FusedArgs &A, const W &w, int h, const Res &res) {
        own_columns<Plan, P>([&](auto bcc) {
            constexpr int bc = decltype(bcc)::value;
            A.bits[w.fN[h] + bc * SZ + w.r0] = res.bits.get(bc / Plan::NP);
        });
    }
    // ... the channel LLRs as the lam of a frame that did not converge
    static __device__ __forceinline__ void store_channel_lam(const FusedArgs &A, const W &w, int h) {
        with_llr_format(A.llr_fmt, [&](auto fc) {
            own_columns<Plan, P>([&](auto bcc) {
                constexpr int bc = decltype(bcc)::value;
                const size_t gi = w.fN[h] + bc * SZ + w.r0;
                A.final_lam[gi] = Cell::template channel<decltype(fc)::value>(A, gi);
            });
        });
    }
};

// ---- packed fp16: L <- -(channel LLRs) of the lane's two frames.  Every LLR is read from memory once; the hard decisions of the
// lane's own columns stay in obits[h] (the answer of a frame that runs out of turns).
template <class Plan, int SZ, int P, class Cell = LamCellPk16, class Bits>
__device__ __forceinline__ void load_llrs_pk16(const FusedArgs &A, char *lds, uint32_t p4, Bits (&obits)[2]) {
    using F = Frame<Plan, SZ, P, Cell>;
    const typename F::W w(p4, A.batch);   // (a frame past the batch shadows frame 0: every load below is unconditional and in range)
    with_llr_format(A.llr_fmt, [&](auto fc) {
        constexpr int FMT = decltype(fc)::value;
        float x[F::NBCP][2];          // all of the thread's loads first, back to back: 2 x 22 of them
        own_columns<Plan, P>([&](auto bcc) {
            constexpr int bc = decltype(bcc)::value;
#pragma unroll
            for (int h = 0; h < 2; h++) x[bc / Plan::NP][h] = load_llr_as<float, FMT>(A.llr, w.fN[h] + bc * SZ + w.r0);
        });
        own_columns<Plan, P>([&](auto bcc) {
            constexpr int bc = decltype(bcc)::value;
            uint32_t packed = 0;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const uint32_t b = Cell::neg_llr16(x[bc / Plan::NP][h]);
                obits[h].set(bc / Plan::NP, (b >> 15) & 1u);      // hard(llr) = llr > 0 = sign of -llr
                packed |= b << (16 * h);
            }
            lds_st<uint32_t>(lds, p4 + (bc * F::V * 4), packed);
        });
    });
}

}  // namespace ldpc
