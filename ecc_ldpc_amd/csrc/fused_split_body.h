// fused_split_body.h -- device code of the four-wave "split" fused kernel (see fused_split.hip for the design notes).
// Compiled two ways from this one source: ahead of time for the shipped matrices (fused_split.hip, tables in
// generated_tables.h) and at run time by hiprtc for any other single-circulant quasi-cyclic H (jit.cc: plan and
// rotation table generated as constexpr structs from the code's description) -- so it includes nothing host-side.
// The ahead-of-time f32 min-sum instances with whole waves of one frame (sz = 128) are built in a tighter form behind
// SPLIT_WAVE_SPEC, SPLIT_FLAGS_LDS, SPLIT_NEG_LAM, SPLIT_SYN_SKIP and SPLIT_STORE_ADDTID below; all default to off here, so a run-time compiled instance
// and the sz = 32 instances compile to what they were.
// What is not about check rows or column rounds -- LDS layout, lane locator, per-frame workgroup OR, the stores of trace rows,
// snapshots and results -- is shared with the packed-fp16 and the layered bodies: fused_frame.h.
#pragma once
#include "fused_frame.h"   // (brings fused_rows.h)

#ifndef SPLIT_ORIG_REGS
#define SPLIT_ORIG_REGS 1
#endif
// round-0 channel-LLR copies of the f32 min-sum instances with sz >= 64 that live in a lane-private LDS area instead of VGPRs
// (the first SPLIT_ORIG_LDS slots; the rest stay in registers).  fused_split.hip sets it for its ahead-of-time instances;
// run-time compiled instances keep every copy in registers.
#ifndef SPLIT_ORIG_LDS
#define SPLIT_ORIG_LDS 0
#endif
// One straight-line program per WAVE of a group instead of one per group (f32 min-sum, whole waves of one frame, more than one
// wave per group): the wave's index inside its group becomes a compile-time constant, and with it which edges can wrap around
// their circulant in that wave (fused_rows.h WaveRot): for every rotation at least one of a group's two waves adds no wrap
// arithmetic, only an immediate.  fused_split.hip sets it for its ahead-of-time instances; run-time compiled instances keep one
// program per group.
#ifndef SPLIT_WAVE_SPEC
#define SPLIT_WAVE_SPEC 0
#endif
// which phases address by the wave's own rotations when SPLIT_WAVE_SPEC is on: bit 0 = phase A (check rows), bit 1 = phase B
// (column rounds).  The other phase keeps the thread's offset inside its pair and the plain rotations.
#ifndef SPLIT_WAVE_PHASES
#define SPLIT_WAVE_PHASES 3
#endif
// the per-wave syndrome words read and written as LDS (address space 3) accesses instead of through a generic volatile pointer,
// whose loads go down the flat path and count against vmcnt as well as lgkmcnt right behind the barrier (same instances)
#ifndef SPLIT_FLAGS_LDS
#define SPLIT_FLAGS_LDS 0
#endif
// lam kept NEGATED in LDS, L = 0 - lam with an exact zero always as +0 (same instances): the syndrome becomes the XOR of the
// gathered words' sign bits (fused_rows.h rows_a NEG).  Phase B subtracts, L' = L - ne'; whatever leaves the kernel as lam
// (final_lam, trace) or enters it (channel LLRs, a given lam) is negated on the way.
#ifndef SPLIT_NEG_LAM
#define SPLIT_NEG_LAM 0
#endif
// Syndrome skip (same instances; one wave = one frame): K > 0 = after the first K of its group's block rows a wave asks, with one
// ballot, whether any of its lanes has seen an unsatisfied row.  If so its share of the frame's OR "some row is unsatisfied" is
// settled, and the group's other rows of this turn branch around their parity chains (fused_rows.h rows_a MAY_SKIP): exact,
// because that OR is the parities' only use.  If not, the other rows run as before.  0 = off.
#ifndef SPLIT_SYN_SKIP
#define SPLIT_SYN_SKIP 0
#endif
// Phase B's stores of edges that cannot wrap in their wave as ds_write_addtid_b32 (same instances; needs SPLIT_WAVE_SPEC): the
// cell of such an edge is lane * 4 + a constant, which that instruction addresses as M0[15:0] + 16-bit offset + 4 * lane with no
// address VGPR -- the store's transfer to LDS is then one source dword instead of two.  The reads keep their form whatever
// SPLIT_WAVE_PHASES says; only the store is decided by the wave's own rotations (fused_rows.h WaveRot).  The instruction sits in
// inline assembly, which the compiler's wait-count pass does not see: split_body waits for lgkmcnt(0) itself before the barrier
// of every round.  Bits: 1 = in the read-add-write rounds (q >= 1), 2 = in round 0 (lam = msg + channel LLR: no read, so the
// edge's address arithmetic goes with the register), 0 = off.  4 = timing only, results WRONG: the wrapping edges too (each lands
// in a cell of its block column that is not its own) -- the upper bound of what 3 can give, tools/build_ablation.sh.
#ifndef SPLIT_STORE_ADDTID
#define SPLIT_STORE_ADDTID 0
#endif
// wave priority while in phase A (check rows: long stretches of independent VALU work) and in phase B (column
// rounds: short, LDS-bound, barrier-separated).  Measured on jpl.4096, 65 536 frames: A=0/B=0 20.72 ms,
// A=0/B=2 20.90, A=2/B=0 20.24 (A = 1, 2 or 3 alike).  The priority is raised after the first phase B only:
// a workgroup that starts (global loads, first syndrome) at high priority costs 0.1-0.2 ms.
#ifndef SPLIT_PRIO_A
#define SPLIT_PRIO_A 2
#endif
#ifndef SPLIT_PRIO_B
#define SPLIT_PRIO_B 0
#endif
// edges per read-add-write batch inside a column round (2 registers per edge in flight).  Measured on jpl.4096,
// 65 536 frames: 4: 20.66 ms, 6: 20.15, 8: 20.01, 10: 19.50, 11: 19.36, 12: 19.29, 14: 19.42, 16: 19.57, 24: 19.47.
#ifndef SPLIT_CH
#define SPLIT_CH 12
#endif
// sz = 32 (two frames per workgroup, one wave per pair): jpl.1024 4.80 ms at 12, 4.76 at 16, 4.68 at 24
#ifndef SPLIT_CH_SMALL
#define SPLIT_CH_SMALL 24
#endif

namespace ldpc {

// the instances SPLIT_WAVE_SPEC and SPLIT_FLAGS_LDS apply to: f32 min-sum, one frame per workgroup in whole waves, several waves per group
template <typename CT, int VARIANT, int SZ>
constexpr bool kSplitWholeWaves = VARIANT == LDPC_V_MINSUM && sizeof(CT) == 4 && QcGeom<SZ>::CPW == 1 && QcGeom<SZ>::VT == QcGeom<SZ>::V && QcGeom<SZ>::VT > 64;
// the syndrome words of a workgroup, one per wave.  volatile either way: they are rewritten behind every barrier.
template <bool LDS_AS> struct SynFlags;
template <> struct SynFlags<false> {
    volatile uint32_t *p;
    __device__ __forceinline__ explicit SynFlags(char *at) : p(reinterpret_cast<volatile uint32_t *>(at)) {}
    __device__ __forceinline__ volatile uint32_t &operator[](uint32_t w) const { return p[w]; }
};
template <> struct SynFlags<true> {
    typedef __attribute__((address_space(3))) volatile uint32_t *ptr_t;
    ptr_t p;
    __device__ __forceinline__ explicit SynFlags(char *at) : p((ptr_t)at) {}
    __device__ __forceinline__ __attribute__((address_space(3))) volatile uint32_t &operator[](uint32_t w) const { return p[w]; }
};

// hard bits of the block columns a lane's group fills, NB of them
#ifndef SPLIT_RESULT_PACKED
#define SPLIT_RESULT_PACKED 1   // run-time compiled instances set 0: no limit on max_iters
#endif
template <int NB, bool PACKED = (SPLIT_RESULT_PACKED && NB <= 22)> struct SplitResult;
template <int NB> struct SplitResult<NB, true> {
    struct Bits {
        uint32_t w = 0;
        __device__ __forceinline__ void set(int i, bool b) { w |= (b ? 1u : 0u) << i; }
        __device__ __forceinline__ uint32_t get(int i) const { return (w >> i) & 1u; }
    } bits;
    __device__ __forceinline__ void converge_at(int n) { bits.w = (1u << 22) | ((uint32_t)n << 23); }
    __device__ __forceinline__ bool converged() const { return (bits.w >> 22) & 1u; }
    __device__ __forceinline__ int turn() const { return (int)(bits.w >> 23); }
};
template <int NB> struct SplitResult<NB, false> {
    struct Bits {
        uint32_t w[(NB + 31) / 32] = {};
        __device__ __forceinline__ void set(int i, bool b) { w[i >> 5] |= (b ? 1u : 0u) << (i & 31); }
        __device__ __forceinline__ uint32_t get(int i) const { return (w[i >> 5] >> (i & 31)) & 1u; }
    } bits;
    uint32_t flag = 0;   // bit 31: converged; low bits: the turn
    __device__ __forceinline__ void converge_at(int n) { bits = Bits{}; flag = 0x80000000u | (uint32_t)n; }
    __device__ __forceinline__ bool converged() const { return flag >> 31; }
    __device__ __forceinline__ int turn() const { return (int)(flag & 0x7fffffffu); }
};

// ownership and per-pair register slots, all compile time
template <class Plan, class T>
struct Split {
    static constexpr int br_of(int e) {
        int br = 0;
        for (int b = 0; b < Plan::NBR; b++) if (Plan::ebeg(b) <= e) br = b;
        return br;
    }
    static constexpr int owner_br(int br) { return Plan::owner_br(br); }
    static constexpr int owner(int e) { return owner_br(br_of(e)); }
    static constexpr int own_index(int br) {  // index of block row br among its owner's block rows, plan order
        int c = 0;
        for (int b = 0; b < br; b++) c += owner_br(b) == owner_br(br) ? 1 : 0;
        return c;
    }
    static constexpr int slot(int e) {  // index of e among its owner's edges, plan order
        int c = 0;
        for (int j = 0; j < e; j++) c += owner(j) == owner(e) ? 1 : 0;
        return c;
    }
    static constexpr int nmsg(int p) {
        int c = 0;
        for (int e = 0; e < T::NEDGE; e++) c += owner(e) == p ? 1 : 0;
        return c;
    }
    static constexpr int max_over_groups(int (*f)(int)) { int m = 0; for (int g = 0; g < Plan::NP; g++) m = f(g) > m ? f(g) : m; return m; }
    static constexpr int NMSG = max_over_groups(nmsg);
    // channel LLR of the column a thread writes in round 0 of block column bc: held by the owner of that edge
    static constexpr int oowner(int bc) { return owner(Rounds<T>::round0_edge(bc)); }
    static constexpr int oslot(int bc) {
        int c = 0;
        for (int j = 0; j < bc; j++) c += oowner(j) == oowner(bc) ? 1 : 0;
        return c;
    }
    static constexpr int norig(int p) {
        int c = 0;
        for (int bc = 0; bc < T::NBC; bc++) c += oowner(bc) == p ? 1 : 0;
        return c;
    }
    static constexpr int NORIG = max_over_groups(norig);
    // edges of round q owned by pair p, highest edge index first
    static constexpr int count(int q, int p) {
        int c = 0;
        for (int e = 0; e < T::NEDGE; e++) c += (Rounds<T>::round_of(e) == q && owner(e) == p) ? 1 : 0;
        return c;
    }
    static constexpr int nth(int q, int p, int i) {
        int c = 0;
        for (int e = T::NEDGE - 1; e >= 0; e--)
            if (Rounds<T>::round_of(e) == q && owner(e) == p) { if (c == i) return e; c++; }
        return -1;
    }
};

// LDS of a workgroup: lam (block column after block column), one syndrome word per wave, then NOL slots of round-0 LLR copies,
// slot-major and one word per thread (lane-private: written and read by the same thread only, conflict-free, no barrier)
template <typename CT, int VARIANT, class Plan, int SZ, class T>
struct SplitLds {
    static constexpr int V = QcGeom<SZ>::V, VT = QcGeom<SZ>::VT, THREADS = Plan::NP * VT, NW = THREADS / 64, ES = sizeof(CT);
    static constexpr int LAM_BYTES = SplitGeom<Plan, SZ, ES>::LAM_BYTES;
    static constexpr int ORIG_OFF = LAM_BYTES + (4 * NW + 15) / 16 * 16;
    static constexpr int NOL_WANT = (VARIANT == LDPC_V_MINSUM && ES == 4 && SZ >= 64 && SPLIT_ORIG_REGS) ? SPLIT_ORIG_LDS : 0;
    static constexpr int NOL = NOL_WANT < Split<Plan, T>::NORIG ? NOL_WANT : Split<Plan, T>::NORIG;
    static constexpr int BYTES = NOL ? ORIG_OFF + NOL * THREADS * ES : SplitGeom<Plan, SZ, ES>::lds_bytes();
    // byte offset of slot os of the thread in group P at lane offset p4 (= its lane index * ES): an immediate + p4
    static constexpr uint32_t orig_at(int P, int os) { return ORIG_OFF + (uint32_t)(os * THREADS + P * VT) * ES; }
};

// b4: the address base of the thread -- its byte offset inside a block column (WV < 0), or its LANE's, with the wave's rows
// folded into the rotations (WV = the wave inside the group, WaveRot).  An edge that cannot wrap is base + immediate and
// holds no address register; the fence keeps the wrapped addresses of the others from being hoisted out of the turn loop.
// WVS >= 0 (SPLIT_STORE_ADDTID): the program's wave inside the group whatever WV says, for the stores alone -- an edge that
// cannot wrap in that wave is stored by lane id (split_store_addtid), and its address register dies with the read.
// M0_TOO: the chunk's first such store, which also sets M0 to the LDS address of the workgroup's array.  One wait state between the
// scalar write of M0 and the DS instruction that reads it (without it the instruction takes the old M0): the compiler does not look
// into inline assembly, so the s_nop is written here, and ecc_ldpc_amd/build.py checks that nothing else in the kernel writes M0.
template <int OFF, bool M0_TOO>
__device__ __forceinline__ void split_store_addtid(float v, uint32_t lds_base) {
    static_assert(OFF >= 0 && OFF < 65536, "16-bit offset field");
    if constexpr (M0_TOO) asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tds_write_addtid_b32 %0 offset:%2" ::"v"(v), "s"(lds_base), "n"(OFF) : "memory");
    else asm volatile("ds_write_addtid_b32 %0 offset:%1" ::"v"(v), "n"(OFF) : "memory");
}
template <typename CT, int VARIANT, int SZ, class Plan, class T, int P, int WV, int WVS, int Q, int I0, int I1>
__device__ __forceinline__ void split_round_chunk(char *lds, const uint32_t b4, uint32_t vmask, const CT *msg, const CT *orig_rot, const float *gllr, uint32_t r0) {
    using S = Split<Plan, T>;
    using L = SplitLds<CT, VARIANT, Plan, SZ, T>;
    using R = WaveRot<SZ, WV>;
    using RS = WaveRot<SZ, WVS>;
    constexpr uint32_t ES = sizeof(CT), V = QcGeom<SZ>::V;
    constexpr uint32_t WOFF = WV < 0 ? 0 : WV * 64 * ES;   // own position inside a block column = b4 + WOFF
    constexpr bool NEG = SPLIT_NEG_LAM && kSplitWholeWaves<CT, VARIANT, SZ>;   // LDS (lam and the round-0 copies) holds 0 - lam
    constexpr bool FENCE = [] {
        for (int i = I0; i < I1; i++) if (!R::nowrap(T::rot[S::nth(Q, P, i)])) return true;
        return false;
    }();
    uint32_t p4 = b4;
    if constexpr (FENCE) asm volatile("" : "+v"(p4));
    auto pos = [&](auto ec) -> uint32_t {   // position of edge e inside its block column
        constexpr uint32_t rot = T::rot[decltype(ec)::value];
        if constexpr (R::nowrap(rot)) return b4 + R::rot(rot) * ES; else return qc_wrap(p4 + R::rot(rot) * ES, vmask);
    };
    // the store of edge e: by lane id where the program's wave cannot wrap it, else to `at()` (= pos(e))
    constexpr auto by_lane = [](int e) { return WVS >= 0 && ((SPLIT_STORE_ADDTID & (Q == 0 ? 2 : 1)) != 0) && ((SPLIT_STORE_ADDTID & 4) != 0 || RS::nowrap(T::rot[e])); };
    constexpr int FIRST = [by_lane] {   // the chunk's first store by lane id
        for (int i = I0; i < I1; i++) if (by_lane(S::nth(Q, P, i))) return i;
        return -1;
    }();
    auto put = [&](auto ic, auto at, CT v) {
        constexpr int i = decltype(ic)::value, e = S::nth(Q, P, i);
        if constexpr (by_lane(e)) {
            constexpr uint32_t s = RS::nowrap(T::rot[e]) ? RS::rot(T::rot[e]) : RS::rot(T::rot[e]) % 64;   // (% 64: the timing-only form, a cell of the same column)
            static_assert(s + 63 < V && (T::bc[e] + 1) * V * ES <= (uint32_t)L::LAM_BYTES, "inside the block column, inside lam");
            split_store_addtid<(int)(T::bc[e] * V * ES + s * ES), i == FIRST>(v, (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)lds);
        } else {
            lds_st<CT>(lds + T::bc[e] * V * ES, at(), v);
        }
    };
    if constexpr (Q == 0) {
        static_for<I0, I1>([&](auto ic) {
            // (constexpr VARIABLES: a constexpr function call in a subscript is not a constant expression and was
            //  left as a run-time loop, which kept msg[] in scratch memory)
            constexpr int e = S::nth(Q, P, decltype(ic)::value);
            constexpr int ms = S::slot(e), os = S::oslot(T::bc[e]);
            CT o;
            if constexpr (SPLIT_ORIG_REGS && os < L::NOL) o = lds_ld<CT>(lds + L::orig_at(P, os) + WOFF, b4);
            else if constexpr (SPLIT_ORIG_REGS) o = orig_rot[os]; else o = (CT)gllr[T::bc[e] * SZ + ((r0 + T::rot[e]) % SZ)];
            put(ic, [&] { return pos(std::integral_constant<int, e>{}); }, NEG ? o - msg[ms] : msg[ms] + o);
        });
        return;
    }
    CT cur[I1 - I0];
    uint32_t adr[I1 - I0];
    static_for<I0, I1>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        constexpr int e = S::nth(Q, P, i);
        adr[i - I0] = pos(std::integral_constant<int, e>{});
        cur[i - I0] = lds_ld<CT>(lds + T::bc[e] * V * ES, adr[i - I0]);
    });
    static_for<I0, I1>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        constexpr int e = S::nth(Q, P, i);
        constexpr int ms = S::slot(e);
        put(ic, [&] { return adr[i - I0]; }, NEG ? cur[i - I0] - msg[ms] : msg[ms] + cur[i - I0]);
    });
    asm volatile("" ::: "memory");
}
template <typename CT, int VARIANT, int SZ, class Plan, class T, int P, int WV, int WVS, int Q, int I0>
__device__ __forceinline__ void split_round(char *lds, uint32_t p4, uint32_t vmask, const CT *msg, const CT *orig_rot, const float *gllr, uint32_t r0) {
    constexpr int CNT = Split<Plan, T>::count(Q, P), CH = SZ < 64 ? SPLIT_CH_SMALL : SPLIT_CH;
    if constexpr (I0 < CNT) {
        split_round_chunk<CT, VARIANT, SZ, Plan, T, P, WV, WVS, Q, I0, (I0 + CH < CNT ? I0 + CH : CNT)>(lds, p4, vmask, msg, orig_rot, gllr, r0);
        split_round<CT, VARIANT, SZ, Plan, T, P, WV, WVS, Q, I0 + CH>(lds, p4, vmask, msg, orig_rot, gllr, r0);
    }
}

// The whole decode of one pair: P is a compile-time constant, so every ownership test below is resolved
// at compile time and the two pairs are two independent straight-line programs (one wave-uniform branch
// in the kernel).  WV >= 0: the program of wave WV of the pair alone (SPLIT_WAVE_SPEC); the register that lives
// across the loop is then the LANE's offset b4, and the thread's own position p4 = b4 + an immediate.
// Keeping them as separate regions matters for the register allocator: with both pairs'
// code merged in one loop body the 105 loop-carried registers met in phi nodes at every branch merge and
// were spilled wholesale.
template <typename CT, int VARIANT, class Plan, int SZ, class T, int P, int WV>
__device__ __forceinline__ void split_body(const FusedArgs &A, char *lds, const uint32_t tid) {
    using S = Split<Plan, T>;
    // what LDS holds for a lam (and for a channel LLR among the round-0 copies), and back: lam itself, or 0 - lam (SPLIT_NEG_LAM)
    constexpr bool NEG = SPLIT_NEG_LAM && kSplitWholeWaves<CT, VARIANT, SZ>;
    using Cell = LamCell<CT, NEG>;
    using F = Frame<Plan, SZ, P, Cell>;
    using Where = typename F::W;
    constexpr int CPW = F::CPW, V = F::V, VT = F::VT, NW = F::NW;  // frames per workgroup, positions per block column, threads per group, waves
    constexpr uint32_t ES = sizeof(CT), vmask = F::vmask, FULL = F::FULL;
    // Only p4 (the lane's LDS byte offset inside a block column) lives across the iteration loop; everything else
    // about the lane's place -- frame, row, global offsets -- is recomputed from it where needed (Where), so that
    // it does not occupy registers next to the messages.
    if constexpr (VT != V) { if ((tid % VT) >= (uint32_t)V) return; }   // circulant size not a multiple of 64: the top lanes of the group idle
    const uint32_t b4 = (tid % (WV < 0 ? VT : 64)) * ES;
    const uint32_t p4 = b4 + (WV < 0 ? 0 : WV * 64) * ES;
    constexpr int WVA = (SPLIT_WAVE_PHASES & 1) ? WV : -1, WVB = (SPLIT_WAVE_PHASES & 2) ? WV : -1;   // per phase: specialised or not
    constexpr int WVS = (SPLIT_STORE_ADDTID && kSplitWholeWaves<CT, VARIANT, SZ>) ? WV : -1;   // phase B's stores by lane id where this wave cannot wrap
    auto fE_of = [](const Where &w) { return (size_t)(w.valid[0] ? w.frame0 : 0) * Plan::NEDGE * SZ; };   // the frame's messages (step mode)
    const Where w0(p4, A.batch);
    const uint32_t r0 = w0.r0;
    const size_t fN = w0.fN[0], fE = fE_of(w0);
    // ---- messages (own block rows) and round-0 channel LLRs (own round-0 edges)
    CT msg[S::NMSG];
    CT orig[SPLIT_ORIG_REGS ? S::NORIG : 1];
#pragma unroll
    for (int i = 0; i < S::NMSG; i++) msg[i] = CT(0);  // Orig.hs:64-65
#pragma unroll
    for (int i = 0; i < (SPLIT_ORIG_REGS ? S::NORIG : 1); i++) orig[i] = CT(0);
    using L = SplitLds<CT, VARIANT, Plan, SZ, T>;
    static_assert(L::NOL == 0 || L::BYTES <= 65536, "LDS of one workgroup");
    auto put_orig = [&](int os, CT v) {   // (os is a constant after inlining)
        if (os < L::NOL) lds_st<CT>(lds + L::orig_at(P, os), p4, v); else orig[os] = v;
    };
    // ---- lam <- LLRs (or the given lam): pair P fills the block columns bc with bc % 2 == P.  One dispatch on the
    // LLR element type around ALL of the thread's loads (46 of them): they issue back to back.
    // Every channel LLR is read from global memory ONCE (the input may be page-locked HOST memory read over PCIe,
    // api.cc zero-copy path): the hard decisions of the thread's own columns are kept in `obits` -- the answer of a
    // frame that runs out of turns (Orig.hs:70) -- and the rotated copies phase B wants come out of LDS below.
    typename SplitResult<(Plan::NBC + Plan::NP - 1) / Plan::NP>::Bits obits{};
    with_llr_format(A.llr_fmt, [&](auto fc) {
        constexpr int FMT = decltype(fc)::value;
        own_columns<Plan, P>([&](auto bcc) {
            constexpr int bc = decltype(bcc)::value;
            CT v = maybe_round_f16<CT>(load_llr_as<CT, FMT>(A.llr, fN + bc * SZ + r0), A.llr_round16);
            obits.set(bc / Plan::NP, v > CT(0));
            if (A.step_mode) v = (CT)A.st_lam[fN + bc * SZ + r0];
            lds_st<CT>(lds, p4 + (bc * V * ES), Cell::stored(v));
        });
        if (A.step_mode) {   // teacher-forced step: LDS holds the given lam, the channel LLRs come from memory
            static_for<0, Plan::NBC>([&](auto bcc) {
                constexpr int bc = decltype(bcc)::value;
                if constexpr (SPLIT_ORIG_REGS && S::oowner(bc) == P) {
                    constexpr int e0 = Rounds<T>::round0_edge(bc);
                    constexpr int os = S::oslot(bc);
                    put_orig(os, Cell::stored(maybe_round_f16<CT>(load_llr_as<CT, FMT>(A.llr, fN + bc * SZ + ((r0 + T::rot[e0]) % SZ)), A.llr_round16)));
                }
            });
        }
    });
    if (A.step_mode) {
        static_for<0, Plan::NBR>([&](auto brc) {
            constexpr int br = decltype(brc)::value;
            if constexpr (S::owner_br(br) == P) {
                constexpr int D = Plan::deg(br);
                static_for<0, D>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    constexpr int ms = S::slot(Plan::ebeg(br) + k);
                    msg[ms] = (CT)A.st_ne_in[fE + (size_t)SZ * Plan::ebeg(br) + (size_t)D * r0 + k];
                });
            }
        });
    }
    __syncthreads();
    if (!A.step_mode) {   // lam == channel LLRs right now: the round-0 (rotated) copies are an LDS gather away
        static_for<0, Plan::NBC>([&](auto bcc) {
            constexpr int bc = decltype(bcc)::value;
            if constexpr (SPLIT_ORIG_REGS && S::oowner(bc) == P) {
                constexpr int e0 = Rounds<T>::round0_edge(bc);
                constexpr int os = S::oslot(bc);
                put_orig(os, lds_ld<CT>(lds + bc * V * ES, qc_wrap(p4 + T::rot[e0] * CPW * ES, vmask)));
            }
        });
    }

    const SynFlags<SPLIT_FLAGS_LDS && kSplitWholeWaves<CT, VARIANT, SZ>> flags(lds + F::LAM_BYTES);
    // done: bit s = frame s of this workgroup has finished.  Workgroup-uniform (derived from the shared flags), so
    // loop control and barriers stay uniform with several frames.  A finished frame keeps its answer in `snap`;
    // its lanes then keep computing on their own (disjoint) LDS columns until the workgroup's other frames are
    // done -- masking them off instead makes every message register live across divergent control flow.
    uint32_t done = 0;
#pragma unroll
    for (int s2 = 0; s2 < CPW; s2++) done |= ((long long)blockIdx.x * CPW + s2 < A.batch) ? 0u : (1u << s2);
    // Result of the lane's frame: one hard bit per block column the lane's group fills (NBCP of them) + converged flag
    // + the turn it converged at.  Packed into ONE register when it fits (NBCP <= 22: bits 0..21 hard bits, bit 22
    // converged, bits 23..31 the turn -- max_iters <= kSplitMaxIters, the host checks), else bits and flag/turn apart.
    SplitResult<(Plan::NBC + Plan::NP - 1) / Plan::NP> res;
    res.bits = obits;       // until the frame converges: the hard decisions of its channel LLRs (flag clear)
    const int turns = A.step_mode ? 1 : A.max_iters;

    for (int n = 0;; n++) {
        if (done == FULL) break;
        if (A.trace && !((done >> ((p4 / ES) % CPW)) & 1u)) {
            LDPC_COLD_PATH();
            const Where w(p4, A.batch);
            F::trace_frame(A, lds, p4, w, 0, n);
        }
        const bool last = (n >= turns);
        // ---- phase A over the pair's block rows
        bool unsat = false;
        // Syndrome skip: one wave is one frame here, and all a frame takes from its rows' parities is the OR over its waves' lanes.  A
        // wave in which some lane has seen an unsatisfied row among the group's first SKIP rows has settled its share of that OR:
        // its other rows of this turn branch around their XOR chains (rows_a `settled`; one scalar branch per row, if-then only --
        // an if-else over the rows is linearised by the structurizer into "if (c) A; if (!c) B", with both arms' messages live at once).
        // The parity blocks are an ordinary turn's work too, not a cold path: a wave runs them whenever its first rows hold.
        constexpr int SKIP = (NEG && CPW == 1) ? SPLIT_SYN_SKIP : 0;
        bool settled = false;   // wave-uniform
        static_for<0, Plan::NBR>([&](auto brc) {
            constexpr int br = decltype(brc)::value;
            if constexpr (S::owner_br(br) == P) {
                constexpr int D = Plan::deg(br), ms0 = S::slot(Plan::ebeg(br));
                StatRowW<CT, SZ, T, Plan::ebeg(br), WVA> row;
                if constexpr (SKIP > 0 && S::own_index(br) == SKIP) settled = !last && __ballot(unsat) != 0ull;
                if (last) unsat |= rows_a<CT, VARIANT, D, 1, 0, true, NEG>(lds, row, WVA < 0 ? p4 : b4, vmask, (CT *)nullptr);
                else unsat |= rows_a<CT, VARIANT, D, 1, 0, false, NEG, (SKIP > 0 && S::own_index(br) >= SKIP)>(lds, row, WVA < 0 ? p4 : b4, vmask, &msg[ms0], settled);
            }
        });
        // per wave: bit s = some lane of frame s saw an odd row parity (frames interleave lane by lane)
        // the barrier inside (syndrome OR over the workgroup's waves) also fences phase A reads from phase B writes
        const uint32_t fbits = frames_with<CPW, NW, 1, false>(flags, tid, [&](int) { return unsat; });
        if (A.step_mode) {
            const Where w(p4, A.batch);
            if (w.valid[0] && w.r0 == 0 && P == 0) A.st_syn[w.frame0] = ((fbits >> w.sub) & 1u) ? 0 : 1;
        } else {
            uint32_t newly = ~fbits & ~done & FULL;  // Orig.hs:69: frames whose syndrome is zero now
            if constexpr (kVetoesNonFinite<CT, VARIANT>) {
                if (newly != 0u) {   // (workgroup-uniform, once per frame) LLRs that left the float range: failed, not "converged" (ldpc_math.h)
                    LDPC_COLD_PATH();
                    bool nf = false;
                    if ((newly >> ((p4 / ES) % CPW)) & 1u)
                        own_columns<Plan, P>([&](auto bcc) {
                            constexpr int bc = decltype(bcc)::value;
                            nf |= not_finite(lds_ld<CT>(lds, p4 + (bc * V * ES)));
                        });
                    __syncthreads();   // every wave has read the syndrome flags
                    // (written out: frames_with<CPW, NW, 1, true> here reorders the LDS reads above in the wave-specialised instance)
                    const unsigned long long vb = __ballot(nf);
                    uint32_t vbits = 0;
#pragma unroll
                    for (int s2 = 0; s2 < CPW; s2++) {
                        unsigned long long m = 0;
                        for (int i = 0; i < 64; i += CPW) m |= 1ull << i;
                        vbits |= ((vb & (m << s2)) != 0ull) ? (1u << s2) : 0u;
                    }
                    if ((tid & 63) == 0) flags[tid >> 6] = vbits;
                    __syncthreads();
                    uint32_t veto = 0;
#pragma unroll
                    for (int w = 0; w < NW; w++) veto |= flags[w];
                    veto = __builtin_amdgcn_readfirstlane(veto) & newly;
                    __syncthreads();   // (the flags are rewritten by the next turn's syndrome)
                    done |= veto;      // stops here as a failure: `res` keeps the channel's hard decisions and a clear flag
                    newly &= ~veto;
                }
            }
            if ((newly >> ((p4 / ES) % CPW)) & 1u) {
                LDPC_COLD_PATH();   // once per frame
                res.converge_at(n);
                F::hard_bits(lds, p4, 0, res.bits);
                if (A.final_lam) {
                    const Where w(p4, A.batch);
                    F::store_lam(A, lds, p4, w, 0);
                }
            }
            done |= newly;
            // the snapshot read columns that the OTHER pair rewrites in round 0 when the workgroup goes on
            if (CPW > 1 && newly != 0u && done != FULL) __syncthreads();
        }
        if (last) break;  // Orig.hs:70
        if (done != FULL) {
            __builtin_amdgcn_s_setprio(SPLIT_PRIO_B);
            static_for<0, Rounds<T>::num_rounds()>([&](auto qc) {
                split_round<CT, VARIANT, SZ, Plan, T, P, WVB, WVS, decltype(qc)::value, 0>(lds, WVB < 0 ? p4 : b4, vmask, msg, orig, reinterpret_cast<const float *>(A.llr) + fN, r0);
                // stores by lane id are inline assembly, which the compiler's wait counts do not include: every one has landed before the barrier
                if constexpr (WVS >= 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __syncthreads();  // the next round adds into the same columns
            });
            __builtin_amdgcn_s_setprio(SPLIT_PRIO_A);
        }
        if (A.step_mode) break;
    }

    const Where w(p4, A.batch);
    if (!w.valid[0]) return;
    if (A.step_mode) {
        F::store_lam(A, lds, p4, w, 0);
        static_for<0, Plan::NBR>([&](auto brc) {
            constexpr int br = decltype(brc)::value;
            if constexpr (S::owner_br(br) == P) {
                constexpr int D = Plan::deg(br);
                static_for<0, D>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    constexpr int ms = S::slot(Plan::ebeg(br) + k);
                    A.st_ne_out[fE_of(w) + (size_t)SZ * Plan::ebeg(br) + (size_t)D * w.r0 + k] = (double)msg[ms];
                });
            }
        });
        return;
    }
    // ---- result: hard(lam at convergence) for a converged frame, hard(channel LLR) otherwise (Orig.hs:59,69-70)
    const bool converged = res.converged();
    if (converged) {
        F::store_bits(A, w, 0, res);
    } else {
        F::store_bits(A, w, 0, res);   // hard(channel LLR)
        if (A.final_lam) F::store_channel_lam(A, w, 0);
    }
    if (w.r0 == 0 && P == 0) {
        if (A.iters) A.iters[w.frame0] = converged ? res.turn() : turns;
        if (A.conv) A.conv[w.frame0] = converged ? 1 : 0;
    }
}

// the kernel proper: every wave group runs its own straight-line program (same loop structure, same barriers)
template <typename CT, int VARIANT, class Plan, int SZ, class T>
__device__ __forceinline__ void split_kernel_body(const FusedArgs &A) {
    using G = SplitGeom<Plan, SZ>;
    static_assert(SZ >= 2, "circulant size");
    __shared__ __attribute__((aligned(16))) char lds[SplitLds<CT, VARIANT, Plan, SZ, T>::BYTES];
    const uint32_t tid = threadIdx.x;
    constexpr int WPG = G::VT / 64;   // waves per group
    if constexpr (SPLIT_WAVE_SPEC && kSplitWholeWaves<CT, VARIANT, SZ>) {
        const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / 64);
        static_for<0, Plan::NP * WPG>([&](auto wc) {
            constexpr int P = decltype(wc)::value / WPG, WV = decltype(wc)::value % WPG;
            if (wave == (uint32_t)decltype(wc)::value) split_body<CT, VARIANT, Plan, SZ, T, P, WV>(A, lds, tid);
        });
    } else {
        in_own_group<Plan, G::VT>(tid, [&](auto pc) { split_body<CT, VARIANT, Plan, SZ, T, decltype(pc)::value, -1>(A, lds, tid); });
    }
}

}  // namespace ldpc
