// layered_csr_body.h -- the body of layered_csr_kernel (layered_csr.hip), as TEXT: that file includes it three times, once into
// layered_csr_kernel with LAYERED_CSR_SOFT 0 and once into layered_csr_soft_kernel with LAYERED_CSR_SOFT 1, where the frame's epilogue also
// writes the soft output S (ldpc_decode_batch_dev_soft).  Text and not a function template, so that the eighteen instances without a
// soft output are compiled from exactly what they were compiled from before the soft output existed: they are instruction for instruction
// and register for register what they were.  No include guard.  In scope: DCLASS, CELL, g, rec_all, A, and (soft) S.
// A third inclusion, with LAYERED_CSR_CONT 1 (and LAYERED_CSR_SOFT 1), is layered_csr_cont_kernel (ldpc_decode_batch_dev_continue): the frame's
// records are those of its slot of a decode state (K.rec; no rec_all), the prologue adds the slot's sum of check messages K.sum to the channel
// LLRs, every sweep reads its records, the epilogue writes the new sum for every frame and the soft output only when S.out is not null.
// The other two inclusions define LAYERED_CSR_CONT as 0: their preprocessed text is what it was.  In scope there: K, and no rec_all.
    typedef typename CellOf<CELL>::type LT;
    constexpr int RULE = CellOf<CELL>::rule;          // the 3/4, the rule of A.rule, or the A-min* row (which reads no argument)
    CsrRule rule{};
    if constexpr (RULE == kRuleScaled) rule = A.rule;
    typedef typename Cell<LT>::vec8 cell8;
    typedef typename Cell<LT>::Rec Rec;               // the row record follows the lam cell: 12 bytes (fp16, f32), 8 bytes (int8)
    constexpr bool kInt8 = std::is_same<LT, int8_t>::value;
    constexpr bool kVeto = kVetoesNonFinite<float, LDPC_V_MINSUM> && sizeof(LT) == 4;    // (fp16 lam saturates by its own rule)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LT *lam = reinterpret_cast<LT *>(smem);
    // [0] next frame; [1..3] "sweep n moved" at 1 + n % 3 (cleared by thread 0 two sweeps before its use); [4] "the channel's hard
    // decisions are not a codeword"; [5] (f32 lam) "some LLR of the frame that just stopped is not finite"
    int *ctl = reinterpret_cast<int *>(smem + (((size_t)g.N * sizeof(LT) + 15) & ~(size_t)15));
    const int T = g.T, tid = threadIdx.x;
    const int W = T >> 6, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nslab = ((ctab_t)g.step_ptr)[g.nstep];
    const uint32_t lam0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem;   // LDS byte address of lam
#if !LAYERED_CSR_CONT
    Rec *const rec = rec_all + (size_t)blockIdx.x * nslab * T + tid;        // this thread's record of slab s: rec[s T]
#else
    typedef typename std::conditional<kInt8, int16_t, float>::type ST;      // a cell of the state's sum of check messages
#endif
    int frame = blockIdx.x;
    while (frame < A.batch) {
        const size_t fN = (size_t)frame * g.N;
#if LAYERED_CSR_CONT
        // the frame's slot of the state: its records (this thread's of slab s: rec[s T]) and its row of sums
        const size_t slot = (size_t)K.first + (size_t)frame;
        Rec *const rec = reinterpret_cast<Rec *>(K.rec) + slot * nslab * T + tid;
        ST *const sum = reinterpret_cast<ST *>(K.sum) + slot * g.N;
#endif
        // ---- lam <- channel LLRs, as stored: saturated, rounded to fp16 / the float (eight per lane and request when the frame is 16-byte aligned)
        bool wide;
        if constexpr (kInt8)    // (int8 LLRs: 8 cells are one 8-byte request)
            wide = (g.N & 7) == 0 && A.llr_fmt != LLR_F64 && !A.final_lam && (((uintptr_t)A.bits + fN) & 7) == 0 &&
                   (((uintptr_t)A.llr + fN * (A.llr_fmt == LLR_I8 ? 1 : A.llr_fmt == LLR_F16 ? 2 : 4)) & (A.llr_fmt == LLR_I8 ? 7 : 15)) == 0;
        else
            wide = (g.N & 7) == 0 && A.llr_fmt != LLR_F64 && !A.final_lam &&
                          (((uintptr_t)A.llr + fN * (A.llr_fmt == LLR_F16 ? 2 : 4)) & 15) == 0 && (((uintptr_t)A.bits + fN) & 7) == 0;   // (uniform)
#if LAYERED_CSR_CONT
        wide = wide && ((uintptr_t)sum & 15) == 0;      // (the slot's row of sums is read and written eight cells per lane as well; uniform)
        // ---- lam <- the channel LLRs as the cell takes them in, plus the slot's sum of check messages, as the cell stores that:
        // fl32(C' + S) (f32), that saturated and rounded to fp16, or clip(q + S, +-127) (int8).  A reset slot adds +0
        if constexpr (kInt8) {
            if (wide) {
                with_llr_format_i8(A.llr_fmt, [&](auto fmt) {
#pragma unroll 4
                    for (int i = tid * 8; i < g.N; i += T * 8)
                        *reinterpret_cast<uint2 *>(lam + i) = add_sum_q8(load_q8<decltype(fmt)::value>(A.llr, fN + i, A.qscale), *reinterpret_cast<const uint4 *>(sum + i));
                });
            } else {
                with_llr_format_i8(A.llr_fmt, [&](auto fmt) {
#pragma unroll 8
                    for (int i = tid; i < g.N; i += T) lam[i] = (int8_t)min(max(load_q<decltype(fmt)::value>(A.llr, fN + i, A.qscale) + (int)sum[i], -127), 127);
                });
            }
        } else if (wide) {
            with_llr_format(A.llr_fmt, [&](auto fmt) {
#pragma unroll 4
                for (int i = tid * 8; i < g.N; i += T * 8) {
                    cell8 h;
                    load_llr8<LT, decltype(fmt)::value>(A.llr, fN + i, h);
                    const float4 a = *reinterpret_cast<const float4 *>(sum + i), b = *reinterpret_cast<const float4 *>(sum + i + 4);
                    h[0] = Cell<LT>::of((float)h[0] + a.x); h[1] = Cell<LT>::of((float)h[1] + a.y); h[2] = Cell<LT>::of((float)h[2] + a.z); h[3] = Cell<LT>::of((float)h[3] + a.w);
                    h[4] = Cell<LT>::of((float)h[4] + b.x); h[5] = Cell<LT>::of((float)h[5] + b.y); h[6] = Cell<LT>::of((float)h[6] + b.z); h[7] = Cell<LT>::of((float)h[7] + b.w);
                    Cell<LT>::st8(lam + i, h);
                }
            });
        } else {
            with_llr_format(A.llr_fmt, [&](auto fmt) {
#pragma unroll 8
                for (int i = tid; i < g.N; i += T) lam[i] = Cell<LT>::of((float)Cell<LT>::llr(load_llr_as<float, decltype(fmt)::value>(A.llr, fN + i)) + sum[i]);
            });
        }
#else
        if constexpr (kInt8) {
            // ---- lam <- the quantised channel LLRs (int8 LLRs as they are)
            if (wide) {
                with_llr_format_i8(A.llr_fmt, [&](auto fmt) {
#pragma unroll 4
                    for (int i = tid * 8; i < g.N; i += T * 8) *reinterpret_cast<uint2 *>(lam + i) = load_q8<decltype(fmt)::value>(A.llr, fN + i, A.qscale);
                });
            } else {
                with_llr_format_i8(A.llr_fmt, [&](auto fmt) {
#pragma unroll 8
                    for (int i = tid; i < g.N; i += T) lam[i] = (int8_t)load_q<decltype(fmt)::value>(A.llr, fN + i, A.qscale);
                });
            }
        } else if (wide) {
            with_llr_format(A.llr_fmt, [&](auto fmt) {
#pragma unroll 4
                for (int i = tid * 8; i < g.N; i += T * 8) {
                    cell8 h;
                    load_llr8<LT, decltype(fmt)::value>(A.llr, fN + i, h);
                    Cell<LT>::st8(lam + i, h);
                }
            });
        } else {
            with_llr_format(A.llr_fmt, [&](auto fmt) {
#pragma unroll 8
                for (int i = tid; i < g.N; i += T) lam[i] = Cell<LT>::llr(load_llr_as<float, decltype(fmt)::value>(A.llr, fN + i));
            });
        }
#endif
        if (tid == 0) { ctl[1] = 0; ctl[2] = 0; ctl[3] = 0; ctl[4] = 0; if constexpr (kVeto) ctl[5] = 0; }
        lds_barrier();
        bool conv = false;
        int n = 0;
        {   // syndrome of the hard decisions before the first sweep (reads only: no barrier between steps)
            bool odd = false;
            for (int s = 0; s < nslab; s++) {
                const int c0 = ((ctab_t)g.slab)[2 * s], wd = ((ctab_t)g.wdeg)[s * W + wave] & 0xFF;
                const uint16_t *cp = g.cols + c0 + tid;
                bool par = false;
                for (int k = 0; k < wd; k++) {
                    const uint32_t c = cp[(size_t)k * T];
                    if (c != kNoEdge) par ^= *lds_cell<LT>(lam0 + (uint32_t)sizeof(LT) * c) > (LT)0;
                }
                odd |= par;
            }
            if (__builtin_amdgcn_ballot_w64(odd) != 0 && (tid & 63) == 0) ctl[4] = 1;
            lds_barrier();
            conv = ctl[4] == 0;
        }
        if (!conv) {
            for (n = 1; n <= A.max_iters; n++) {
                bool odd = false, flip = false;
                if (tid == 0) ctl[1 + (n + 1) % 3] = 0;                 // the flag of the NEXT sweep (last read two sweeps ago)
                for (int st = 0; st < g.nstep; st++) {
                    const int s0 = ((ctab_t)g.step_ptr)[st], s1 = ((ctab_t)g.step_ptr)[st + 1];
                    for (int s = s0; s < s1; s++) {
                        const int c0 = ((ctab_t)g.slab)[2 * s], wv = ((ctab_t)g.wdeg)[s * W + wave];
                        const uint16_t *cp = g.cols + c0 + tid;
                        Rec out;
#if LAYERED_CSR_CONT
                        {   // every sweep subtracts the stored messages: the first one those the slot holds (all +0 in a reset slot)
                            const Rec in = rec[(size_t)s * T];
                            csr_row_at<LT, DCLASS, false, RULE>(cp, T, wv & 0xFF, (wv & 0x100) != 0, lam0, in, out, odd, flip, rule);
                        }
#else
                        if (n == 1) {
                            const Rec none{};
                            csr_row_at<LT, DCLASS, true, RULE>(cp, T, wv & 0xFF, (wv & 0x100) != 0, lam0, none, out, odd, flip, rule);
                        } else {
                            const Rec in = rec[(size_t)s * T];
                            csr_row_at<LT, DCLASS, false, RULE>(cp, T, wv & 0xFF, (wv & 0x100) != 0, lam0, in, out, odd, flip, rule);
                        }
#endif
                        rec[(size_t)s * T] = out;
                    }
                    if (st == g.nstep - 1 && __builtin_amdgcn_ballot_w64(odd || flip) != 0 && (tid & 63) == 0) ctl[1 + n % 3] = 1;
                    lds_barrier();
                }
                if (ctl[1 + n % 3] == 0) { conv = true; break; }
            }
            if (n > A.max_iters) n = A.max_iters;
        }
        if constexpr (kVeto) {
            // LLRs that are not finite -- they left the float range, or the channel gave them: failed, not "converged" (ldpc_math.h),
            // also for a frame whose channel decisions are a codeword before the first sweep.  Once per frame; `conv` comes from a
            // control word every thread read after a barrier, so it is workgroup-uniform and every wave reaches the barrier below
            if (conv) {
                bool bad = false;
                for (int i = tid; i < g.N; i += T) bad |= not_finite(lam[i]);
                if (__builtin_amdgcn_ballot_w64(bad) != 0 && (tid & 63) == 0) ctl[5] = 1;
                lds_barrier();
                conv = ctl[5] == 0;
            }
        }
        // ---- result: hard(lam) of a frame that stopped by the rule, the channel's decisions (as stored) otherwise (Orig.hs:69-70)
        if constexpr (kInt8) {
            // a frame out of sweeps quantises its channel LLRs again; no veto: the clip bounds the state
            if (wide) {
                with_llr_format_i8(A.llr_fmt, [&](auto fmt) {
#pragma unroll 4
                    for (int i = tid * 8; i < g.N; i += T * 8) {
                        const uint2 w = conv ? *reinterpret_cast<const uint2 *>(lam + i) : load_q8<decltype(fmt)::value>(A.llr, fN + i, A.qscale);
                        *reinterpret_cast<uint2 *>(A.bits + fN + i) = hard_q8(w);
                    }
                });
            } else {
                with_llr_format_i8(A.llr_fmt, [&](auto fmt) {
#pragma unroll 4
                    for (int i = tid; i < g.N; i += T) {
                        const int v = conv ? (int)lam[i] : load_q<decltype(fmt)::value>(A.llr, fN + i, A.qscale);
                        A.bits[fN + i] = v > 0 ? 1 : 0;
                        if (A.final_lam) A.final_lam[fN + i] = (double)v / (double)A.qscale;
                    }
                });
            }
        } else if (wide) {
            auto put = [&](int i, const cell8 &h) {
                uint32_t lo = 0, hi = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) { lo |= (h[k] > (LT)0 ? 1u : 0u) << (8 * k); hi |= (h[k + 4] > (LT)0 ? 1u : 0u) << (8 * k); }
                *reinterpret_cast<uint2 *>(A.bits + fN + i) = make_uint2(lo, hi);
            };
            if (conv) {
#pragma unroll 4
                for (int i = tid * 8; i < g.N; i += T * 8) put(i, Cell<LT>::ld8(lam + i));
            } else {
                with_llr_format(A.llr_fmt, [&](auto fmt) {
#pragma unroll 4
                    for (int i = tid * 8; i < g.N; i += T * 8) {
                        cell8 h;
                        load_llr8<LT, decltype(fmt)::value>(A.llr, fN + i, h);
                        put(i, h);
                    }
                });
            }
        } else {
            with_llr_format(A.llr_fmt, [&](auto fmt) {
#pragma unroll 4
                for (int i = tid; i < g.N; i += T) {
                    const float v = conv ? (float)lam[i] : (float)Cell<LT>::llr(load_llr_as<float, decltype(fmt)::value>(A.llr, fN + i));
                    A.bits[fN + i] = v > 0.f ? 1 : 0;
                    if (A.final_lam) A.final_lam[fN + i] = (double)v;
                }
            });
        }
#if LAYERED_CSR_CONT
        {
            // ---- the slot's new sum of check messages: lam as it stands less the channel LLR as the cell took it in, read from memory again --
            // the extrinsic value before its output format --, for EVERY frame however it stopped.  (The records are already the slot's.)
            if constexpr (kInt8) {
                with_llr_format_i8(A.llr_fmt, [&](auto fmt) {
                    if (wide) {
#pragma unroll 2
                        for (int i = tid * 8; i < g.N; i += T * 8)
                            *reinterpret_cast<uint4 *>(sum + i) = diff_q8(*reinterpret_cast<const uint2 *>(lam + i), load_q8<decltype(fmt)::value>(A.llr, fN + i, A.qscale));
                    } else {
#pragma unroll 4
                        for (int i = tid; i < g.N; i += T) sum[i] = (int16_t)((int)lam[i] - load_q<decltype(fmt)::value>(A.llr, fN + i, A.qscale));
                    }
                });
            } else {
                with_llr_format(A.llr_fmt, [&](auto fmt) {
                    if (wide) {
#pragma unroll 2
                        for (int i = tid * 8; i < g.N; i += T * 8) {
                            const cell8 h = Cell<LT>::ld8(lam + i);
                            cell8 c;
                            load_llr8<LT, decltype(fmt)::value>(A.llr, fN + i, c);
                            *reinterpret_cast<float4 *>(sum + i) = make_float4((float)h[0] - (float)c[0], (float)h[1] - (float)c[1], (float)h[2] - (float)c[2], (float)h[3] - (float)c[3]);
                            *reinterpret_cast<float4 *>(sum + i + 4) = make_float4((float)h[4] - (float)c[4], (float)h[5] - (float)c[5], (float)h[6] - (float)c[6], (float)h[7] - (float)c[7]);
                        }
                    } else {
#pragma unroll 4
                        for (int i = tid; i < g.N; i += T) sum[i] = (float)lam[i] - (float)Cell<LT>::llr(load_llr_as<float, decltype(fmt)::value>(A.llr, fN + i));
                    }
                });
            }
        }
        if (S.out != nullptr)                           // (the soft output is optional here; workgroup-uniform)
#endif
#if LAYERED_CSR_SOFT
        {
            // ---- soft output: lam as it stands -- whether the frame converged, ran out of sweeps or was vetoed --, less (extrinsic) the
            // channel LLR as the cell took it in, read from memory again as the branch of a frame out of sweeps above reads it
            const bool ext = S.kind != 0;
            const size_t ob = S.fmt == MOD_LLR_F32 ? 4 : S.fmt == MOD_LLR_F16 ? 2 : 1;
            const bool swide = wide && (((uintptr_t)S.out + fN * ob) & (ob == 1 ? 7 : 15)) == 0;     // (uniform)
            with_soft_format(S.fmt, [&](auto *tag) {
                typedef typename std::remove_pointer<decltype(tag)>::type OT;
                OT *const row = reinterpret_cast<OT *>(S.out) + fN;
                if constexpr (kInt8) {
                    with_llr_format_i8(A.llr_fmt, [&](auto fmt) {
                        if (swide) {
#pragma unroll 2
                            for (int i = tid * 8; i < g.N; i += T * 8) {
                                const uint2 w = *reinterpret_cast<const uint2 *>(lam + i);
                                uint2 c = make_uint2(0u, 0u);
                                if (ext) c = load_q8<decltype(fmt)::value>(A.llr, fN + i, A.qscale);
                                OT o[8];
#pragma unroll
                                for (int k = 0; k < 4; k++) {
                                    o[k] = soft_of_q<OT>((int)(int8_t)(w.x >> (8 * k)) - (int)(int8_t)(c.x >> (8 * k)), A.qscale);
                                    o[k + 4] = soft_of_q<OT>((int)(int8_t)(w.y >> (8 * k)) - (int)(int8_t)(c.y >> (8 * k)), A.qscale);
                                }
                                st_soft8(row + i, o);
                            }
                        } else {
#pragma unroll 4
                            for (int i = tid; i < g.N; i += T) {
                                int v = (int)lam[i];
                                if (ext) v -= load_q<decltype(fmt)::value>(A.llr, fN + i, A.qscale);
                                row[i] = soft_of_q<OT>(v, A.qscale);
                            }
                        }
                    });
                } else {
                    with_llr_format(A.llr_fmt, [&](auto fmt) {
                        if (swide) {
#pragma unroll 2
                            for (int i = tid * 8; i < g.N; i += T * 8) {
                                const cell8 h = Cell<LT>::ld8(lam + i);
                                cell8 c = h;
                                if (ext) load_llr8<LT, decltype(fmt)::value>(A.llr, fN + i, c);
                                OT o[8];
#pragma unroll
                                for (int k = 0; k < 8; k++) o[k] = llr_out<OT>(ext ? (float)h[k] - (float)c[k] : (float)h[k], S.qscale);
                                st_soft8(row + i, o);
                            }
                        } else {
#pragma unroll 4
                            for (int i = tid; i < g.N; i += T) {
                                float v = (float)lam[i];
                                if (ext) v = v - (float)Cell<LT>::llr(load_llr_as<float, decltype(fmt)::value>(A.llr, fN + i));
                                row[i] = llr_out<OT>(v, S.qscale);
                            }
                        }
                    });
                }
            });
        }
#endif
        if (tid == 0) {
            if (A.iters) A.iters[frame] = conv ? n : A.max_iters;
            if (A.conv) A.conv[frame] = conv ? 1 : 0;
            ctl[0] = (int)gridDim.x + atomicAdd(A.work_counter, 1);
        }
        lds_barrier();   // also: every lam read of this frame is done before the next frame's LLRs are written over it
        frame = ctl[0];
        lds_barrier();   // (nobody still reads ctl[0] when thread 0 of a fast wave writes the next one)
    }
