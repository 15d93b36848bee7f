"""Frame errors, frames sent on, mean sweeps and time of the two-stage decode (ldpc_cascade_decode_dev) next to its two stages alone, on
IDENTICAL frames -- the method of tools/aminstar_fer.py, so that the rows line up with profiles/r23_aminstar.txt.

Codes: codes/jpl.1024.4.5 and codes/jpl.4096.4.5.  Frames: the device frame source (ldpc_sim_generate, all-zero codewords + AWGN, f32 LLRs), one
seeded batch per (code, Eb/N0), decoded by every leg.  Legs: stage 1 alone, twice -- the quasi-cyclic on-chip layered kernel (3/4, f32) and
the on-chip layered kernel for any H (3/4, fp16 cells, CSR with the block rows as layers); A-min* alone (the kernel for any H, fp16 cells);
the cascade of each first stage with that A-min* context at capacity = batch, batch / 4 and batch / 16.  Per leg: frame errors over the k
message bits, frames sent to stage 2, overflow (frames that failed stage 1 beyond the capacity), mean of the returned sweep counts, the time
of the WHOLE call (HIP events on the caller's stream around it; a warm-up call, then --reps timed calls, the legs taking turns; median
[min..max]) and decoded-information Gbit/s = frames x k / that time.

usage: python tools/cascade_fer.py [--frames 16384] [--reps 3] [--max-iters 20] [--codes jpl.1024.4.5 jpl.4096.4.5] [--ebn0 DB [DB ...]]
(profiles/r24_cascade.txt)"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ecc_ldpc_amd as E  # noqa: E402
from tests.helpers import load  # noqa: E402

EBN0 = (2.5, 3.0, 3.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-iters", type=int, default=20)
    ap.add_argument("--codes", nargs="+", default=["jpl.1024.4.5", "jpl.4096.4.5"])
    ap.add_argument("--ebn0", type=float, nargs="+", default=list(EBN0))
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    out = lambda s: print(s, flush=True)   # noqa: E731
    E.init(0)
    F, MI = a.frames, a.max_iters
    stream = torch.cuda.Stream()
    out(f"# two-stage decode on identical frames: {F} frames per point from the device frame source (all-zero codewords + AWGN, seed {a.seed}), {MI} sweeps at most in "
        f"either stage, {a.reps} timed calls per leg after a warm-up (HIP events around the whole call; median [min..max]), legs alternating")
    for name in a.codes:
        c = load(name)
        csr = E.Code.from_csr(c.graph.row_ptr, c.graph.col_idx, c.N)
        csr.set_layers(np.arange(0, c.M + 1, c.sz, dtype=np.int32))
        qc = E.Decoder(E.Code.from_qc(c.sz, c.offsets), "min", "f32", F, schedule="layered")
        f16 = E.Decoder(csr, "min", "f16", F, schedule="layered", path="fused")
        amin = E.Decoder(csr, "min", "f16", F, schedule="layered", path="fused", cn_rule="aminstar")
        caps = (F, F // 4, F // 16)
        legs = [("QC 3/4 f32 alone", qc), ("CSR 3/4 f16 alone", f16), ("A-min* f16 alone", amin)]
        legs += [(f"{lab} > A-min*, cap {cap}", E.Cascade(d, amin, cap)) for lab, d in (("QC 3/4 f32", qc), ("CSR 3/4 f16", f16)) for cap in caps]
        sim = E.Sim(csr, c.k, c.n_tx, max_batch=F)
        out(f"{name} N={c.N} M={c.M} k={c.k} transmitted={c.n_tx}")
        out(f"  stage 1 (QC): {qc.kernel_name}; stage 1 (CSR): {f16.kernel_name}; stage 2: {amin.kernel_name}; cascade device bytes at capacity {F}: {legs[3][1].nbytes}")
        llr = torch.empty((F, c.N), dtype=torch.float32, device="cuda")
        bits = torch.empty((F, c.N), dtype=torch.uint8, device="cuda")
        iters = torch.empty(F, dtype=torch.int32, device="cuda")
        conv = torch.empty(F, dtype=torch.uint8, device="cuda")
        stats = torch.zeros(3, dtype=torch.int32, device="cuda")
        for db in a.ebn0:
            sim.generate(a.seed, 0, F, db, llr.data_ptr())
            torch.cuda.synchronize()
            times, last = [[] for _ in legs], [None] * len(legs)
            for r in range(a.reps + 1):
                for j, (_, leg) in enumerate(legs):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    if isinstance(leg, E.Cascade):
                        leg.decode_batch_dev(llr.data_ptr(), bits.data_ptr(), F, MI, MI, iters.data_ptr(), conv.data_ptr(), None, stats.data_ptr(), stream.cuda_stream)
                    else:
                        leg.decode_batch_dev(llr.data_ptr(), bits.data_ptr(), F, MI, iters.data_ptr(), conv.data_ptr(), stream.cuda_stream)
                    t1.record(stream)
                    stream.synchronize()
                    if r:
                        times[j].append(t0.elapsed_time(t1))
                    if r == a.reps:
                        st = stats.cpu().numpy().view(np.uint32).tolist() if isinstance(leg, E.Cascade) else None
                        last[j] = (int(bits[:, :c.k].any(dim=1).sum()), float(iters.float().mean()), int((conv == 0).sum()), st)
            for (label, _), t, (fe, sw, unconv, st) in zip(legs, times, last):
                ms = statistics.median(t)
                sent = f"sent on {st[1]:6d}  overflow {st[0] - st[1]:6d}  failed again {st[2]:6d}" if st else f"not converged {unconv:6d}" + " " * 39
                out(f"  {db:.1f} dB {label:<34s}: frame errors {fe:6d} / {F}  {sent}  sweeps {sw:6.3f}  {ms:8.3f} ms [{min(t):.3f}..{max(t):.3f}]  "
                    f"{F * c.k / (ms * 1e-3) / 1e9:6.2f} Gbit/s")
        del llr, bits
        torch.cuda.empty_cache()
        sim.close()
        for _, leg in legs[3:]:
            leg.close()
        for d in (qc, f16, amin):
            d.close()
    E.close_all()


if __name__ == "__main__":
    main()
