#!/usr/bin/env python3
"""tools/demap_apriori_rate.py [BATCH=8192] -- the time of one ldpc_demap_dev_il_apriori call (csrc/demap_apriori.hip) next to
ldpc_demap_dev_il and ldpc_demap_dev_il_csi on the same samples, table and output buffer: rows of N = 6144 float32 LLRs through a random
interleaver, samples that are constellation points plus noise at a per-symbol SNR of 3 m dB, a-priori values N(0, 4^2).
  (a) QPSK (m = 2)   (b) 16QAM (m = 4)   (c) 64-QAM as a table object (the 8 x 8 grid, m = 6), each under max-log and log-MAP
HIP events around each call, 3 warm-up runs, then 10 timed runs with the calls alternating inside a repetition (tools/demap_rule_rate.py);
median, min and max, and the ratio of the a-priori call's median to ldpc_demap_dev_il's."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecc_ldpc_amd as E  # noqa: E402

WARM, REPS, N = 3, 10, 6144
B = int(os.environ.get("BATCH", "8192"))


def samples(mod, n_sym, dev, seed):
    pts = torch.from_numpy(np.array(mod.points)).to(dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    idx = torch.randint(0, pts.shape[0], (B, n_sym), device=dev, generator=g)
    nv = mod.energy / 2.0 / 10.0 ** (0.3 * mod.bits)
    return (pts[idx] + torch.randn((B, n_sym, 2), device=dev, generator=g) * nv ** 0.5).contiguous(), nv


def main():
    E.init(0)
    dev = torch.device("cuda", 0)
    lev = (np.arange(8) * 2.0 - 7.0) / np.sqrt(42.0)
    grid = np.array([[lev[p >> 3], lev[p & 7]] for p in range(64)], np.float32)
    out = torch.empty((B, N), dtype=torch.float32, device=dev)
    la = (torch.randn((B, N), device=dev, generator=torch.Generator(device=dev).manual_seed(3)) * 4.0).contiguous()
    il = E.Interleaver(np.random.default_rng(9).permutation(N).astype(np.int32), N)
    print(f"[{B}][{N}] float32 LLRs a call, {REPS} timed runs after {WARM} warm-up runs, the calls alternating inside a repetition; HIP events around each call", flush=True)
    for name, base in (("(a) QPSK", E.Modulation("qpsk")), ("(b) 16QAM", E.Modulation("16qam")), ("(c) 64-QAM table", E.Modulation(grid))):
        for rule in ("maxlog", "logmap"):
            mod = base.with_rule(rule)
            sym, nv = samples(base, base.symbols(N), dev, 7)
            gain = torch.ones((B, base.symbols(N)), device=dev)
            calls = {"demap_il": lambda: E.demap_il(mod, il, B, sym.data_ptr(), nv, out.data_ptr(), "f32", 0.0, None),
                     "demap_il_csi": lambda: E.demap_il_csi(mod, il, B, sym.data_ptr(), gain.data_ptr(), nv, out.data_ptr(), "f32", 0.0, None),
                     "demap_il_apriori": lambda: E.demap_il_apriori(mod, il, B, sym.data_ptr(), None, nv, la.data_ptr(), out.data_ptr(), "f32", 0.0, None)}
            res = {k: [] for k in calls}
            torch.cuda.synchronize()
            for rep in range(WARM + REPS):
                for k, f in calls.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    f()
                    b.record()
                    b.synchronize()
                    if rep >= WARM:
                        res[k].append(a.elapsed_time(b))
            med = {k: float(np.median(v)) for k, v in res.items()}
            for k, v in res.items():
                print(f"{name:18s} {rule:7s} {k:17s} median {med[k]:9.3f} ms   min {min(v):9.3f}   max {max(v):9.3f}   {B * N / med[k] / 1e6:9.2f} G LLR/s", flush=True)
            print(f"{name:18s} {rule:7s} demap_il_apriori / demap_il = {med['demap_il_apriori'] / med['demap_il']:.2f}", flush=True)
            mod.close()
            del sym
        base.close()
    il.close()


if __name__ == "__main__":
    main()
