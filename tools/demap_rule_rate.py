#!/usr/bin/env python3
"""tools/demap_rule_rate.py [BATCH=8192] -- the time of one demapper call under the two LLR rules (max-log and log-MAP:
include/ldpc_hip.h THE LLR RULE), on the same buffers: rows of N = 6144 float32 LLRs from samples that are constellation points plus
noise at a per-symbol SNR of 3 m dB.
  (a) 64-QAM as a table object (the 8 x 8 grid, m = 6), ldpc_demap_dev
  (b) 64-QAM as a product object (b = 3), ldpc_demap_dev
  (c) 4096-QAM (b = 6), ldpc_demap_dev
  (d) 64-QAM product through a circular rate-matching table with E = 2 N (fan-in 2), ldpc_demap_dev_rm
HIP events around each call, 3 warm-up runs, then 10 timed runs with the two rules alternating inside a repetition (tools/crc_rate.py);
median, min and max, and the log-MAP / max-log ratio of the medians."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecc_ldpc_amd as E  # noqa: E402

WARM, REPS, N = 3, 10, 6144
B = int(os.environ.get("BATCH", "8192"))


def stats(v):
    return float(np.median(v)), min(v), max(v)


def samples(mod, n_sym, dev, seed):
    pts = torch.from_numpy(mod.points).to(dev)
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
    rm = E.Ratematch.circular(N, 0, 2 * N)
    cases = (("(a) 64-QAM table, ldpc_demap_dev", E.Modulation(grid), None), ("(b) 64-QAM product, ldpc_demap_dev", E.Modulation("64qam"), None),
             ("(c) 4096-QAM, ldpc_demap_dev", E.Modulation("4096qam"), None), ("(d) 64-QAM product, ldpc_demap_dev_rm, fan-in 2", E.Modulation("64qam"), rm))
    print(f"[{B}][{N}] float32 LLRs a call, {REPS} timed runs after {WARM} warm-up runs, the rules alternating inside a repetition; HIP events around each call", flush=True)
    for name, base, table in cases:
        mods = {"max-log": base, "log-MAP": base.with_rule("logmap")}
        n_bits = N if table is None else 2 * N
        sym, nv = samples(base, base.symbols(n_bits), dev, 7)
        res = {k: [] for k in mods}
        torch.cuda.synchronize()
        for rep in range(WARM + REPS):
            for k, mod in mods.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                if table is None:
                    E.demap(mod, B, N, N, sym.data_ptr(), nv, out.data_ptr(), "f32", 0.0, None)
                else:
                    E.demap_rm(mod, table, B, sym.data_ptr(), None, nv, out.data_ptr(), "f32", 0.0, False, None)
                b.record()
                b.synchronize()
                if rep >= WARM:
                    res[k].append(a.elapsed_time(b))
        med = {}
        for k, v in res.items():
            med[k], lo, hi = stats(v)
            print(f"{name:50s} {k:8s} median {med[k]:9.3f} ms   min {lo:9.3f}   max {hi:9.3f}   {B * N / med[k] / 1e6:9.2f} G LLR/s", flush=True)
        print(f"{name:50s} log-MAP / max-log = {med['log-MAP'] / med['max-log']:.2f}", flush=True)
        for m in mods.values():
            m.close()
        del sym
    rm.close()


if __name__ == "__main__":
    main()
