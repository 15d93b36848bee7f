"""Frame error rate, mean sweeps and kernel time of the check-node rules of the on-chip layered kernel for any H (csrc/layered_csr.hip):
the 3/4, each (alpha, beta) of --cn-scale / --cn-offset, and A-min* (cn_rule = LDPC_CN_AMINSTAR), on IDENTICAL frames.

Codes: codes/jpl.1024.4.5 and codes/jpl.4096.4.5 as CSR with their block rows as layers (punctured columns: LLR 0), and the DVB-S2-shaped
short code (tests/dvbs2_short.py) in the order ldpc_csr_layer_order proposes.  Frames: the device frame source (ldpc_sim_generate, all-zero
codewords + AWGN, f32 LLRs), one seeded batch per (code, Eb/N0), decoded by every rule.  Per leg: frame errors over the k message bits
(a frame that is not converged returns the channel's decisions), mean sweeps, the kernel time of one launch (HIP events around the decode
kernel; a warm-up launch, then --reps timed launches, the legs taking turns; median [min..max]), microseconds per frame and decoded-
information Gbit/s = frames x k / kernel time.  The last lines of a point give A-min* against the 3/4: time per frame, time per frame and
sweep, and frame errors.

usage: python tools/aminstar_fer.py [--frames 16384] [--reps 3] [--max-iters 20] [--cell f16|f32] [--cn-scale A [A ...]] [--cn-offset B [B ...]]
                                    [--codes jpl.1024.4.5 jpl.4096.4.5 dvbs2-short] [--ebn0 DB [DB ...]]
(profiles/r23_aminstar.txt: --cn-scale 0.8125 0.875 --cn-offset 0 0 --reps 3)"""
from __future__ import annotations

import argparse
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ecc_ldpc_amd as E  # noqa: E402
from tests import dvbs2_short  # noqa: E402
from tests.helpers import load  # noqa: E402

ASM = os.path.join(ROOT, "ecc_ldpc_amd", "build", "layered_csr-hip-amdgcn-amd-amdhsa-gfx950.s")
EBN0 = {"jpl.1024.4.5": (2.5, 3.0, 3.5), "jpl.4096.4.5": (2.0, 2.5, 3.0), "dvbs2-short": (1.5, 2.0, 2.5)}


def resources(out):
    """registers and scratch of the A-min* instances next to the 3/4 ones, from the device assembly the build keeps"""
    try:
        text = open(ASM).read()
    except OSError:
        out(f"#   (no device assembly at {os.path.relpath(ASM, ROOT)}: registers and scratch not listed)")
        return
    for fam, n in (("layered_csr_kernel", 18), ("layered_csr_soft_kernel", 23), ("layered_csr_cont_kernel", 23)):
        for d in (8, 20, 32):
            for cell, t in (("DF16_", "_Float16"), ("f", "float")):
                row = []
                for arg in (cell, "NS_7MinStarI%sEE" % cell):
                    m = re.search(r"\.name:\s+_ZN4ldpc%d%sILi%dE%sEE\S*\n((?:\s+\.[a-z_]+:.*\n)+)" % (n, fam, d, arg), text)
                    f = dict(re.findall(r"\.([a-z_]+):\s+(\d+)", m.group(1))) if m else {}
                    row.append(f"VGPRs={f.get('vgpr_count')} scratch={f.get('private_segment_fixed_size')} B spilled VGPRs={f.get('vgpr_spill_count')}")
                out(f"#   {fam}<{d}, {t}>: {row[0]};  <{d}, MinStar<{t}>>: {row[1]}")


def codes(names):
    for name in names:
        if name == "dvbs2-short":
            rp, ci = dvbs2_short.csr()
            N, k = dvbs2_short.N, dvbs2_short.K
            perm, lp = E.Code.csr_layer_order(rp, ci, N)
            rp, ci = E.Code.permute_rows(rp, ci, perm)
            n_tx = N
        else:
            c = load(name)
            rp, ci, N, k, n_tx = c.graph.row_ptr, c.graph.col_idx, c.N, c.k, c.n_tx
            lp = np.arange(0, c.M + 1, c.sz, dtype=np.int32)
        code = E.Code.from_csr(rp, ci, N)
        code.set_layers(lp)
        yield name, code, N, len(rp) - 1, k, n_tx, len(lp) - 1


def in_turn(decs, llr, max_iters, reps):
    """a warm-up launch each, then `reps` timed launches each, taking turns -> per context (median ms, min, max, sweeps [F], bits [F][N])"""
    F, N = llr.shape
    bits = torch.empty((F, N), dtype=torch.uint8, device="cuda")
    iters = torch.empty(F, dtype=torch.int32, device="cuda")
    times, last = [[] for _ in decs], [None] * len(decs)
    for r in range(reps + 1):
        for j, dec in enumerate(decs):
            dec.set_timing(True)
            dec.decode_batch_dev(llr.data_ptr(), bits.data_ptr(), F, max_iters, iters.data_ptr(), None)
            dec.synchronize()
            n, ms = dec.kernel_time()
            if r:
                times[j].append(ms / max(n, 1))
            if r == reps:
                last[j] = (iters.clone(), bits.clone())
    return [(statistics.median(t), min(t), max(t)) + l for t, l in zip(times, last)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-iters", type=int, default=20)
    ap.add_argument("--cell", choices=("f16", "f32"), default="f16")
    ap.add_argument("--cn-scale", type=float, nargs="+", default=[])
    ap.add_argument("--cn-offset", type=float, nargs="+", default=[])
    ap.add_argument("--codes", nargs="+", choices=tuple(EBN0), default=list(EBN0))
    ap.add_argument("--ebn0", type=float, nargs="+", help="Eb/N0 in dB for every code (default: three points per code)")
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    n = max(len(a.cn_scale), len(a.cn_offset))
    sc = a.cn_scale * (n if len(a.cn_scale) == 1 else 1) or [0.75] * n
    of = a.cn_offset * (n if len(a.cn_offset) == 1 else 1) or [0.0] * n
    assert len(sc) == len(of) == n, "--cn-scale and --cn-offset: lists of one length, or one of them a single value"
    out = lambda s: print(s, flush=True)   # noqa: E731
    E.init(0)
    F, MI = a.frames, a.max_iters
    out(f"# check-node rules of layered_csr on identical frames: {F} frames per point from the device frame source (all-zero codewords + AWGN, seed {a.seed}), "
        f"{a.cell} cells, {MI} sweeps at most, {a.reps} timed launches per leg (median [min..max]), legs alternating")
    resources(out)
    for name, code, N, M, k, n_tx, nl in codes(a.codes):
        legs = [("3/4 min", dict())] + [(f"({s:g}, {o:g})", dict(cn_scale=s, cn_offset=o)) for s, o in zip(sc, of)] + [("A-min*", dict(cn_rule="aminstar"))]
        decs = [E.Decoder(code, "min", a.cell, F, schedule="layered", path="fused", **kw) for _, kw in legs]
        sim = E.Sim(code, k, n_tx, max_batch=F)
        out(f"{name} N={N} M={M} k={k} transmitted={n_tx} layers={nl}")
        for (label, _), d in zip(legs, decs):
            out(f"  {label:<14s}: {d.kernel_name} threads/wg={d.kernel_geometry[0]}")
        llr = torch.empty((F, N), dtype=torch.float32, device="cuda")
        for db in (a.ebn0 or EBN0[name]):
            sim.generate(a.seed, 0, F, db, llr.data_ptr())
            torch.cuda.synchronize()
            res = in_turn(decs, llr, MI, a.reps)
            row = {}
            for (label, _), (ms, lo, hi, iters, bits) in zip(legs, res):
                fe = int(bits[:, :k].any(dim=1).sum())
                sw = float(iters.float().mean())
                row[label] = (ms, sw, fe)
                out(f"  {db:.1f} dB {label:<14s}: frame errors {fe:6d} / {F} (FER {fe / F:.3e})  sweeps {sw:6.3f}  {ms:8.3f} ms [{lo:.3f}..{hi:.3f}]  "
                    f"{1e3 * ms / F:7.3f} us/frame  {1e6 * ms / F / max(sw, 1e-9):7.2f} ns/frame/sweep  {F * k / (ms * 1e-3) / 1e9:6.2f} Gbit/s")
            (m0, s0, f0), (m1, s1, f1) = row["3/4 min"], row["A-min*"]
            out(f"  {db:.1f} dB A-min* / 3/4 min: time per frame and sweep {(m1 / max(s1, 1e-9)) / (m0 / max(s0, 1e-9)):.3f}x, sweeps {s1 / max(s0, 1e-9):.3f}x, "
                f"time per frame {m1 / m0:.3f}x, frame errors {f1} against {f0}")
        del llr
        torch.cuda.empty_cache()
        sim.close()
        for d in decs:
            d.close()
    E.close_all()


if __name__ == "__main__":
    main()
