#!/usr/bin/env python3
"""tools/ratematch_rate.py -- what the gather form of csrc/demap_rm.hip costs (profiles/r18_ratematch.txt).  E = N = 64 800, batch 4 096
(RM_BATCH overrides), fp16 output, a 64-point table object and the 64QAM product object:
  (a) ldpc_demap_dev_rm with an injective circular table (a rotation) against ldpc_demap_dev_il, the lane = symbol scatter, same table;
  (b) ldpc_demap_dev_rm with E = 2 N against the two calls it fuses: ldpc_demap_dev (float32, n_tx = N = E) + ldpc_ratematch_llr_dev.
HIP events around each call, 3 warm-up runs, then 10 timed runs with the versions alternating inside a repetition; median, min and max.
Each pair's outputs are compared bit for bit at the timed size."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecc_ldpc_amd as E  # noqa: E402
from tests import modulation_spec as ms  # noqa: E402
from tests import ratematch_spec as rs  # noqa: E402

N, B = 64800, int(os.environ.get("RM_BATCH", "4096"))
REPS, WARM = 10, 3
E.init(0)
dev = torch.device("cuda", 0)


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)


def timed(fns):
    """alternating: every repetition runs each fn once between two events -> {name: [ms]}"""
    res = {k: [] for k in fns}
    for rep in range(WARM + REPS):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= WARM:
                res[k].append(a.elapsed_time(b))
    return res


def report(tag, res):
    for k, v in res.items():
        v = sorted(v)
        say(f"{tag:34s} {k:38s} median {v[len(v) // 2]:9.3f} ms   min {v[0]:9.3f}   max {v[-1]:9.3f}   ({len(v)} runs)")


objs = {"64-point table (grid64)": E.Modulation(ms.grid64()), "64QAM product (b = 3)": E.Modulation("64qam")}
say(f"N = {N}, batch = {B}, fp16 output, {REPS} timed runs after {WARM} warm-up runs, versions alternating inside a repetition; HIP events around each call")
for name, mod in objs.items():
    m = mod.bits
    assert m == 6
    # (a) an injective circular table (a rotation of the codeword), E = N
    pos = rs.circular_positions(N, 12345, N)
    rm, il = E.Ratematch(pos, N), E.Interleaver(pos, N)
    ns = mod.symbols(N)
    g = torch.Generator(device=dev).manual_seed(1)
    sym = torch.randn((B, ns, 2), device=dev, generator=g, dtype=torch.float32)
    o1 = torch.empty((B, N), dtype=torch.float16, device=dev)
    o2 = torch.empty((B, N), dtype=torch.float16, device=dev)
    res = timed({"ldpc_demap_dev_rm (gather)": lambda: E.demap_rm(mod, rm, B, sym.data_ptr(), None, 0.05, o1.data_ptr(), "f16", 0.0, False, None),
                 "ldpc_demap_dev_il (scatter)": lambda: E.demap_il(mod, il, B, sym.data_ptr(), 0.05, o2.data_ptr(), "f16", 0.0, None)})
    torch.cuda.synchronize()
    say(f"(a) {name}: outputs equal bit for bit: {bool(torch.equal(o1.view(torch.int16), o2.view(torch.int16)))}")
    report(f"(a) {name}", res)
    rm.close(); il.close()
    del sym, o2
    # (b) E = 2 N circular: fused against ldpc_demap_dev (float32, n_tx = N = E) + ldpc_ratematch_llr_dev
    E2 = 2 * N
    pos = rs.circular_positions(N, 12345, E2)
    rm = E.Ratematch(pos, N)
    ns = mod.symbols(E2)
    sym = torch.randn((B, ns, 2), device=dev, generator=g, dtype=torch.float32)
    tx = torch.empty((B, E2), dtype=torch.float32, device=dev)
    o2 = torch.empty((B, N), dtype=torch.float16, device=dev)

    def two():
        E.demap(mod, B, E2, E2, sym.data_ptr(), 0.05, tx.data_ptr(), "f32", 0.0, None)
        E.ratematch_llr(rm, B, tx.data_ptr(), o2.data_ptr(), "f16", 0.0, False, None)

    res = timed({"ldpc_demap_dev_rm (fused)": lambda: E.demap_rm(mod, rm, B, sym.data_ptr(), None, 0.05, o1.data_ptr(), "f16", 0.0, False, None),
                 "ldpc_demap_dev + ldpc_ratematch_llr_dev": two,
                 "  of which ldpc_demap_dev": lambda: E.demap(mod, B, E2, E2, sym.data_ptr(), 0.05, tx.data_ptr(), "f32", 0.0, None),
                 "  of which ldpc_ratematch_llr_dev": lambda: E.ratematch_llr(rm, B, tx.data_ptr(), o2.data_ptr(), "f16", 0.0, False, None)})
    torch.cuda.synchronize()
    say(f"(b) {name}: outputs equal bit for bit: {bool(torch.equal(o1.view(torch.int16), o2.view(torch.int16)))}")
    report(f"(b) {name}", res)
    rm.close()
    del sym, tx, o1, o2
    mod.close()
