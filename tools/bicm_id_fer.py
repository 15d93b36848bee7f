#!/usr/bin/env python3
"""tools/bicm_id_fer.py [--code 1920.1280.3.303] [--labels gray|nongray|FILE.npy] [--ebn0 3.5,4,4.5,5] [--outer 4] [--sweeps 10] [--frames 4096]
[--batch 1024] [--rule maxlog|logmap] [--cell f32|f16|i8] [--decoder restart|continue] -- the frame error rate of the iterative receiver
(BICM-ID) after 1 .. R outer iterations, over Eb/N0.
--decoder continue: the decoder keeps its check messages across the outer iterations (one ldpc_decode_state for the batch, reset once per
batch of frames, ldpc_decode_batch_dev_continue in place of the soft call); the default, restart, is everything said below.

One outer iteration: ldpc_demap_dev_il_apriori, then ldpc_decode_batch_dev_soft with the extrinsic kind and float32 output, whose output is the
next a-priori buffer.  The first iteration's a-priori values are zeros; the decoder is restarted each time (it keeps no check-node messages
across outer iterations).  The symbols come from ldpc_sim_transmit_il (the code's own H as the encoder, random messages) through a random
interleaver (seed 9) and are the same for every outer iteration; a frame is in error when a message bit of the decoder's d_bits is
(ldpc_sim_tally; a frame out of sweeps returns the channel's decisions there).
Any table object can be given as a .npy file of [2^m][2] float32 points; built in are two labellings of 16QAM: "gray" (the library's) and
"nongray" (those points with the labels shuffled by numpy's default_rng(5).permutation(16), the labelling of tests/test_bicm_id_gpu.py)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecc_ldpc_amd as E  # noqa: E402


def labelling(name):
    if name in ("gray", "nongray"):
        m = E.Modulation("16qam")
        pts = np.array(m.points, np.float32)
        m.close()
        return pts if name == "gray" else np.ascontiguousarray(pts[np.random.default_rng(5).permutation(16)])
    return np.ascontiguousarray(np.load(name), np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--code", default="1920.1280.3.303")
    ap.add_argument("--labels", default="nongray")
    ap.add_argument("--ebn0", default="3.5,4.0,4.5,5.0")
    ap.add_argument("--outer", type=int, default=4)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rule", default="maxlog", choices=("maxlog", "logmap"))
    ap.add_argument("--cell", default="f32", choices=("f32", "f16", "i8"))
    ap.add_argument("--decoder", default="restart", choices=("restart", "continue"))
    a = ap.parse_args()
    from tests.helpers import load
    E.init(0)
    dev = torch.device("cuda", 0)
    c = load(a.code)
    N, B = c.N, a.batch
    code = E.Code.from_csr(c.graph.row_ptr, c.graph.col_idx, N)
    sim = E.Sim(code, None, N, systematic=True, max_batch=B)
    mod = E.Modulation(labelling(a.labels)).with_rule(a.rule)
    il = E.Interleaver(np.random.default_rng(9).permutation(N).astype(np.int32), N)
    dec = E.Decoder(code, "min", a.cell, B, schedule="layered", path="fused")
    state = E.DecodeState(dec, B) if a.decoder == "continue" else None
    n_sym = mod.symbols(N)
    sym = torch.empty((B, n_sym, 2), dtype=torch.float32, device=dev)
    llr, zeros = torch.empty((B, N), dtype=torch.float32, device=dev), torch.zeros((B, N), dtype=torch.float32, device=dev)
    ext = [torch.empty((B, N), dtype=torch.float32, device=dev) for _ in range(2)]
    bits = torch.empty((B, N), dtype=torch.uint8, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    print(f"# {a.code} (K = {sim.k}, N = {N}), {a.labels} labels of {1 << mod.bits} points, rule {a.rule}, cells {a.cell}, {a.outer} outer iterations of {a.sweeps} sweeps, "
          f"{a.frames} frames a point in batches of {B}" + (", the decoder continues from its state of the previous outer iteration" if state is not None else ""), flush=True)
    print("# Eb/N0 dB   " + "   ".join(f"FER after {r + 1}" for r in range(a.outer)) + "    frame errors", flush=True)
    for db in [float(x) for x in a.ebn0.split(",")]:
        nv = sim.noise_var(mod, db)
        tally = torch.zeros((a.outer, 4), dtype=torch.int64, device=dev)
        for first in range(0, a.frames, B):
            n = min(B, a.frames - first)
            torch.cuda.synchronize()
            sim.transmit_il(mod, il, 1, first, n, db, sym.data_ptr())
            la = zeros
            for r in range(a.outer):
                E.demap_il_apriori(mod, il, n, sym.data_ptr(), None, nv, la.data_ptr(), llr.data_ptr(), "f32", 0.0, None)
                torch.cuda.synchronize()                  # (the decoder runs on the context's own stream)
                if state is None:
                    dec.decode_batch_dev_soft(llr.data_ptr(), bits.data_ptr(), ext[r & 1].data_ptr(), n, a.sweeps, "extrinsic", "f32", 0.0, iters.data_ptr())
                else:
                    if r == 0:
                        state.reset()                     # once per batch of frames (on the decoder's stream, before its first call)
                    dec.decode_batch_dev_continue(state, llr.data_ptr(), bits.data_ptr(), n, a.sweeps, ext[r & 1].data_ptr(), "extrinsic", "f32", 0.0, iters.data_ptr())
                dec.synchronize()
                sim.tally(n, bits.data_ptr(), iters.data_ptr(), tally[r].data_ptr())
                la = ext[r & 1]
        torch.cuda.synchronize()
        t = tally.cpu().numpy()
        assert (t[:, 0] == a.frames).all()
        print(f"{db:9.2f}   " + "   ".join(f"{t[r, 1] / t[r, 0]:11.3e}" for r in range(a.outer)) + "    " + " ".join(str(int(t[r, 1])) for r in range(a.outer)), flush=True)
    assert ("layered_csr_soft_kernel" if state is None else "layered_csr_cont_kernel") in dec.kernel_name, dec.kernel_name
    if state is not None:
        state.close()
    for o in (dec, il, mod, sim, code):
        o.close()


if __name__ == "__main__":
    main()
