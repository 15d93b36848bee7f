#!/usr/bin/env python3
"""tools/demap_rule_fer.py [--code jpl.1024.4.5] [--frames 16384] [--batch 8192] [--iters 50] [--seed 1] [--block 8] [--qscale 4.0]
[--only awgn|rayleigh] -- frame error rate against Eb/N0 under the two LLR rules of the demappers (max-log and log-MAP:
include/ldpc_hip.h THE LLR RULE), on the two-step route: transmit, demap, decode, tally.  64-QAM and 1024-QAM (the product built-ins),
over AWGN (ldpc_sim_transmit, ldpc_demap_dev) and over Rayleigh block fading with perfect channel state (ldpc_sim_transmit_il_fading
through the identity table, --block symbols per gain; ldpc_demap_dev_il_csi).  Every point transmits once, with one seed, and the same
samples are demapped by both rules, into float32 and into int8 (--qscale, the same for both rules: a receiver would retune it for the
new LLR distribution; the int8 LLRs are divided by it again and decoded by the same float32 context, so the row shows the quantiser
alone).  The decoder is the code's flooding min-sum float32 context; the errors are tallied on the device (ldpc_sim_tally)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecc_ldpc_amd as E  # noqa: E402

POINTS = {("awgn", "64qam"): (9, 10, 11, 12, 13, 14), ("awgn", "1024qam"): (16, 17, 18, 19, 20, 21, 22),
          ("rayleigh", "64qam"): (14, 16, 18, 20, 22, 24, 26), ("rayleigh", "1024qam"): (22, 24, 26, 28, 30, 32, 34)}
ROWS = (("maxlog", "f32"), ("logmap", "f32"), ("maxlog", "i8"), ("logmap", "i8"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--code", default="jpl.1024.4.5", choices=["jpl.1024.4.5", "jpl.4096.4.5"])
    ap.add_argument("--frames", type=int, default=16384)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--qscale", type=float, default=4.0)
    ap.add_argument("--only", default=None, choices=["awgn", "rayleigh"])
    a = ap.parse_args()
    B = min(a.batch, a.frames)
    E.init(0)
    dev = torch.device("cuda", 0)
    ecc = E.ECC(os.path.join(ROOT, "codes"), f"ldpc/hip-minsum/{a.code}/{a.iters}/4/5", max_batch=B)
    sim, dec, n_tx, N = ecc.sim, ecc.decoder, ecc.codeword_length, ecc.unpunctured_length
    il = E.Interleaver(torch.arange(n_tx, dtype=torch.int32).numpy(), N)
    fad = E.Fading(a.block, 0.0)
    f32 = torch.empty((B, N), dtype=torch.float32, device=dev)
    i8 = torch.empty((B, N), dtype=torch.int8, device=dev)
    bits = torch.empty((B, N), dtype=torch.uint8, device=dev)
    its = torch.empty(B, dtype=torch.int32, device=dev)
    print(f"{a.code} (k = {sim.k}, n_tx = {n_tx}, N = {N}), {dec.kernel_name}, {a.iters} iterations, {a.frames} frames a point in batches of {B}, seed {a.seed}; "
          f"fading: Rayleigh, {a.block} symbols a block, perfect channel state; int8: qscale {a.qscale:g} for both rules", flush=True)
    for (chan, name), points in POINTS.items():
        if a.only and chan != a.only:
            continue
        base = E.Modulation(name)
        mods = {"maxlog": base, "logmap": base.with_rule("logmap")}
        ns = base.symbols(n_tx)
        sym = torch.empty((B, ns, 2), dtype=torch.float32, device=dev)
        gain = torch.empty((B, ns), dtype=torch.float32, device=dev)
        print(f"\n{name} (m = {base.bits}), {chan}", flush=True)
        print(f"{'Eb/N0 dB':>9s} {'frames':>8s} " + " ".join(f"{'FER ' + r + ' ' + f:>16s}" for r, f in ROWS) + " " + " ".join(f"{'iters ' + r + ' ' + f:>16s}" for r, f in ROWS), flush=True)
        for db in points:
            tally = torch.zeros((len(ROWS), 4), dtype=torch.int64, device=dev)
            done = 0
            while done < a.frames:
                n = min(B, a.frames - done)
                if chan == "awgn":
                    sim.transmit(base, a.seed, done, n, float(db), sym.data_ptr())
                else:
                    sim.transmit_il_fading(base, il, fad, a.seed, done, n, float(db), sym.data_ptr(), gain.data_ptr())
                nv = sim.noise_var(base, float(db))
                for row, (rule, fmt) in enumerate(ROWS):
                    out = f32 if fmt == "f32" else i8
                    if chan == "awgn":
                        E.demap(mods[rule], n, n_tx, N, sym.data_ptr(), nv, out.data_ptr(), fmt, a.qscale, None)
                    else:
                        E.demap_il_csi(mods[rule], il, n, sym.data_ptr(), gain.data_ptr(), nv, out.data_ptr(), fmt, a.qscale, None)
                    llr = f32 if fmt == "f32" else i8.to(torch.float32) / a.qscale
                    torch.cuda.synchronize()                     # the context decodes on its own stream
                    dec.decode_batch_dev(llr.data_ptr(), bits.data_ptr(), n, a.iters, its.data_ptr(), None, None)
                    dec.synchronize()
                    sim.tally(n, bits.data_ptr(), its.data_ptr(), tally[row].data_ptr(), None)
                done += n
            torch.cuda.synchronize()
            t = tally.cpu().tolist()
            print(f"{db:9.2f} {t[0][0]:8d} " + " ".join(f"{t[r][1] / t[r][0]:16.3e}" for r in range(len(ROWS))) + " " + " ".join(f"{t[r][3] / t[r][0]:16.2f}" for r in range(len(ROWS))),
                  flush=True)
        for m in mods.values():
            m.close()
    il.close(); ecc.close()


if __name__ == "__main__":
    main()
