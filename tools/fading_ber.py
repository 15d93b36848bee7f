#!/usr/bin/env python3
"""tools/fading_ber.py [--code jpl.1024.4.5] [--modulation 16qam] [--block 1] [--k 0] [--interleaver none|block|random]
[--ebn0 12,14,16,18] [--frames 4096] [--batch 1024] [--iters 50] [--seed 1] -- frame and bit error rates over the fading channel
(csrc/sim_mod_fading.hip): per Eb/N0 point, batches of ldpc_sim_generate_mod_il_fading (float32 LLRs weighted per symbol) are decoded
by a flooding min-sum float32 context and tallied on the device (ldpc_sim_tally).  Prints frames, frame errors, message-bit errors and
mean iterations per point.
--modulation: bpsk, qpsk, 8psk, 16qam, 64qam, 256qam, 1024qam, 4096qam.  --block: symbols per fading block; --k: the Rician factor (0 =
Rayleigh).  --interleaver none: the identity table; block: the block table of floor(n_tx / m) rows and m columns over the first rows * m
bits, the rest in place; random: a seeded random permutation of the transmitted prefix.  --code: jpl.1024.4.5 or jpl.4096.4.5."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecc_ldpc_amd as E  # noqa: E402
from encoder_rate import table_positions  # noqa: E402  (tools/encoder_rate.py: the three tables of its --interleaver)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--code", default="jpl.1024.4.5", choices=["jpl.1024.4.5", "jpl.4096.4.5"])
    ap.add_argument("--modulation", default="16qam", choices=["bpsk", "qpsk", "8psk", "16qam", "64qam", "256qam", "1024qam", "4096qam"])
    ap.add_argument("--block", type=int, default=1)
    ap.add_argument("--k", type=float, default=0.0)
    ap.add_argument("--interleaver", default="none", choices=["none", "block", "random"])
    ap.add_argument("--ebn0", default="12,14,16,18")
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    points = [float(x) for x in a.ebn0.split(",")]
    B = min(a.batch, a.frames)
    E.init(0)
    dev = torch.device("cuda", 0)
    ecc = E.ECC(os.path.join(ROOT, "codes"), f"ldpc/hip-minsum/{a.code}/{a.iters}/4/5", max_batch=B)
    sim, n_tx, N = ecc.sim, ecc.codeword_length, ecc.unpunctured_length
    mod = E.Modulation(a.modulation)
    il = E.Interleaver(table_positions(a.interleaver, n_tx, mod.bits), N)
    fad = E.Fading(a.block, a.k)
    dec = ecc.decoder
    llr = torch.empty((B, N), dtype=torch.float32, device=dev)
    bits = torch.empty((B, N), dtype=torch.uint8, device=dev)
    its = torch.empty(B, dtype=torch.int32, device=dev)
    print(f"{a.code}, {a.modulation} (m = {mod.bits}, {mod.symbols(n_tx)} symbols a frame), fading block = {a.block}, K = {a.k:g}, interleaver {a.interleaver}, "
          f"{dec.kernel_name}, {a.iters} iterations, seed {a.seed}", flush=True)
    print(f"{'Eb/N0 dB':>9s} {'frames':>8s} {'frame errors':>13s} {'bit errors':>11s} {'FER':>10s} {'BER':>10s} {'mean iterations':>16s}", flush=True)
    for db in points:
        tally = torch.zeros(4, dtype=torch.int64, device=dev)
        done = 0
        while done < a.frames:
            n = min(B, a.frames - done)
            sim.generate_mod_il_fading(mod, il, fad, a.seed, done, n, db, llr.data_ptr(), "f32", 0.0, None, None, "bytes", None, None)
            torch.cuda.synchronize()                             # the context decodes on its own stream
            dec.decode_batch_dev(llr.data_ptr(), bits.data_ptr(), n, a.iters, its.data_ptr(), None, None)
            dec.synchronize()
            sim.tally(n, bits.data_ptr(), its.data_ptr(), tally.data_ptr(), None)
            done += n
        torch.cuda.synchronize()
        fr, fe, be, it = tally.cpu().tolist()
        print(f"{db:9.2f} {fr:8d} {fe:13d} {be:11d} {fe / fr:10.3e} {be / (fr * sim.k):10.3e} {it / fr:16.2f}", flush=True)
    il.close(); mod.close(); ecc.close()


if __name__ == "__main__":
    main()
