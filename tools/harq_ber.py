#!/usr/bin/env python3
"""tools/harq_ber.py [--code jpl.1024.4.5] [--modulation 16qam] [--mode chase|ir] [--rounds 3] [--bits E] [--block B] [--k 0]
[--ebn0 2,4,6,8] [--frames 4096] [--batch 1024] [--iters 50] [--seed 1] [--llr f32|f16|i8] [--crc KIND] -- frame error rate after 1 .. R HARQ rounds
over block fading (csrc/demap_rm.hip, csrc/ratematch.cc).  The circular buffer is the source's transmitted prefix 0 .. n_tx - 1; every
round sends E bits of it (--bits, default n_tx; E > n_tx repeats bits inside a round):
  chase  every round reads the buffer from offset 0: the same bits again;
  ir     round r reads from offset (r E) mod n_tx: incremental redundancy, another window of the buffer.
Round r draws its noise and its gains with seed + r and carries the messages of round 0 (ldpc_sim_transmit_rm with d_msg_in); its
samples are demapped with their gains and added to the soft buffer of the earlier rounds (ldpc_demap_dev_rm, accumulate from round 1
on), the buffer is decoded by a flooding min-sum float32 context and tallied on the device.  Eb/N0 is that of ONE round, at its rate
k / E.  --block: symbols per fading block (default: one gain per frame and round); --k: the Rician factor (0 = Rayleigh).  --llr: the
format of the soft buffer; f16 and i8 saturate, and are converted to float32 for the decoder here.
--crc KIND (crc6, crc11, crc16, crc24a, crc24b, crc24c, crc32; csrc/crc.hip): the last w message bits are the CRC of the others.  The
payloads are drawn by a torch generator seeded with --seed, the CRC is attached on the device (ldpc_crc_attach_dev) and the messages
enter round 0 as d_msg_in.  Every round is judged as a receiver judges it, by ldpc_sim_crc_check on the decoded bits; an ACK is sticky:
a frame counts as delivered in the first round its CRC passes.  Further columns: the NACK rate after each round (frames not yet ACKed),
the undetected errors (frames whose message was wrong in the round that ACKed them; ldpc_sim_tally_crc) and the mean number of rounds
until the ACK, over the ACKed frames.  The FER columns stay the genie's.  Without --crc the output is what it was."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecc_ldpc_amd as E  # noqa: E402


def crc_columns(k, R):
    """k [R][4]: per round {frames, first ACKs, frames in error, first ACKs in error} -> the --crc columns ("" without --crc: no ACKs, no frames)"""
    if not k[0][0]:
        return ""
    acked = [sum(k[q][1] for q in range(r + 1)) for r in range(R)]
    rounds = sum((r + 1) * k[r][1] for r in range(R)) / acked[R - 1] if acked[R - 1] else float("nan")
    return " " + " ".join(f"{1.0 - acked[r] / k[r][0]:13.3e}" for r in range(R)) + f" {sum(k[r][3] for r in range(R)):10d} {rounds:18.2f}"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--code", default="jpl.1024.4.5", choices=["jpl.1024.4.5", "jpl.4096.4.5"])
    ap.add_argument("--modulation", default="16qam", choices=["bpsk", "qpsk", "8psk", "16qam", "64qam", "256qam", "1024qam", "4096qam"])
    ap.add_argument("--mode", default="chase", choices=["chase", "ir"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bits", type=int, default=0)
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--k", type=float, default=0.0)
    ap.add_argument("--ebn0", default="2,4,6,8")
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--llr", default="f32", choices=["f32", "f16", "i8"])
    ap.add_argument("--crc", default=None, choices=sorted(E.CRC_KINDS))
    a = ap.parse_args()
    points = [float(x) for x in a.ebn0.split(",")]
    B, R = min(a.batch, a.frames), a.rounds
    E.init(0)
    dev = torch.device("cuda", 0)
    ecc = E.ECC(os.path.join(ROOT, "codes"), f"ldpc/hip-minsum/{a.code}/{a.iters}/4/5", max_batch=B)
    sim, n_tx, N = ecc.sim, ecc.codeword_length, ecc.unpunctured_length
    mod = E.Modulation(a.modulation)
    n_bits = a.bits or n_tx
    tables = [E.Ratematch.circular(N, (r * n_bits) % n_tx if a.mode == "ir" else 0, n_bits, n_buf=n_tx) for r in range(R)]
    ns = mod.symbols(n_bits)
    fad = E.Fading(a.block or ns, a.k)
    dec = ecc.decoder
    soft = torch.empty((B, N), dtype={"f32": torch.float32, "f16": torch.float16, "i8": torch.int8}[a.llr], device=dev)
    sym = torch.empty((B, ns, 2), dtype=torch.float32, device=dev)
    gain = torch.empty((B, ns), dtype=torch.float32, device=dev)
    msgs = torch.empty((B, sim.k), dtype=torch.uint8, device=dev)
    bits = torch.empty((B, N), dtype=torch.uint8, device=dev)
    its = torch.empty(B, dtype=torch.int32, device=dev)
    qscale = 4.0
    crc = None
    if a.crc:
        crc = E.Crc.builtin(a.crc, sim.k - E.Crc.builtin_params(a.crc)[0])
        draw = torch.Generator(device=dev).manual_seed(a.seed)
        pay = torch.empty((B, sim.k), dtype=torch.uint8, device=dev)
        ok = torch.empty(B, dtype=torch.uint8, device=dev)
    print(f"{a.code}, {a.modulation} (m = {mod.bits}), {a.mode}, {R} rounds of {n_bits} bits ({ns} symbols; n_tx = {n_tx}, N = {N}), fading block = {fad.block}, "
          f"K = {a.k:g}, soft buffer {a.llr}, {dec.kernel_name}, {a.iters} iterations, seed {a.seed}" + (f", {a.crc}: {crc.n_bits} payload bits + {crc.width}" if crc else ""), flush=True)
    print(f"{'Eb/N0 dB':>9s} {'frames':>8s} " + " ".join(f"{'FER after ' + str(r + 1):>13s}" for r in range(R)) + f" {'mean iterations after ' + str(R):>24s}"
          + (" " + " ".join(f"{'NACK after ' + str(r + 1):>13s}" for r in range(R)) + f" {'undetected':>10s} {'mean rounds to ACK':>18s}" if crc else ""), flush=True)
    for db in points:
        tally = torch.zeros((R, 4), dtype=torch.int64, device=dev)
        acks = torch.zeros((R, 4), dtype=torch.int64, device=dev)   # per round: {frames, first ACKs, frames in error, first ACKs in error}
        done = 0
        while done < a.frames:
            n = min(B, a.frames - done)
            if crc:
                pay[:n] = torch.randint(0, 2, (n, sim.k), dtype=torch.uint8, device=dev, generator=draw)
                crc.attach(n, pay.data_ptr(), "bytes", None)
                acked = torch.zeros(n, dtype=torch.uint8, device=dev)
            for r, rm in enumerate(tables):
                sim.transmit_rm(mod, rm, fad, a.seed + r, done, n, db, sym.data_ptr(), gain.data_ptr(), (pay.data_ptr() if crc else None) if r == 0 else msgs.data_ptr(), "bytes",
                                msgs.data_ptr() if r == 0 else None, None)
                E.demap_rm(mod, rm, n, sym.data_ptr(), gain.data_ptr(), sim.noise_var_rm(mod, rm, db), soft.data_ptr(), a.llr, qscale, r > 0, None)
                llr = soft if a.llr == "f32" else soft.to(torch.float32) / (qscale if a.llr == "i8" else 1.0)
                torch.cuda.synchronize()                         # the context decodes on its own stream
                dec.decode_batch_dev(llr.data_ptr(), bits.data_ptr(), n, a.iters, its.data_ptr(), None, None)
                dec.synchronize()
                sim.tally(n, bits.data_ptr(), its.data_ptr(), tally[r].data_ptr(), None)
                if crc:
                    sim.crc_check(crc, n, bits.data_ptr(), ok.data_ptr(), "bytes", None)
                    first = ok[:n] & (1 - acked)                 # the ACK is sticky: a frame is judged in the first round it passes
                    acked |= first
                    sim.tally_crc(n, bits.data_ptr(), first.data_ptr(), acks[r].data_ptr(), None)
            done += n
        torch.cuda.synchronize()
        t = tally.cpu().tolist()
        print(f"{db:9.2f} {t[0][0]:8d} " + " ".join(f"{t[r][1] / t[r][0]:13.3e}" for r in range(R)) + f" {t[R - 1][3] / t[R - 1][0]:24.2f}" + crc_columns(acks.cpu().tolist(), R), flush=True)
    for rm in tables:
        rm.close()
    if crc:
        crc.close()
    mod.close(); ecc.close()


if __name__ == "__main__":
    main()
