#!/usr/bin/env python3
"""tools/crc_rate.py -- what the CRC check on decoded codewords costs (csrc/crc.hip; profiles/r19_crc.txt).  jpl.4096.4.5 decoded
bytes [batch][N], batch 65 536 (CRC_BATCH overrides), k = 4096 = 4072 payload bits + the 24 bits of crc24a:
  (a) ldpc_sim_crc_check: the flags straight from the decoded bytes (rows 4-byte aligned: four bytes a lane); (a1) the same bytes
      from an odd address, which takes the instance that loads a byte a lane;
  (b) ldpc_sim_extract_messages (bytes) followed by ldpc_crc_check_dev: the two calls (a) replaces;
  (c) ldpc_sim_extract_messages alone: the yardstick, a kernel older than the CRC, which reads the same k bytes a frame as (a) and
      writes k bytes a frame where (a) writes one.
HIP events around each version, 3 warm-up runs, then 10 timed runs with the versions alternating inside a repetition; median, min and
max.  The flags of (a) and (b) are compared at the timed size.  Every other frame carries a valid CRC'd message, the others random bits.
DECODE=1 also times the headline decoder (50 iterations of min-sum at 2 dB on frames of this source) on the same batch, for the share."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecc_ldpc_amd as E  # noqa: E402

B = int(os.environ.get("CRC_BATCH", "65536"))
REPS, WARM = 10, 3
E.init(0)
dev = torch.device("cuda", 0)


def say(*a):
    print(" ".join(str(x) for x in a), flush=True)


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


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


ecc = E.ECC(os.path.join(ROOT, "codes"), "ldpc/hip-minsum/jpl.4096.4.5/50/4/5", max_batch=B)
sim, N, k = ecc.sim, ecc.unpunctured_length, ecc.sim.k
w = E.Crc.builtin_params("crc24a")[0]
crc = E.Crc.builtin("crc24a", k - w)
g = torch.Generator(device=dev).manual_seed(19)
bits = torch.randint(0, 2, (B, N), device=dev, generator=g, dtype=torch.uint8)
msg = torch.empty((B, k), dtype=torch.uint8, device=dev)
ok_a = torch.full((B,), 7, dtype=torch.uint8, device=dev)
ok_b = torch.full((B,), 7, dtype=torch.uint8, device=dev)
# every other frame: a valid message at the message positions (0 .. k - 1 on this source)
sim.extract_messages(B, bits.data_ptr(), msg.data_ptr(), "bytes")
crc.attach(B, msg.data_ptr(), "bytes")
torch.cuda.synchronize()
bits[::2, :k] = msg[::2]
torch.cuda.synchronize()


def two():
    sim.extract_messages(B, bits.data_ptr(), msg.data_ptr(), "bytes")
    crc.check(B, msg.data_ptr(), ok_b.data_ptr(), "bytes")


say(f"jpl.4096.4.5 decoded bytes [{B}][{N}], k = {k} = {k - w} + {w} (crc24a), {REPS} timed runs after {WARM} warm-up runs, versions alternating inside a repetition; "
    "HIP events around each version")
odd = torch.empty(B * N + 1, dtype=torch.uint8, device=dev)[1:]        # the same bytes from an odd address: the byte-a-lane instance
odd.copy_(bits.reshape(-1))
ok_o = torch.full((B,), 7, dtype=torch.uint8, device=dev)
res = timed({"(a) ldpc_sim_crc_check": lambda: sim.crc_check(crc, B, bits.data_ptr(), ok_a.data_ptr(), "bytes"),
             "(a1) the same from base + 1: a byte a lane": lambda: sim.crc_check(crc, B, odd.data_ptr(), ok_o.data_ptr(), "bytes"),
             "(b) ldpc_sim_extract_messages + ldpc_crc_check_dev": two,
             "(c) ldpc_sim_extract_messages alone (the yardstick)": lambda: sim.extract_messages(B, bits.data_ptr(), msg.data_ptr(), "bytes")})
torch.cuda.synchronize()
a, b = ok_a.cpu(), ok_b.cpu()
say(f"flags of (a) and (b) equal: {bool(torch.equal(a, b))}, of (a) and (a1): {bool(torch.equal(a, ok_o.cpu()))}; passes: {int(a.sum())} of {B} (every other frame carries a valid message: {bool(a[::2].all())})")
for name, v in res.items():
    med, lo, hi = stats(v)
    say(f"{name:54s} median {med:9.3f} ms   min {lo:9.3f}   max {hi:9.3f}   ({len(v)} runs)")
(ma, _, _), (mc, lc, hc) = stats(res["(a) ldpc_sim_crc_check"]), stats(res["(c) ldpc_sim_extract_messages alone (the yardstick)"])
say(f"(a) median - (c) median = {ma - mc:+.3f} ms; the spread of (c), max - min = {hc - lc:.3f} ms: (a) {'within' if ma - mc <= hc - lc else 'OUTSIDE'} it")
say(f"(a) reads {B * k / 1e6:.1f} MB of decoded bytes in {ma:.3f} ms: {B * k / ma / 1e6:.1f} GB/s")
if os.environ.get("DECODE") == "1":
    llr = torch.empty((B, N), dtype=torch.float32, device=dev)
    out = torch.empty((B, N), dtype=torch.uint8, device=dev)
    sim.generate(1, 0, B, 2.0, llr.data_ptr(), None, None)
    torch.cuda.synchronize()
    dec = ecc.decoder

    def decode():
        dec.decode_batch_dev(llr.data_ptr(), out.data_ptr(), B, 50, None, None, None)
        dec.synchronize()

    ts = []
    for rep in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        decode()
        e1.record()
        e1.synchronize()
        if rep >= WARM:
            ts.append(e0.elapsed_time(e1))
    md, ld, hd = stats(ts)
    say(f"{dec.kernel_name}: decode of the same batch at 2 dB, 50 iterations: median {md:9.3f} ms   min {ld:9.3f}   max {hd:9.3f}; (a) is {100 * ma / md:.2f} % of it")
crc.close(); ecc.close()
