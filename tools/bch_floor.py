#!/usr/bin/env python3
"""tools/bch_floor.py -- what a BCH outer code does to the errors an LDPC decode leaves (csrc/bch.hip).  On a source of the caller's
choice (default jpl.1024.4.5 min-sum; --code dvbs2like.64800.1.2 for the long code, layered fp16) and over a few Eb/N0:
  payload -> ldpc_bch_encode_dev -> ldpc_sim_generate_from -> LDPC decode -> ldpc_sim_bch_decode -> ldpc_sim_extract_messages
and the frame and bit error rate of the k PAYLOAD bits before and after the outer decode, with the frames counted as
  clean        nerr = 0 and the row is the one sent          corrected    nerr > 0 and the row is the one sent
  failed       nerr = -1 (more than t errors, detected)      miscorrected nerr >= 0 and the row is another codeword than the one sent
The BCH code is (m, prim_poly, t) shortened to n = the source's message length.  The information rate drops by k / n, so each point is
printed under both conventions: Eb/N0 of the LDPC message bits (what ldpc_sim_generate_from takes) and Eb/N0 of the payload bits,
which is higher by 10 log10(n / k) dB.
A source without an encoder (the long code: H only, and neither triangular nor small enough for the systematic form) can send the
all-zero codeword alone.  The zero row is a BCH codeword and every decoder here is symmetric in the codeword sent, so the tool then sends
the zero payload, still through ldpc_bch_encode_dev, and draws the frames with ldpc_sim_generate; it says so in its first line."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecc_ldpc_amd as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--code", default="jpl.1024.4.5")
ap.add_argument("--name", default=None, help="the decoder's full name; default: min-sum for --code (layered fp16 for the long code)")
ap.add_argument("--ebn0", type=float, nargs="+", default=None, help="Eb/N0 of the LDPC message bits, dB")
ap.add_argument("--frames", type=int, default=65536)
ap.add_argument("--batch", type=int, default=8192)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--m", type=int, default=None)
ap.add_argument("--prim-poly", type=lambda s: int(s, 0), default=None)
ap.add_argument("--t", type=int, default=None)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()

long_code = args.code.startswith("dvbs2like")
name = args.name or (f"ldpc/hip-minsum-layered-f16/{args.code}/{args.iters}" if long_code else f"ldpc/hip-minsum/{args.code}/{args.iters}/4/5")
f16 = "-f16" in name
ebn0s = args.ebn0 or ([2.0, 2.2, 2.4] if long_code else [3.0, 3.5, 4.0])
B = args.batch
E.init(0)
dev = torch.device("cuda", 0)
ecc = E.ECC(os.path.join(ROOT, "codes"), name, max_batch=B)
dec, N = ecc.decoder, ecc.unpunctured_length
sim = ecc.sim
zero = sim.encoder == "none"
n = sim.k
m, poly, t = E.Bch.builtin_params("m16t12") if n > 16383 else E.Bch.builtin_params("m14t12") if n > 2047 else (11, 0x805, 4)
m, poly, t = args.m or m, args.prim_poly or poly, args.t or t
bch = E.Bch(m, poly, t, n)
k, p = bch.k, bch.p
mp = torch.from_numpy(sim.positions()[0].astype("int64")).to(dev)
shift = 10 * math.log10(n / k)
print(f"{name}: N = {N}, LDPC message length n = {n}; BCH m = {m}, prim_poly = {poly:#x}, t = {t}: k = {k} payload bits, p = {p}; "
      f"rate k/n = {k / n:.4f}, Eb/N0(payload) = Eb/N0(LDPC message) + {shift:.3f} dB; {args.frames} frames a point in batches of {B}, {args.iters} iterations"
      + ("; the source has no encoder: the zero payload is sent" if zero else ""), flush=True)

msg = torch.empty((B, n), dtype=torch.uint8, device=dev)
llr = torch.empty((B, N), dtype=torch.float16 if f16 else torch.float32, device=dev)
bits = torch.empty((B, N), dtype=torch.uint8, device=dev)
nerr = torch.empty((B,), dtype=torch.int32, device=dev)
g = torch.Generator(device=dev).manual_seed(args.seed)
for db in ebn0s:
    tot = dict(frames=0, fe0=0, be0=0, fe1=0, be1=0, clean=0, corrected=0, failed=0, miscorrected=0)
    first = 0
    while tot["frames"] < args.frames:
        if zero:
            msg.zero_()
        else:
            msg.copy_(torch.randint(0, 2, (B, n), device=dev, generator=g, dtype=torch.uint8))
        bch.encode(B, msg.data_ptr(), "bytes")
        torch.cuda.synchronize()
        if zero:
            sim.generate(args.seed, first, B, db, llr.data_ptr(), None, None, llr_f16=f16)
        else:
            sim.generate_from(args.seed, first, B, db, msg.data_ptr(), llr.data_ptr(), "bytes", None, llr_f16=f16)
        torch.cuda.synchronize()                                             # the context decodes on its own stream
        dec.decode_batch_dev(llr.data_ptr(), bits.data_ptr(), B, args.iters, None, None, None, llr_f16=f16)
        dec.synchronize()
        before = (bits[:, mp] & 1) != msg
        sim.bch_decode(bch, B, bits.data_ptr(), nerr.data_ptr(), "bytes")
        torch.cuda.synchronize()
        after = (bits[:, mp] & 1) != msg
        right = ~after.any(1)
        tot["frames"] += B
        tot["fe0"] += int(before[:, :k].any(1).sum()); tot["be0"] += int(before[:, :k].sum())
        tot["fe1"] += int(after[:, :k].any(1).sum()); tot["be1"] += int(after[:, :k].sum())
        tot["clean"] += int(((nerr == 0) & right).sum()); tot["corrected"] += int(((nerr > 0) & right).sum())
        tot["failed"] += int((nerr < 0).sum()); tot["miscorrected"] += int(((nerr >= 0) & ~right).sum())
        first += B
    F = tot["frames"]
    print(f"Eb/N0 {db:5.2f} dB (LDPC message) = {db + shift:5.2f} dB (payload): {F} frames;  before: FER {tot['fe0'] / F:.3e} BER {tot['be0'] / (F * k):.3e};  "
          f"after: FER {tot['fe1'] / F:.3e} BER {tot['be1'] / (F * k):.3e};  clean {tot['clean']}, corrected {tot['corrected']}, failed {tot['failed']}, "
          f"miscorrected {tot['miscorrected']}", flush=True)
bch.close()
ecc.close()
