#!/usr/bin/env python3
"""tools/bch_rate.py -- what the BCH outer code costs (csrc/bch.hip; profiles/bch_rate.txt).  n = 32 400 = the message length of the long
code (codes/dvbs2like.64800.1.2), m = 16, t = 12 (p = 192, a table entry of 6 words), batch 16 384 (BCH_BATCH overrides), rows in bytes
and packed:
  (a) ldpc_bch_encode_dev;
  (b) ldpc_bch_decode_dev on clean frames: the remainder alone -- what almost every frame costs after LDPC decoding;
  (c) ldpc_bch_decode_dev on frames that carry t errors each: remainder, syndromes, Berlekamp-Massey, Chien search and the flips.  The
      frames are restored from a copy before every run, outside the timed window.
HIP events around each call, 3 warm-up runs, then 10 timed runs with the versions alternating inside a repetition; median, min and max.
The results are checked at the timed size: (b) gives nerr = 0 everywhere, (c) gives nerr = t everywhere and the rows sent.
The numbers go to --out (default profiles/bch_rate.txt) as well as to the terminal."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecc_ldpc_amd as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bch_rate.txt"))
ap.add_argument("--n", type=int, default=32400)
args = ap.parse_args()
B = int(os.environ.get("BCH_BATCH", "16384"))
REPS, WARM = 10, 3
E.init(0)
dev = torch.device("cuda", 0)
lines = []


def say(*a):
    lines.append(" ".join(str(x) for x in a))
    print(lines[-1], flush=True)


def timed(fns):
    """alternating: every repetition runs each (prepare, fn) once, fn between two events -> {name: [ms]}"""
    res = {k: [] for k in fns}
    for rep in range(WARM + REPS):
        for k, (prepare, fn) in fns.items():
            if prepare:
                prepare()
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


def pack(bits, nbytes):
    """bits [B][n] 0 / 1 on the device -> packed rows [B][nbytes], bit i in byte i / 8 at bit i % 8"""
    out = torch.zeros((bits.shape[0], nbytes), dtype=torch.uint8, device=dev)
    wts = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=dev)
    for lo in range(0, bits.shape[0], 1024):
        b = torch.zeros((min(1024, bits.shape[0] - lo), nbytes * 8), dtype=torch.int32, device=dev)
        b[:, :bits.shape[1]] = bits[lo:lo + 1024]
        out[lo:lo + 1024] = (b.view(-1, nbytes, 8) * wts).sum(-1).to(torch.uint8)
    return out


n = args.n
bch = E.Bch.builtin("m16t12", n)
m, poly, t, _, k = bch.params()
p, PB = bch.p, 4 * ((n + 31) // 32)
g = torch.Generator(device=dev).manual_seed(23)
clean = torch.randint(0, 2, (B, n), device=dev, generator=g, dtype=torch.uint8)
nerr = torch.full((B,), -7, dtype=torch.int32, device=dev)
bch.encode(B, clean.data_ptr(), "bytes")
torch.cuda.synchronize()
# t errors a frame, one in each of t equal strata: distinct positions
at = torch.arange(t, device=dev)[None, :] * (n // t) + torch.randint(0, n // t, (B, t), device=dev, generator=g)
dirty = clean.clone()
dirty.scatter_(1, at, dirty.gather(1, at) ^ 1)
assert int((dirty != clean).sum()) == B * t
clean_p, dirty_p = pack(clean, PB), pack(dirty, PB)
work, work_p = clean.clone(), clean_p.clone()
torch.cuda.synchronize()

say(f"BCH m = {m}, prim_poly = {poly:#x}, t = {t}: n = {n}, k = {k}, p = {p} ({(p + 31) // 32} table words); batch {B}; rows of {n} bytes or {PB} packed bytes; "
    f"{REPS} timed runs after {WARM} warm-up runs, versions alternating inside a repetition; HIP events around each call")
res = timed({
    "(a) encode, bytes": (None, lambda: bch.encode(B, work.data_ptr(), "bytes")),
    "(a) encode, packed": (None, lambda: bch.encode(B, work_p.data_ptr(), "packed")),
    "(b) decode of clean frames, bytes": (None, lambda: bch.decode(B, clean.data_ptr(), nerr.data_ptr(), "bytes")),
    "(b) decode of clean frames, packed": (None, lambda: bch.decode(B, clean_p.data_ptr(), nerr.data_ptr(), "packed")),
    f"(c) decode of frames with {t} errors, bytes": (lambda: work.copy_(dirty), lambda: bch.decode(B, work.data_ptr(), nerr.data_ptr(), "bytes")),
    f"(c) decode of frames with {t} errors, packed": (lambda: work_p.copy_(dirty_p), lambda: bch.decode(B, work_p.data_ptr(), nerr.data_ptr(), "packed")),
})
torch.cuda.synchronize()
# the results at the timed size
ok = True
for fmt, c, d_, w in (("bytes", clean, dirty, work), ("packed", clean_p, dirty_p, work_p)):
    w.copy_(c)
    bch.encode(B, w.data_ptr(), fmt)
    torch.cuda.synchronize()
    same = bool(torch.equal(w, c))
    nerr.fill_(-7)
    bch.decode(B, w.data_ptr(), nerr.data_ptr(), fmt)
    torch.cuda.synchronize()
    zero = bool((nerr == 0).all()) and bool(torch.equal(w, c))
    w.copy_(d_)
    nerr.fill_(-7)
    bch.decode(B, w.data_ptr(), nerr.data_ptr(), fmt)
    torch.cuda.synchronize()
    fixed = bool((nerr == t).all()) and bool(torch.equal(w, c))
    say(f"{fmt}: encoding a codeword again leaves it: {same}; clean frames give nerr = 0 and stay: {zero}; frames with {t} errors give nerr = {t} and the rows sent: {fixed}")
    ok = ok and same and zero and fixed
for name, v in res.items():
    med, lo, hi = stats(v)
    say(f"{name:48s} median {med:9.3f} ms   min {lo:9.3f}   max {hi:9.3f}   ({len(v)} runs)")
mb = stats(res["(b) decode of clean frames, bytes"])[0]
words = (p + 31) // 32
say(f"(b) bytes reads {B * n / 1e6:.1f} MB of rows in {mb:.3f} ms: {B * n / mb / 1e6:.1f} GB/s of row bytes, beside {words * 4} table bytes a row bit "
    f"({B * n * words * 4 / mb / 1e6:.1f} GB/s from the {n * words * 4 / 1024:.0f} KiB table, which every frame reads whole)")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
bch.close()
sys.exit(0 if ok else 1)
