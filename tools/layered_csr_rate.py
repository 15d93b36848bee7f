"""Decode rate of the on-chip layered min-sum kernel for any H (csrc/layered_csr.hip) next to the kernels a user had before it.

  (a) layered_csr, fp16 lam on-chip, on the DVB-S2-structured natural-order code (tests/dvbs2_natural.py) in the order
      ldpc_csr_layer_order proposes, at 1.5 / 2.0 / 2.5 dB;
  (b) flood.hip, f32 layered (path="flood"), same code, layers and frames;
  (c) layered_lds.hip on codes/dvbs2like.64800.1.2 (the quasi-cyclic reference);
  and layered_csr on codes/1920.1280.3.303 in file order and in helper order (with (b) for it).
Decoded-information Gbit/s = frames x k / kernel time (HIP events around the decode kernel, the median of the timed launches);
frames: the all-zero codeword + AWGN, f32 LLRs generated on the device.

usage: python tools/layered_csr_rate.py [--frames 16384] [--reps 3] [--quick]"""
from __future__ import annotations

import argparse
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ecc_ldpc_amd as E  # noqa: E402
from oracle import channel, formats  # noqa: E402
from tests import dvbs2_natural  # noqa: E402

ASM = os.path.join(ROOT, "ecc_ldpc_amd", "build", "layered_csr-hip-amdgcn-amd-amdhsa-gfx950.s")


def kernel_resources(dclass):
    """(vgpr_count, private_segment_fixed_size) of layered_csr_kernel<dclass> from the device assembly the build keeps"""
    try:
        text = open(ASM).read()
    except OSError:
        return None, None
    m = re.search(r"\.name:\s+_ZN4ldpc18layered_csr_kernelILi%dE\S*\n((?:\s+\.[a-z_]+:.*\n)+)" % dclass, text)
    if not m:
        return None, None
    f = dict(re.findall(r"\.([a-z_]+):\s+(\d+)", m.group(1)))
    return int(f.get("vgpr_count", -1)), int(f.get("private_segment_fixed_size", -1))


def device_frames(F, N, k, db, seed):
    s2 = channel.sigma2(db, k, N)
    g = torch.Generator(device="cuda").manual_seed(seed)
    y = -1.0 + torch.randn((F, N), generator=g, device="cuda", dtype=torch.float32) * float(np.sqrt(s2))
    return (2.0 / s2) * y


def rate(dec, llr, k, max_iters, reps):
    F, N = llr.shape
    bits = torch.empty((F, N), dtype=torch.uint8, device="cuda")
    iters = torch.empty(F, dtype=torch.int32, device="cuda")
    conv = torch.empty(F, dtype=torch.uint8, device="cuda")
    dec.set_timing(True)
    dec.decode_batch_dev(llr.data_ptr(), bits.data_ptr(), F, max_iters, iters.data_ptr(), conv.data_ptr())   # warm-up
    dec.synchronize()
    dec.kernel_time()
    times = []
    for _ in range(reps):
        dec.decode_batch_dev(llr.data_ptr(), bits.data_ptr(), F, max_iters, iters.data_ptr(), conv.data_ptr())
        dec.synchronize()
        n, ms = dec.kernel_time()
        times.append(ms / max(n, 1))
    ms = statistics.median(times)
    return {"ms": ms, "gbps": F * k / (ms * 1e-3) / 1e9, "sweeps": float(iters.float().mean()), "conv": float(conv.float().mean()),
            "bits": bits}


def describe(dec, lds=None):
    t, f = dec.kernel_geometry
    s = f"{dec.kernel_name} path={dec.path} threads/wg={t} frames/wg={f}"
    m = re.search(r"layered_csr_kernel<(\d+)>", dec.kernel_name)
    if m:
        v, sc = kernel_resources(int(m.group(1)))
        s += f" LDS={lds} B VGPRs={v} scratch={sc} B"
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-iters", type=int, default=50)
    ap.add_argument("--quick", action="store_true", help="(a) at 2 dB only (profiler runs)")
    a = ap.parse_args()
    E.init(0)
    F, MI = a.frames, a.max_iters
    out = lambda s: print(s, flush=True)   # noqa: E731
    out(f"# layered_csr rate: {F} frames, {MI} sweeps at most, {a.reps} timed launches (median), f32 LLRs on the device")

    # ---- DVB-S2-structured natural-order code, helper order
    rp, ci = dvbs2_natural.csr()
    N, K = dvbs2_natural.N, dvbs2_natural.K
    perm, lp = E.Code.csr_layer_order(rp, ci, N)
    prp, pci = E.Code.permute_rows(rp, ci, perm)
    lds = ((2 * N + 15) // 16) * 16 + 32
    t0 = time.time()
    code = E.Code.from_csr(prp, pci, N)
    code.set_layers(lp)
    dec = E.Decoder(code, "min", "f16", F, schedule="layered")
    out(f"dvbs2-natural N={N} M={N - K} E={len(ci)} layers (helper order)={len(lp) - 1} rows/layer {np.diff(lp).min()}..{np.diff(lp).max()}"
        f" (context {time.time() - t0:.1f} s)")
    out(f"  (a) {describe(dec, lds)}")
    ra = {}
    for db in ((2.0,) if a.quick else (1.5, 2.0, 2.5)):
        llr = device_frames(F, N, K, db, 17)
        r = rate(dec, llr, K, MI, a.reps)
        ra[db] = r
        out(f"  (a) {db:.1f} dB: {r['gbps']:.2f} Gbit/s  {r['ms']:.1f} ms  sweeps {r['sweeps']:.2f}  converged {r['conv']:.4f}")
        if db == 2.0 and not a.quick:
            fl = E.Decoder(code, "min", "f32", F, schedule="layered", path="flood")
            out(f"  (b) {describe(fl)}")
            rb = rate(fl, llr, K, MI, a.reps)
            out(f"  (b) {db:.1f} dB: {rb['gbps']:.2f} Gbit/s  {rb['ms']:.1f} ms  sweeps {rb['sweeps']:.2f}  converged {rb['conv']:.4f}")
            out(f"  (a)/(b) at 2.0 dB: {r['gbps'] / rb['gbps']:.2f}x")
            fl.close()
            del rb
        del llr, r["bits"]
        torch.cuda.empty_cache()
    dec.close()
    if a.quick:
        return

    # ---- (c) the quasi-cyclic reference
    sz, rows = formats.read_qc(open(os.path.join(ROOT, "codes", "dvbs2like.64800.1.2", "H.q")).read())
    qc = E.Code.from_qc(sz, formats.qc_offsets(sz, rows))
    dq = E.Decoder(qc, "min", "f16", F, schedule="layered")
    out(f"dvbs2like.64800.1.2 (quasi-cyclic, block rows as layers)\n  (c) {describe(dq)}")
    for db in (1.5, 2.0, 2.5):
        llr = device_frames(F, N, K, db, 17)
        r = rate(dq, llr, K, MI, a.reps)
        out(f"  (c) {db:.1f} dB: {r['gbps']:.2f} Gbit/s  {r['ms']:.1f} ms  sweeps {r['sweeps']:.2f}  converged {r['conv']:.4f}")
        del llr, r["bits"]
    dq.close()
    torch.cuda.empty_cache()

    # ---- 1920.1280.3.303 (MacKay), file order and helper order
    H = formats.read_alist_mackay(open(os.path.join(ROOT, "codes", "1920.1280.3.303")).read())
    Hm, Hn = H.shape
    rp3 = np.concatenate([[0], np.cumsum(H.sum(1))]).astype(np.int32)
    ci3 = np.nonzero(H)[1].astype(np.int32)
    k3 = 640
    llr = device_frames(F, Hn, k3, 2.0, 23)
    p3, lp3 = E.Code.csr_layer_order(rp3, ci3, Hn)
    prp3, pci3 = E.Code.permute_rows(rp3, ci3, p3)
    out(f"1920.1280.3.303 N={Hn} M={Hm} (rate 1/3, k = {k3}) at 2.0 dB")
    for label, (r_, c_, l_) in (("file order", (rp3, ci3, None)), (f"helper order ({len(lp3) - 1} layers)", (prp3, pci3, lp3))):
        c3 = E.Code.from_csr(r_, c_, Hn)
        if l_ is not None:
            c3.set_layers(l_)
        d3 = E.Decoder(c3, "min", "f16", F, schedule="layered")
        r = rate(d3, llr, k3, MI, a.reps)
        out(f"  layered_csr, {label}: {r['gbps']:.2f} Gbit/s  {r['ms']:.2f} ms  sweeps {r['sweeps']:.2f}  converged {r['conv']:.4f}\n    {describe(d3, ((2 * Hn + 15) // 16) * 16 + 32)}")
        f3 = E.Decoder(c3, "min", "f32", F, schedule="layered", path="flood")
        r = rate(f3, llr, k3, MI, a.reps)
        out(f"  flood.hip f32 layered, {label}: {r['gbps']:.2f} Gbit/s  {r['ms']:.2f} ms  sweeps {r['sweeps']:.2f}  converged {r['conv']:.4f}")
        d3.close(); f3.close()
    E.close_all()


if __name__ == "__main__":
    main()
