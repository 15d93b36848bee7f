"""Decode rate of the on-chip layered min-sum kernel for any H (csrc/layered_csr.hip) next to the kernels a user had before it.

  (a) layered_csr, fp16 lam on-chip, on the DVB-S2-structured natural-order code (tests/dvbs2_natural.py) in the order
      ldpc_csr_layer_order proposes, at 1.5 / 2.0 / 2.5 dB;
  (b) flood.hip, f32 layered (path="flood"), same code, layers and frames;
  (c) layered_lds.hip on codes/dvbs2like.64800.1.2 (the quasi-cyclic reference);
  and layered_csr on codes/1920.1280.3.303 in file order and in helper order (with (b) for it).
  --lam f32|f16|both: the f32-lam instances (layered_csr_kernel<D, float>, path="fused") next to the fp16-lam ones and flood.hip f32
  layered, on identical frames and layers, at 1.5 / 2.0 / 2.5 dB: codes/1920.1280.3.303 and the DVB-S2 short-frame structure
  (tests/dvbs2_short.py), both in helper order.  The legs of one point take turns launch by launch (warm-up launch first).
  --lam i8: the int8 fixed-point instances (LDPC_I8, layered_csr_kernel<D, signed char>, qscale 4) next to the fp16-lam ones on identical
  frames and layers, same method, on those two codes and on the N = 64 800 code of tests/dvbs2_natural.py: rate, workgroups per CU,
  threads, VGPRs, record bytes per sweep, and the frame / bit error rates and mean sweeps of both.  The int8 leg runs at the threads per
  workgroup the library chooses and, where that differs from the fp16 leg's, at those too (LDPC_LAYERED_CSR_THREADS).
  --cn-scale A [A ...] --cn-offset B [B ...]: the check-node rule (ldpc_ctx_config cn_scale / cn_offset), pair by pair (a single value of
  one list goes with every value of the other; 0.75 / 0 is the default rule): fp16 and int8 lam under each rule on identical frames and
  layers, same method, on tests/dvbs2_short.py and tests/dvbs2_natural.py at 1.5 / 2.0 / 2.5 dB -- rate, mean sweeps, converged share,
  frame and bit error rate per leg.  Nothing else is run.
  --codewords zero|random (the --lam i8 and --cn-scale / --cn-offset comparisons, which report error rates): zero, the default, transmits
  the all-zero codeword; random takes the codewords of random messages from the frame source's encoder from H (Sim(from_H=True).encode_batch)
  on the structures that qualify (the DVB-S2 ones), from its systematic form (Sim(systematic=True)) otherwise (1920.1280.3.303), and mirrors the SAME torch noise onto
  them, y = (2c - 1) + noise with the same generator and seed: a zero leg and a random leg differ only in the codeword.  FER / BER are
  counted against the transmitted codeword.
Decoded-information Gbit/s = frames x k / kernel time (HIP events around the decode kernel, the median of the timed launches);
frames: the all-zero codeword + AWGN unless --codewords random, f32 LLRs generated on the device.

  --soft: only the cost of the soft output (ldpc_decode_batch_dev_soft): on 1920.1280.3.303, for each lam cell, the context's plain decode and
      its soft decode (posterior, extrinsic; float32 and fp16 out) on the same frames, kernel time by HIP events
  --continue: only the cost of a continuing call (ldpc_decode_batch_dev_continue) from a reset state, with and without a soft output, against the
      soft call of the same context on the same frames, same method (profiles/r21_decode_continue.txt)
usage: python tools/layered_csr_rate.py [--frames 16384] [--reps 3] [--quick] [--lam f32|f16|both|i8 [--lam-only]] [--soft] [--continue] [--asm FILE]
                                        [--cn-scale A [A ...]] [--cn-offset B [B ...]] [--codewords zero|random] [--codes NAME [NAME ...]]
(profiles/r07_layered_csr_f32_rate.txt: --lam both --lam-only --reps 5; profiles/r09_layered_csr_i8_rate.txt: --lam i8 --lam-only --reps 5;
profiles/r10_layered_rule_ber.txt: --cn-scale 0.75 0.8125 0.875 1 1 --cn-offset 0 0 0 0.25 0.5 --reps 5;
profiles/r11_sparse_encoder.txt: --lam i8 --lam-only --codes dvbs2-short --codewords zero, then the same with --codewords random)"""
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
from tests import dvbs2_natural, dvbs2_short  # noqa: E402

ASM = os.path.join(ROOT, "ecc_ldpc_amd", "build", "layered_csr-hip-amdgcn-amd-amdhsa-gfx950.s")


def kernel_resources(dclass, lam="f16", rule=False):
    """(vgpr_count, private_segment_fixed_size) of layered_csr_kernel<dclass, lam cell type> from the device assembly the build keeps
    (the cell type is part of the mangled name: DF16_ = _Float16, f = float, a = signed char; rule: the Ruled<cell type> instance)"""
    try:
        text = open(ASM).read()
    except OSError:
        return None, None
    cell = {"f32": "f", "i8": "a"}.get(lam, "DF16_")
    m = re.search(r"\.name:\s+_ZN4ldpc18layered_csr_kernelILi%dE%sEE\S*\n((?:\s+\.[a-z_]+:.*\n)+)" % (dclass, "NS_5RuledI%sEE" % cell if rule else cell), text)
    if not m:
        return None, None
    f = dict(re.findall(r"\.([a-z_]+):\s+(\d+)", m.group(1)))
    return int(f.get("vgpr_count", -1)), int(f.get("private_segment_fixed_size", -1))


def device_frames(F, N, k, db, seed, cw=None):
    """cw: the transmitted codewords [F][N] (uint8, device), None = all-zero; the noise depends on (seed, shape) only"""
    s2 = channel.sigma2(db, k, N)
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = -1.0 if cw is None else 2.0 * cw.to(torch.float32) - 1.0
    y = x + torch.randn((F, N), generator=g, device="cuda", dtype=torch.float32) * float(np.sqrt(s2))
    llr = (2.0 / s2) * y
    torch.cuda.synchronize()     # the decoders run on their own stream: the frames are complete before the first launch reads them
    return llr


def transmitted(a, code, rp, ci, N, k, F, out):
    """--codewords random: the codewords [F][N] of random messages, from the encoder from H of `code` (rows rp, ci); None (all-zero)
    for --codewords zero and for an H that encoder refuses"""
    if a.codewords != "random":
        return None
    try:
        E.Code.csr_triangular_order(rp, ci, N)
        sim = E.Sim(code, k, N, from_H=True, max_batch=F)
    except E.LdpcError as e:
        try:                                                          # not accumulator-shaped: the systematic form of H
            sim = E.Sim(code, None, N, systematic=True, max_batch=F)
            assert sim.k == k, (sim.k, k)
        except E.LdpcError as e2:
            out(f"  all-zero codewords here: {e}; {e2}")
            return None
    cw = torch.empty((F, N), dtype=torch.uint8, device="cuda")
    sim.encode_batch(0xC0DE, 0, F, cw.data_ptr(), None, None)
    torch.cuda.synchronize()
    par = torch.from_numpy(sim.positions()[1].astype("int64")).cuda()
    out(f"  codewords of random messages ({sim.encoder} encoder from H), parity ones {float(cw[:, par].float().mean()):.4f}")
    sim.close()
    return cw


def error_rates(bits, cw):
    """-> (FER, BER) over the N codeword bits against the transmitted codeword"""
    err = bits if cw is None else bits ^ cw
    return float(err.any(dim=1).float().mean()), float(err.sum(dtype=torch.int64)) / err.numel()


def rate(dec, llr, k, max_iters, reps):
    return rates_in_turn([dec], llr, k, max_iters, reps)[0]


def describe(dec, lds=None):
    t, f = dec.kernel_geometry
    s = f"{dec.kernel_name} path={dec.path} threads/wg={t} frames/wg={f}"
    m = re.search(r"layered_csr_kernel<(\d+)(, float|, signed char)?>", dec.kernel_name)
    if m:
        v, sc = kernel_resources(int(m.group(1)), {", float": "f32", ", signed char": "i8"}.get(m.group(2), "f16"))
        s += f" LDS={lds} B VGPRs={v} scratch={sc} B"
    return s


def rates_in_turn(decs, llr, k, max_iters, reps):
    """several contexts on the same frames: a warm-up launch each, then `reps` timed launches each, taking turns (what else runs on the
    machine then falls on all legs alike).  -> per context: the median kernel time (HIP events) and its spread, the rate, and the mean
    sweeps, converged share and bits of its last launch"""
    F, N = llr.shape
    bits = torch.empty((F, N), dtype=torch.uint8, device="cuda")
    iters = torch.empty(F, dtype=torch.int32, device="cuda")
    conv = torch.empty(F, dtype=torch.uint8, device="cuda")
    times, stats = [[] for _ in decs], []
    for r in range(reps + 1):                                           # r == 0: warm-up
        for j, dec in enumerate(decs):
            dec.set_timing(True)
            dec.decode_batch_dev(llr.data_ptr(), bits.data_ptr(), F, max_iters, iters.data_ptr(), conv.data_ptr())
            dec.synchronize()
            n, ms = dec.kernel_time()
            if r:
                times[j].append(ms / max(n, 1))
            if r == reps:
                stats.append((float(iters.float().mean()), float(conv.float().mean()), bits.clone()))
    out = []
    for j in range(len(decs)):
        ms = statistics.median(times[j])
        out.append({"ms": ms, "min": min(times[j]), "max": max(times[j]), "gbps": F * k / (ms * 1e-3) / 1e9, "sweeps": stats[j][0],
                    "conv": stats[j][1], "bits": stats[j][2]})
    return out


def all_resources(out):
    """the six instances' registers and scratch, from the assembly the build keeps"""
    for lam in ("f16", "f32"):
        for d in (8, 20, 32):
            v, sc = kernel_resources(d, lam)
            out(f"#   layered_csr_kernel<{d}{', float' if lam == 'f32' else ''}>: VGPRs={v} scratch={sc} B")


def workgroups_per_cu(threads, lds, vgprs):
    """resident workgroups of one CU (4 SIMDs x 512 VGPRs, 2048 threads, 160 KB of LDS), from the launch geometry and the registers"""
    waves = threads // 64
    by_regs = (4 * (512 // (-(-vgprs // 8) * 8))) // waves if vgprs and vgprs > 0 else None
    return min(x for x in (160 * 1024 // lds, 2048 // threads, by_regs) if x is not None)


def i8_comparison(a, out):
    """int8 lam (LDPC_I8, qscale 4) / fp16 lam on identical frames and layers: rate and error rates"""
    F, MI = a.frames, a.max_iters
    H = formats.read_alist_mackay(open(os.path.join(ROOT, "codes", "1920.1280.3.303")).read())
    rp3 = np.concatenate([[0], np.cumsum(H.sum(1))]).astype(np.int32)
    ci3 = np.nonzero(H)[1].astype(np.int32)
    rps, cis = dvbs2_short.csr()
    rpn, cin = dvbs2_natural.csr()
    out(f"# int8 lam (LDPC_I8, qscale 4) next to fp16 lam (--lam i8): {F} frames, {MI} sweeps at most, {a.reps} timed launches per leg "
        f"(median [min..max]), legs alternating, f32 LLRs on the device ({'all-zero codeword' if a.codewords == 'zero' else 'codewords of random messages'} + AWGN), helper order; "
        "FER / BER over the N codeword bits of the last launch")
    for d in (8, 20, 32):
        for lam in ("f16", "i8"):
            v, sc = kernel_resources(d, lam)
            out(f"#   layered_csr_kernel<{d}{', signed char' if lam == 'i8' else ''}>: VGPRs={v} scratch={sc} B")
    for label, rp, ci, N, k, seed in (("1920.1280.3.303", rp3, ci3, H.shape[1], 640, 23), ("dvbs2-short", rps, cis, dvbs2_short.N, dvbs2_short.K, 29),
                                      ("dvbs2-natural", rpn, cin, dvbs2_natural.N, dvbs2_natural.K, 17)):
        if a.codes and label not in a.codes:
            continue
        M = len(rp) - 1
        perm, lp = E.Code.csr_layer_order(rp, ci, N)
        prp, pci = E.Code.permute_rows(rp, ci, perm)
        code = E.Code.from_csr(prp, pci, N)
        code.set_layers(lp)
        os.environ.pop("LDPC_LAYERED_CSR_THREADS", None)
        d16 = E.Decoder(code, "min", "f16", F, schedule="layered", path="fused")
        d8 = E.Decoder(code, "min", "i8", F, schedule="layered")
        legs = [("fp16 lam   ", d16, ((2 * N + 15) // 16) * 16 + 32, 24 * M), ("int8 lam   ", d8, ((N + 15) // 16) * 16 + 32, 16 * M)]
        t16, t8 = d16.kernel_geometry[0], d8.kernel_geometry[0]
        if t16 != t8:                                               # the int8 instance at the fp16 leg's threads per workgroup as well
            os.environ["LDPC_LAYERED_CSR_THREADS"] = str(t16)
            legs.append((f"int8 T={t16:<4d}", E.Decoder(code, "min", "i8", F, schedule="layered"), legs[1][2], 16 * M))
            os.environ.pop("LDPC_LAYERED_CSR_THREADS")
        out(f"{label} N={N} M={M} E={len(ci)} k={k} layers (helper order)={len(lp) - 1}")
        for name, dec, lds, rb in legs:
            m = re.search(r"layered_csr_kernel<(\d+)(, signed char)?>", dec.kernel_name)
            v, _ = kernel_resources(int(m.group(1)), "i8" if m.group(2) else "f16")
            out(f"  {name}: {describe(dec, lds)} workgroups/CU={workgroups_per_cu(dec.kernel_geometry[0], lds, v)} record bytes/sweep={rb}")
        cw = transmitted(a, code, prp, pci, N, k, F, out)
        for db in (1.5, 2.0, 2.5):
            llr = device_frames(F, N, k, db, seed, cw)
            res = rates_in_turn([d for _, d, _, _ in legs], llr, k, MI, a.reps)
            for (name, _, _, _), r in zip(legs, res):
                fer, ber = error_rates(r["bits"], cw)
                out(f"  {db:.1f} dB {name}: {r['gbps']:.2f} Gbit/s  {r['ms']:.2f} ms [{r['min']:.2f}..{r['max']:.2f}]  sweeps {r['sweeps']:.2f}  "
                    f"converged {r['conv']:.4f}  FER {fer:.4e}  BER {ber:.4e}")
            out(f"  {db:.1f} dB int8 / fp16 rate: {res[1]['gbps'] / res[0]['gbps']:.2f}x" +
                (f"  (int8 at {t16} threads: {res[2]['gbps'] / res[0]['gbps']:.2f}x; its bits equal the default int8 leg's: "
                 f"{bool(torch.equal(res[1]['bits'], res[2]['bits']))})" if len(legs) > 2 else ""))
            del llr, res
            torch.cuda.empty_cache()
        for _, dec, _, _ in legs:
            dec.close()


def rule_comparison(a, out):
    """the check-node rules of --cn-scale / --cn-offset, fp16 and int8 lam, on identical frames and layers: rate and error rates"""
    F, MI = a.frames, a.max_iters
    n = max(len(a.cn_scale), len(a.cn_offset))
    rules = list(zip(a.cn_scale * (n if len(a.cn_scale) == 1 else 1), a.cn_offset * (n if len(a.cn_offset) == 1 else 1)))
    assert len(rules) == n, "--cn-scale and --cn-offset: lists of one length, or one of them a single value"
    out(f"# check-node rules (--cn-scale / --cn-offset), |msg'| = max(scale * min - offset, 0): {F} frames, {MI} sweeps at most, {a.reps} timed "
        f"launches per leg (median [min..max]), legs alternating, f32 LLRs on the device ({'all-zero codeword' if a.codewords == 'zero' else 'codewords of random messages'} + AWGN), identical for every leg of "
        "a point, helper order; int8 lam at qscale 4; FER / BER over the N codeword bits of the last launch")
    if a.codewords == "zero":
            out("# CAVEAT: the tool transmits the all-zero codeword and hard(0) = 0, so an LLR that is exactly zero -- common in int8, rare in fp16 -- "
            "is decided in that codeword's favour.  On a toy (720, 360) code, mirroring the same noise onto random codewords raised the int8 bit "
            "error count at 2 dB by 10 % at qscale 4 (23 % at qscale 2) and barely moved the frame error count: the BERs below flatter int8 "
            "relative to fp16 by about that much (--codewords random removes the bias).")
    for d in (8, 20, 32):
        for lam in ("f16", "i8"):
            (v0, s0), (v1, s1) = kernel_resources(d, lam), kernel_resources(d, lam, rule=True)
            cell = "signed char" if lam == "i8" else "_Float16"
            out(f"#   layered_csr_kernel<{d}, {cell}>: VGPRs={v0} scratch={s0} B;  <{d}, Ruled<{cell}>>: VGPRs={v1} scratch={s1} B")
    rps, cis = dvbs2_short.csr()
    rpn, cin = dvbs2_natural.csr()
    for label, rp, ci, N, k, seed in (("dvbs2-short", rps, cis, dvbs2_short.N, dvbs2_short.K, 29), ("dvbs2-natural", rpn, cin, dvbs2_natural.N, dvbs2_natural.K, 17)):
        if a.codes and label not in a.codes:
            continue
        perm, lp = E.Code.csr_layer_order(rp, ci, N)
        prp, pci = E.Code.permute_rows(rp, ci, perm)
        code = E.Code.from_csr(prp, pci, N)
        code.set_layers(lp)
        legs = []
        for lam in ("f16", "i8"):
            for sc, off in rules:
                default = (sc, off) == (0.75, 0.0)
                dec = E.Decoder(code, "min", lam, F, schedule="layered", path="fused", cn_scale=None if default else sc, cn_offset=None if default else off)
                legs.append((f"{'fp16' if lam == 'f16' else 'int8'} ({dec.cn_scale:g}, {dec.cn_offset:g})", dec))
        out(f"{label} N={N} M={len(rp) - 1} E={len(ci)} k={k} layers (helper order)={len(lp) - 1}")
        for name, dec in legs:
            out(f"  {name:<22s}: {dec.kernel_name} threads/wg={dec.kernel_geometry[0]}")
        cw = transmitted(a, code, prp, pci, N, k, F, out)
        for db in (1.5, 2.0, 2.5):
            llr = device_frames(F, N, k, db, seed, cw)
            res = rates_in_turn([d for _, d in legs], llr, k, MI, a.reps)
            for (name, _), r in zip(legs, res):
                fer, ber = error_rates(r["bits"], cw)
                out(f"  {db:.1f} dB {name:<22s}: {r['gbps']:.2f} Gbit/s  {r['ms']:.2f} ms [{r['min']:.2f}..{r['max']:.2f}]  sweeps {r['sweeps']:.2f}  "
                    f"converged {r['conv']:.4f}  FER {fer:.4e}  BER {ber:.4e}")
            del llr, res
            torch.cuda.empty_cache()
        for _, dec in legs:
            dec.close()


def lam_comparison(a, out):
    """f32 lam / fp16 lam / flood.hip f32 layered on identical frames and layers"""
    F, MI = a.frames, a.max_iters
    H = formats.read_alist_mackay(open(os.path.join(ROOT, "codes", "1920.1280.3.303")).read())
    rp3 = np.concatenate([[0], np.cumsum(H.sum(1))]).astype(np.int32)
    ci3 = np.nonzero(H)[1].astype(np.int32)
    rps, cis = dvbs2_short.csr()
    out(f"# lam cell type comparison (--lam {a.lam}): {F} frames, {MI} sweeps at most, {a.reps} timed launches per leg (median [min..max]), "
        "legs alternating, f32 LLRs on the device, helper order")
    all_resources(out)
    for label, rp, ci, N, k, seed in (("1920.1280.3.303", rp3, ci3, H.shape[1], 640, 23), ("dvbs2-short", rps, cis, dvbs2_short.N, dvbs2_short.K, 29)):
        perm, lp = E.Code.csr_layer_order(rp, ci, N)
        prp, pci = E.Code.permute_rows(rp, ci, perm)
        code = E.Code.from_csr(prp, pci, N)
        code.set_layers(lp)
        legs = []
        if a.lam in ("f32", "both"):
            legs.append(("f32 lam ", E.Decoder(code, "min", "f32", F, schedule="layered", path="fused"), ((4 * N + 15) // 16) * 16 + 32))
        if a.lam in ("f16", "both"):
            legs.append(("fp16 lam", E.Decoder(code, "min", "f16", F, schedule="layered", path="fused"), ((2 * N + 15) // 16) * 16 + 32))
        legs.append(("flood   ", E.Decoder(code, "min", "f32", F, schedule="layered", path="flood"), None))
        out(f"{label} N={N} M={len(rp) - 1} E={len(ci)} k={k} layers (helper order)={len(lp) - 1}")
        for name, dec, lds in legs:
            out(f"  {name}: {describe(dec, lds)}")
        for db in (1.5, 2.0, 2.5):
            llr = device_frames(F, N, k, db, seed)
            res = rates_in_turn([d for _, d, _ in legs], llr, k, MI, a.reps)
            for (name, _, _), r in zip(legs, res):
                out(f"  {db:.1f} dB {name}: {r['gbps']:.2f} Gbit/s  {r['ms']:.2f} ms [{r['min']:.2f}..{r['max']:.2f}]  sweeps {r['sweeps']:.2f}  converged {r['conv']:.4f}")
            if a.lam in ("f32", "both"):
                same = bool(torch.equal(res[0]["bits"], res[-1]["bits"]))
                out(f"  {db:.1f} dB f32 lam / flood: {res[0]['gbps'] / res[-1]['gbps']:.2f}x  (decoded bits identical: {same})")
            del llr, res
            torch.cuda.empty_cache()
        for _, dec, _ in legs:
            dec.close()


def soft_comparison(a, out):
    """--soft: the cost of the soft output.  One context per lam cell on 1920.1280.3.303; the plain decode (layered_csr_kernel) and the
    soft decode (layered_csr_soft_kernel: posterior and extrinsic, float32 and fp16 out) on the same frames, HIP events around each call,
    the five legs in turn inside a repetition; the median of --reps repetitions after one warm-up"""
    from tests.helpers import load
    c = load("1920.1280.3.303")
    N, k, F, MI = c.N, c.k, a.frames, a.max_iters
    code = E.Code.from_csr(c.graph.row_ptr, c.graph.col_idx, N)
    out(f"# layered_csr soft output: 1920.1280.3.303, {F} frames, {MI} sweeps at most, all-zero codewords, {a.reps} timed repetitions (median), f32 LLRs on the device")
    legs = (("plain", None, None), ("posterior f32", "posterior", "f32"), ("extrinsic f32", "extrinsic", "f32"), ("posterior f16", "posterior", "f16"), ("extrinsic f16", "extrinsic", "f16"))
    for db in (2.0, 4.0):
        llr = device_frames(F, N, k, db, 20)
        bits = torch.empty((F, N), dtype=torch.uint8, device="cuda")
        iters = torch.empty(F, dtype=torch.int32, device="cuda")
        soft = torch.empty((F, N), dtype=torch.float32, device="cuda")
        for cell in ("f16", "f32", "i8"):
            dec = E.Decoder(code, "min", cell, F, schedule="layered", path="fused")
            ms = {n: [] for n, _, _ in legs}
            for rep in range(1 + a.reps):
                for n, kind, fmt in legs:
                    torch.cuda.synchronize()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    dec.set_timing(True)
                    if kind is None:
                        dec.decode_batch_dev(llr.data_ptr(), bits.data_ptr(), F, MI, iters.data_ptr())
                    else:
                        dec.decode_batch_dev_soft(llr.data_ptr(), bits.data_ptr(), soft.data_ptr(), F, MI, kind, fmt, 0.0, iters.data_ptr())
                    dec.synchronize()
                    if rep:
                        ms[n].append(dec.kernel_time()[1])
                    else:
                        dec.kernel_time()
            base = float(np.median(ms["plain"]))
            out(f"  {db} dB  cell {cell:3s}  mean sweeps {float(iters.float().mean()):5.2f}  " + "  ".join(f"{n} {float(np.median(v)):7.3f} ms ({float(np.median(v)) / base:4.2f}x)" for n, v in ms.items())
                + f"   [{dec.kernel_name}]")
            dec.close()
    code.close()


def continue_comparison(a, out):
    """--continue: the cost of a continuing call (ldpc_decode_batch_dev_continue) from a reset state against the soft call on the same frames.
    One context per lam cell on 1920.1280.3.303; layered_csr_soft_kernel (extrinsic, float32 out), layered_csr_cont_kernel with the same
    output, and the latter without a soft output; the state is reset before every continuing call, outside the timed bracket; HIP events
    around each kernel, the legs in turn inside a repetition; the median of --reps repetitions after one warm-up"""
    from tests.helpers import load
    c = load("1920.1280.3.303")
    N, k, F, MI = c.N, c.k, a.frames, a.max_iters
    code = E.Code.from_csr(c.graph.row_ptr, c.graph.col_idx, N)
    out(f"# layered_csr continuing decode from a reset state: 1920.1280.3.303, {F} frames, {MI} sweeps at most, all-zero codewords, {a.reps} timed repetitions (median), f32 LLRs on the device")
    legs = ("soft extrinsic f32", "continue extrinsic f32", "continue, no soft output")
    for db in (2.0, 4.0):
        llr = device_frames(F, N, k, db, 20)
        bits = [torch.empty((F, N), dtype=torch.uint8, device="cuda") for _ in legs]
        iters = [torch.empty(F, dtype=torch.int32, device="cuda") for _ in legs]
        conv = [torch.empty(F, dtype=torch.uint8, device="cuda") for _ in legs]
        soft = [torch.empty((F, N), dtype=torch.float32, device="cuda") for _ in range(2)]
        for cell in ("f16", "f32", "i8"):
            dec = E.Decoder(code, "min", cell, F, schedule="layered", path="fused")
            state = E.DecodeState(dec, F)
            ms = {n: [] for n in legs}
            for rep in range(1 + a.reps):
                for j, n in enumerate(legs):
                    if j:
                        state.reset()
                        dec.synchronize()
                    torch.cuda.synchronize()
                    dec.set_timing(True)
                    if j == 0:
                        dec.decode_batch_dev_soft(llr.data_ptr(), bits[0].data_ptr(), soft[0].data_ptr(), F, MI, "extrinsic", "f32", 0.0, iters[0].data_ptr(), conv[0].data_ptr())
                    else:
                        dec.decode_batch_dev_continue(state, llr.data_ptr(), bits[j].data_ptr(), F, MI, soft[1].data_ptr() if j == 1 else None, "extrinsic", "f32", 0.0, iters[j].data_ptr(),
                                                      conv[j].data_ptr())
                    dec.synchronize()
                    if rep:
                        ms[n].append(dec.kernel_time()[1])
                    else:
                        dec.kernel_time()
            same = bool(all(torch.equal(x[0], x[j]) for x in (bits, iters, conv) for j in (1, 2)) and torch.equal(soft[0].view(torch.int32), soft[1].view(torch.int32)))
            base = float(np.median(ms[legs[0]]))
            out(f"  {db} dB  cell {cell:3s}  mean sweeps {float(iters[0].float().mean()):5.2f}  " + "  ".join(f"{n} {float(np.median(v)):7.3f} ms ({float(np.median(v)) / base:4.2f}x)" for n, v in ms.items())
                + f"   state {state.nbytes / F:.0f} B/frame  bits, sweeps, flags and soft output identical: {same}   [{dec.kernel_name}]")
            state.close()
            dec.close()
    code.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-iters", type=int, default=50)
    ap.add_argument("--quick", action="store_true", help="(a) at 2 dB only (profiler runs)")
    ap.add_argument("--lam", choices=("f32", "f16", "both", "i8"), help="add the lam cell type comparison with these on-chip legs (i8: int8 next to fp16)")
    ap.add_argument("--lam-only", action="store_true", help="only the --lam comparison")
    ap.add_argument("--cn-scale", type=float, nargs="+", help="check-node rule comparison: the scales (0.75: the default)")
    ap.add_argument("--cn-offset", type=float, nargs="+", help="check-node rule comparison: the offsets, in LLR units (0: none)")
    ap.add_argument("--codewords", choices=("zero", "random"), default="zero",
                    help="what the error-rate comparisons transmit: the all-zero codeword, or codewords of random messages (encoder from H) under the same noise")
    ap.add_argument("--codes", nargs="+", choices=("1920.1280.3.303", "dvbs2-short", "dvbs2-natural"),
                    help="the --lam i8 and check-node rule comparisons on these codes only (default: all of theirs)")
    ap.add_argument("--soft", action="store_true", help="only the soft-output comparison: a soft decode against the same context's plain decode")
    ap.add_argument("--continue", dest="cont", action="store_true", help="only the continuing-decode comparison: a continuing call from a reset state against the same context's soft call")
    ap.add_argument("--asm", help="the device assembly of layered_csr.hip, where the build directory's copy is not at hand")
    a = ap.parse_args()
    if a.asm:
        global ASM
        ASM = a.asm
    E.init(0)
    F, MI = a.frames, a.max_iters
    out = lambda s: print(s, flush=True)   # noqa: E731
    if a.soft:
        soft_comparison(a, out)
        E.close_all()
        return
    if a.cont:
        continue_comparison(a, out)
        E.close_all()
        return
    if a.cn_scale or a.cn_offset:
        a.cn_scale, a.cn_offset = a.cn_scale or [0.75], a.cn_offset or [0.0]
        rule_comparison(a, out)
        E.close_all()
        return
    if a.lam_only:
        a.lam = a.lam or "both"
        (i8_comparison if a.lam == "i8" else lam_comparison)(a, out)
        E.close_all()
        return
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
    if a.lam:
        (i8_comparison if a.lam == "i8" else lam_comparison)(a, out)
    E.close_all()


if __name__ == "__main__":
    main()
