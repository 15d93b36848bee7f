"""Specification of the decoder's soft output (ldpc_decode_batch_dev_soft; csrc/layered_csr.hip layered_csr_kernel<DCLASS, Soft<cell>>):
numpy, the three lam cell types, the 3/4 or a per-context check-node rule.  The device kernels reproduce it bit for bit
(tests/test_soft_output_gpu.py).

The sweeps are those of tests/layered_rule_spec.py -- its _rows, _apply, row_update_float and row_update_i8 are used as they are -- in a
loop of its own that KEEPS the lam of every frame.  bits, sweeps and flags are that specification's on every frame
(tests/test_soft_output_spec.py).  What is new:

P, the posterior   lam as it stands when the frame stops, for EVERY frame:
                     converged in sweep n                         lam after sweep n (= final_lam of the decode entry points)
                     out of sweeps                                lam after sweep max_iters (final_lam gives the channel LLRs there)
                     converged before the first sweep, or
                     max_iters = 0                                the channel LLRs as the cell took them in
                     an f32 frame failed by the non-finite veto   lam as it stands: it may hold an infinity or a NaN
C, the channel LLR as the cell took it in:  fp16 cells r16(llr) (a NaN as +0, saturated, rounded); f32 cells the float; int8 cells the
                   quantised integer q = clip(rint(llr * qscale), -127, 127).
E, the extrinsic   P - C: ONE float32 subtraction for float cells, an integer subtraction (in -254 .. 254) for int8 cells.

Output formats ("f32", "f16", "i8"; soft_qscale is read for "i8" alone, 0 = 4.0 as in the demappers):
  float cells   f32  the value as it is
                f16  clamped to +-65504 by compares (a NaN passes), rounded to nearest even: for the posterior of an fp16 cell the cell's bits
                i8   clip(rint(fl(v * soft_qscale)), -127, 127), a NaN as 0                       (tests/layered_i8_spec.quantize)
  int8 cells    f32  fl(float32(v) / float32(llr_qscale)): one division
                f16  that float through the f16 rule above
                i8   clip(v, -127, 127)

What is NOT specified: a NaN that a sweep takes in.  numpy's argmin and the device's min treat a NaN among a row's magnitudes differently,
and the payload of a NaN that arithmetic CREATES (inf - inf) is the machine's.  The tests therefore put a NaN only into a frame that stops
before its first sweep (P = C = the NaN as given), an infinity only where no inf - inf arises in P, and compare an extrinsic row of a
frame that is not finite with NaN == NaN."""
import numpy as np

from oracle import emulate_f16 as em
from tests import layered_rule_spec as rule
from tests.layered_i8_spec import QMAX, quantize

F16_MAX = np.float32(65504.0)
FORMATS = ("f32", "f16", "i8")
KINDS = ("posterior", "extrinsic")


def channel(cell, llr, qscale=4.0):
    """C: the channel LLRs as the cell takes them in -- float32 [F, N] (float cells) or int32 [F, N] (int8 cells)"""
    if cell == "i8":
        return quantize(llr, qscale)
    llr = np.asarray(llr, np.float32)
    return em.r16(llr) if cell == "f16" else llr.copy()


def _syndrome_ok(rows, c):
    ok = np.ones(c.shape[0], bool)
    for cols, _ in rows:
        ok &= ~np.logical_xor.reduce(c[:, cols] > 0, axis=2).any(axis=1)
    return ok


def decode(cell, graph, llr, max_iters, alpha=0.75, beta=0.0, qscale=4.0):
    """llr float [F, N] -> bits [F, N] u8, sweeps [F] i32, converged [F] bool, P [F, N], C [F, N] (float32, or int32 for int8 cells)"""
    rows, E = rule._rows(graph)
    C = channel(cell, llr, qscale)
    F = C.shape[0]
    if cell == "i8":
        update, args, zero = rule.row_update_i8, rule.int_params(alpha, beta, qscale), np.int32
    else:
        update, args, zero = rule.row_update_float, (alpha, beta, {"f16": em.r16, "f32": rule.f32_cast}[cell]), np.float32
    ok = _syndrome_ok(rows, C)
    P = C.copy()
    conv = ok.copy()
    iters = np.zeros(F, np.int32)
    if cell == "f32":       # the veto holds for a frame that is a codeword before the first sweep as well
        conv &= np.isfinite(C).all(axis=1)
        iters[ok & ~conv] = max_iters
    live = np.flatnonzero(~ok)
    lam = C[live].copy()
    msg = np.zeros((len(live), E), zero)
    for n in range(1, max_iters + 1):
        if not len(live):
            break
        moved = np.zeros(len(live), bool)
        for cols, e0 in rows:
            moved |= rule._apply(update, lam, msg, cols, e0, *args)
        P[live] = lam                                   # lam as it stands: every frame, every sweep it ran
        fin = ~moved
        fin_ok = fin & np.isfinite(lam).all(axis=1) if cell == "f32" else fin
        conv[live[fin_ok]] = True
        iters[live[fin_ok]] = n
        iters[live[fin & ~fin_ok]] = max_iters          # vetoed: failed, P stays the lam it stopped with
        live, lam, msg = live[moved], lam[moved], msg[moved]
    iters[live] = max_iters
    bits = (np.where(conv[:, None], P, C) > 0).astype(np.uint8)
    return bits, iters, conv, P, C


def value(cell, P, C, kind):
    """the soft value before its output format: P, or E = P - C"""
    if kind == "posterior":
        return P
    if cell == "i8":
        return P - C
    with np.errstate(invalid="ignore", over="ignore"):
        return (P - C).astype(np.float32)


def _to_f16(v):
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.where(v < -F16_MAX, -F16_MAX, np.where(v > F16_MAX, F16_MAX, v)).astype(np.float32)    # a NaN fails both compares
        return c.astype(np.float16)


def output(cell, v, fmt, soft_qscale=0.0, qscale=4.0):
    """v: value() of a float cell (float32) or of an int8 cell (int32) -> the array ldpc_decode_batch_dev_soft writes:
    float32, float16 or int8"""
    if cell == "i8":
        if fmt == "i8":
            return np.clip(v, -QMAX, QMAX).astype(np.int8)
        f = (v.astype(np.float32) / np.float32(qscale)).astype(np.float32)
        return f if fmt == "f32" else _to_f16(f)
    if fmt == "f32":
        return np.asarray(v, np.float32)
    if fmt == "f16":
        return _to_f16(np.asarray(v, np.float32))
    return quantize(np.asarray(v, np.float32), soft_qscale if soft_qscale else 4.0).astype(np.int8)


def soft(cell, P, C, kind, fmt, soft_qscale=0.0, qscale=4.0):
    return output(cell, value(cell, P, C, kind), fmt, soft_qscale, qscale)
