"""Specification of the A-min* check-node rule (ldpc_ctx_config cn_rule = LDPC_CN_AMINSTAR; Jones, Valles, Smith, Villasenor 2003) of the
on-chip layered kernel for any H, csrc/layered_csr.hip layered_csr_kernel / _soft_kernel / _cont_kernel<DCLASS, MinStar<LT>>: numpy, float
cells (LDPC_F16, LDPC_F32).  The device kernels reproduce it bit for bit (tests/test_layered_aminstar_gpu.py).

The rule replaces the part of a row that turns |t_k| into message magnitudes.  Float32, one rounding per operation, no fused multiply-add:

    c(x)    = n = 0.625 - fl(0.25 * x);  n < 0 ? 0 : n                                      a compare-select: a NaN stays a NaN
    a [+] b = s = fl(min(a, b) + c(fl(a + b)));  n = fl(s - c(|fl(a - b)|));  n < 0 ? 0 : n

c is the two-segment fit of log(1 + exp(-x)); it is non-increasing and a + b >= |a - b|, so 0 <= a [+] b <= min(a, b), and once
|a - b| >= 2.5 both corrections are 0 and a [+] b IS min(a, b).  For a row with t_k = lam[c_k] - old msg_k, edges in CSR order:

    i*     the FIRST k with the least |t_k|;  m1 = |t_i*|
    Delta  the left fold of [+] over |t_k|, k != i*, in ascending k, starting from the first such edge
    n1     Delta [+] m1
    |msg'| Delta on edge i*, n1 on every other edge (an edge that ties with m1 included)
    a row of weight 2 is exact: edge i* gets the other edge's |t|, the other edge gets m1 -- no [+]

Everything else is the shipped specifications': the signs, the parity / flip / stop rule and the lam writes of tests/layered_rule_spec.py
row_update_float (fp16 cells through oracle/emulate_f16.py r16; f32 cells as computed); the channel, the veto, P and the output formats of
tests/soft_output_spec.py; the state and its start of tests/decode_continue_spec.py.  Their decode loops hold their row update by name, so
the loop is restated ONCE here with the row update as an argument (_sweeps); tests/test_layered_aminstar_spec.py holds it, given
row_update_float, to soft_output_spec.decode and decode_continue_spec.call bit for bit.

What is NOT specified is what soft_output_spec leaves open: a NaN that a sweep takes in (numpy's minimum and argmin and the device's
treat it differently)."""
import numpy as np

from oracle import emulate_f16 as em
from tests import decode_continue_spec as cont
from tests import layered_rule_spec as rule
from tests import soft_output_spec as soft

State = cont.State
_STORE = {"f16": em.r16, "f32": rule.f32_cast}


# ---------------------------------------------------------------------------------------------------------------- the rule
def corr(x):
    """c(x), float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        p = (np.float32(0.25) * np.asarray(x, np.float32)).astype(np.float32)
        n = (np.float32(0.625) - p).astype(np.float32)
        return np.where(n < 0, np.float32(0), n).astype(np.float32)


def boxplus(a, b):
    """a [+] b for magnitudes a, b >= 0, float32"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = (np.minimum(a, b) + corr((a + b).astype(np.float32))).astype(np.float32)
        n = (s - corr(np.abs((a - b).astype(np.float32)))).astype(np.float32)
        return np.where(n < 0, np.float32(0), n).astype(np.float32)


def magnitudes(mag_t):
    """|t| float32 [F, d], d >= 2 -> (i* [F], n1 [F, 1], Delta [F, 1])"""
    F, d = mag_t.shape
    i1 = np.argmin(mag_t, axis=1)                                   # the first index of the minimum
    m1 = np.take_along_axis(mag_t, i1[:, None], axis=1)
    others = mag_t[np.arange(d)[None, :] != i1[:, None]].reshape(F, d - 1)      # ascending k
    delta = others[:, 0]
    for j in range(1, d - 1):
        delta = boxplus(delta, others[:, j])
    delta = delta[:, None]
    n1 = m1 if d == 2 else boxplus(delta, m1)
    return i1, n1.astype(np.float32), delta.astype(np.float32)


def row_update_aminstar(l, msg, store=em.r16):
    """l, msg float32 [F, d] -> (lam' as stored, msg', odd [F], flip [F]): tests/layered_rule_spec.py row_update_float with the A-min*
    magnitudes in place of the two scaled minima"""
    with np.errstate(over="ignore", invalid="ignore"):
        t = (l - msg).astype(np.float32)
        pos = t > 0
        par = np.logical_xor.reduce(pos, axis=1, keepdims=True)
        i1, n1, delta = magnitudes(np.abs(t))
        k = np.arange(t.shape[1])[None, :]
        mag = np.where(k == i1[:, None], delta, n1)
        nm = np.where(np.logical_xor(par, pos), mag, -mag).astype(np.float32)
        nw = store((t + nm).astype(np.float32))
    odd = np.logical_xor.reduce(l > 0, axis=1)
    flip = ((nw > 0) != (l > 0)).any(axis=1)
    return nw, nm, odd, flip


# ---------------------------------------------------------------------------------------------------------------- the loop
def _sweeps(cell, graph, C, lam0, msg0, max_iters, update=row_update_aminstar, args=None):
    """The loop of soft_output_spec.decode and decode_continue_spec.call with the row update as an argument.  C: the channel as the cell took
    it in; lam0: the starting lam (C itself in a plain decode); msg0 [F, E]: the stored messages (zeros in a plain decode).
    -> bits, sweeps, converged, P, msg as the last sweep left it (msg0 for a frame that ran no sweep)"""
    rows, E = rule._rows(graph)
    args = (_STORE[cell],) if args is None else args
    F = C.shape[0]
    ok = soft._syndrome_ok(rows, lam0)
    P = lam0.copy()
    conv = ok.copy()
    iters = np.zeros(F, np.int32)
    if cell == "f32":                                   # the veto holds for a frame that stops before its first sweep as well
        conv &= np.isfinite(lam0).all(axis=1)
        iters[ok & ~conv] = max_iters
    live = np.flatnonzero(~ok)
    lam = lam0[live].copy()
    msg = msg0[live].copy()
    out_msg = msg0.copy()
    for n in range(1, max_iters + 1):
        if not len(live):
            break
        moved = np.zeros(len(live), bool)
        for cols, e0 in rows:
            moved |= rule._apply(update, lam, msg, cols, e0, *args)
        P[live] = lam
        out_msg[live] = msg
        fin = ~moved
        fin_ok = fin & np.isfinite(lam).all(axis=1) if cell == "f32" else fin
        conv[live[fin_ok]] = True
        iters[live[fin_ok]] = n
        iters[live[fin & ~fin_ok]] = max_iters
        live, lam, msg = live[moved], lam[moved], msg[moved]
    iters[live] = max_iters
    bits = (np.where(conv[:, None], P, C) > 0).astype(np.uint8)
    return bits, iters, conv, P, out_msg


def _zero_msg(graph, F):
    return np.zeros((F, rule._rows(graph)[1]), np.float32)


# ---------------------------------------------------------------------------------------------------------------- entry points
def decode_soft(cell, graph, llr, max_iters, **kw):
    """soft_output_spec.decode with this row rule: llr float [F, N] -> bits, sweeps, converged, P, C"""
    C = soft.channel(cell, llr)
    bits, iters, conv, P, _ = _sweeps(cell, graph, C, C, _zero_msg(graph, len(C)), max_iters, **kw)
    return bits, iters, conv, P, C


def decode_float(graph, llr, max_iters, cell="f16"):
    """layered_rule_spec.decode_float with this row rule: -> bits [F, N] u8, sweeps [F] i32, converged [F] bool, final_lam [F, N] float32
    (lam of a frame that converged, the channel LLRs as the cell took them in otherwise)"""
    bits, iters, conv, P, C = decode_soft(cell, graph, llr, max_iters)
    return bits, iters, conv, np.where(conv[:, None], P, C).astype(np.float32)


def decode_f16(graph, llr, max_iters):
    return decode_float(graph, llr, max_iters, "f16")


def decode_f32(graph, llr, max_iters):
    return decode_float(graph, llr, max_iters, "f32")


def call(cell, graph, state, llr, max_iters, first=0, **kw):
    """decode_continue_spec.call with this row rule: llr [F, N] on slots first .. first + F - 1 of `state` (decode_continue_spec.State, not
    written) -> (bits, sweeps, converged, P, C'), the new state"""
    C = soft.channel(cell, llr)
    F = C.shape[0]
    assert 0 <= first and first + F <= len(state.S) and state.cell == cell
    sl = slice(first, first + F)
    lam0 = cont.start(cell, C, state.S[sl])
    bits, iters, conv, P, msg = _sweeps(cell, graph, C, lam0, state.msg[sl], max_iters, **kw)
    new = state.copy()
    new.msg[sl] = msg
    new.S[sl] = soft.value(cell, P, C, "extrinsic")
    return (bits, iters, conv, P, C), new
