"""Specification of the per-context check-node rule (ldpc_ctx_config cn_scale = alpha, cn_offset = beta) of the on-chip layered
min-sum kernel for any H, csrc/layered_csr.hip layered_csr_kernel<DCLASS, Ruled<LT>>: numpy, the three lam cell types.  The device
kernels reproduce it bit for bit (tests/test_layered_rule_gpu.py); at (3/4, 0) it IS the three shipped specifications
(tests/test_layered_rule_spec.py), which are pinned to the Double oracle.

The rule replaces ONE line of a row: the one that turns the row's two minima m1 <= m2 of |t_k| into its two message magnitudes.
Gathers, signs, arg-min, lam writes, the stopping rule and final_lam are those of the shipped specifications.

Float cells    (LDPC_F16, LDPC_F32), float32 arithmetic:
                 n = fl(fl(alpha) * m) - fl(beta)          two roundings, no fused multiply-add
                 if n < 0: n = 0                           a compare-select: a NaN stays a NaN
               At (3/4, 0) this is 0.75f * m: the product is >= +0 or not finite, subtracting +0 changes no float, the select never fires.
               LDPC_F16: every lam write saturated and rounded to binary16 (oracle/emulate_f16.py r16); LDPC_F32: lam as computed, and
               the non-finite veto (tests/layered_f32_spec.py): a frame that stops in a sweep with a lam that is not finite is failed.
Int8 cells     (LDPC_I8), integers only; the rule's two integers are fixed when the context is created:
                 a = clip(rint(float32(alpha) * 16), 1, 16)
                 b = rint(float32(beta) * float32(qscale))              rint: ties to even
                 n = min(max(((a m + 8) >> 4) - b, 0), 511)             a m / 16 rounded half up, less b, not below 0
               (12 m + 8) >> 4 == (3 m + 2) >> 2 for every m >= 0, so (a, b) = (12, 0) is tests/layered_i8_spec.py.
               The cap of 511.  A row record holds a magnitude in 9 bits, and the kernel's 32-bit sums rest on |msg| < 2^9.  At
               alpha = 3/4 that holds by induction: |lam| <= 127 and |msg| <= 383 give |t| = |lam - msg| <= 510, so
               n <= (3 * 510 + 2) >> 2 = 383 again.  At alpha = 1 the induction fails -- |msg| <= B gives only n <= 127 + B -- so the
               bound is imposed: with |msg| <= 511, |t| <= 638 and the cap restores 511.  At the default the cap never binds (383 < 511).
"""
import numpy as np

from oracle import emulate_f16 as em
from tests.layered_i8_spec import QMAX, quantize   # noqa: F401  (the quantiser is the shipped one)

MAG_CAP = 511


# ---------------------------------------------------------------------------------------------------------------- the rule
def float_rule(m, alpha=0.75, beta=0.0):
    """m float32 >= 0 (or not finite) -> the message magnitude, float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        p = (np.float32(alpha) * np.asarray(m, np.float32)).astype(np.float32)      # first rounding
        n = (p - np.float32(beta)).astype(np.float32)                               # second rounding
        return np.where(n < 0, np.float32(0), n).astype(np.float32)                 # (NaN < 0 is false: a NaN stays)


def int_params(alpha=0.75, beta=0.0, qscale=4.0):
    """-> (a, b), the integers an LDPC_I8 context computes with; the values it reports are a / 16 and b / qscale"""
    a = int(np.clip(np.rint(np.float32(alpha) * np.float32(16)), 1, 16))
    b = int(np.rint(np.float32(beta) * np.float32(qscale)))
    return a, b


def int_rule(m, a=12, b=0):
    m = np.asarray(m, np.int64)
    return np.minimum(np.maximum(((a * m + 8) >> 4) - b, 0), MAG_CAP)


# ---------------------------------------------------------------------------------------------------------------- graphs
def _csr(g):
    rp = np.asarray(g.row_ptr if hasattr(g, "row_ptr") else g.rp, np.int64)
    ci = np.asarray(g.col_idx if hasattr(g, "col_idx") else g.ci, np.int64)
    return rp, ci


def _rows(g):
    """the rows in ascending order, as groups of consecutive rows of one weight that share no column: (cols [R, d], first edge).  The
    rows of a group touch distinct lam cells and distinct messages, so updating them together IS updating them one after the other
    (what the kernel's barrier steps rest on as well); it only spares numpy calls.  A row without edges is skipped: its parity is even,
    it has no message and it writes no lam"""
    rp, ci = _csr(g)
    groups, cur, e0, seen = [], [], 0, set()
    for m in range(len(rp) - 1):
        cols = ci[rp[m]:rp[m + 1]]
        if not len(cols):
            continue
        if cur and (len(cols) != len(cur[0]) or not seen.isdisjoint(cols.tolist())):
            groups.append((np.stack(cur), e0))
            cur, seen = [], set()
        if not cur:
            e0 = int(rp[m])
        cur.append(cols)
        seen.update(cols.tolist())
    if cur:
        groups.append((np.stack(cur), e0))
    return groups, int(rp[-1])


def _apply(row_update, lam, msg, cols, e0, *rule):
    """one group of rows on the live frames, in place -> moved [F]"""
    F, (R, d) = lam.shape[0], cols.shape
    nl, nm, odd, flip = row_update(lam[:, cols].reshape(F * R, d), msg[:, e0:e0 + R * d].reshape(F * R, d), *rule)
    lam[:, cols] = nl.reshape(F, R, d)
    msg[:, e0:e0 + R * d] = nm.reshape(F, R * d)
    return (odd | flip).reshape(F, R).any(axis=1)


# ---------------------------------------------------------------------------------------------------------------- int8 cells
def row_update_i8(lam_c, msg, a=12, b=0):
    """tests/layered_i8_spec.py row_update with the rule (a, b): lam_c, msg int [F, d] -> (lam', msg', odd [F], flip [F])"""
    lam_c, msg = np.asarray(lam_c, np.int32), np.asarray(msg, np.int32)
    d = lam_c.shape[1]
    t = lam_c - msg
    s = t < 0
    mag_t = np.abs(t)
    two = np.sort(mag_t, axis=1)[:, :2]
    m1, m2 = two[:, 0], two[:, 1]
    n1, n2 = int_rule(m1, a, b).astype(np.int32), int_rule(m2, a, b).astype(np.int32)
    mag = np.where(mag_t == m1[:, None], n2[:, None], n1[:, None])
    neg = bool(d & 1) ^ np.logical_xor.reduce(s, axis=1)[:, None] ^ s
    new_msg = np.where(neg, -mag, mag)
    new_lam = np.clip(t + new_msg, -QMAX, QMAX)
    odd = np.logical_xor.reduce(lam_c > 0, axis=1)
    flip = ((new_lam > 0) != (lam_c > 0)).any(axis=1)
    return new_lam, new_msg, odd, flip


def decode_i8(graph, q, max_iters, qscale=4.0, alpha=0.75, beta=0.0, peak=None):
    """q int [F][N] in -127..127 -> bits [F, N] u8, sweeps [F] i32, converged [F] bool, final_lam [F, N] float64.
    peak: a one-element list that receives the largest message magnitude of the decode"""
    a, b = int_params(alpha, beta, qscale)
    q = np.asarray(q).astype(np.int32)
    assert q.ndim == 2 and np.abs(q).max(initial=0) <= QMAX
    F = q.shape[0]
    rows, E = _rows(graph)
    ok = np.ones(F, bool)
    for cols, _ in rows:
        ok &= ~np.logical_xor.reduce(q[:, cols] > 0, axis=2).any(axis=1)
    out = q.copy()
    conv = ok.copy()
    iters = np.zeros(F, np.int32)
    live = np.flatnonzero(~ok)
    lam = q[live].copy()
    msg = np.zeros((len(live), E), np.int32)
    top = 0
    for n in range(1, max_iters + 1):
        if not len(live):
            break
        moved = np.zeros(len(live), bool)
        for cols, e0 in rows:
            moved |= _apply(row_update_i8, lam, msg, cols, e0, a, b)
        top = max(top, int(np.abs(msg).max(initial=0)))
        fin = ~moved
        out[live[fin]] = lam[fin]; conv[live[fin]] = True; iters[live[fin]] = n
        live, lam, msg = live[moved], lam[moved], msg[moved]
    iters[live] = max_iters
    if peak is not None:
        peak[:] = [top]
    return (out > 0).astype(np.uint8), iters, conv, out.astype(np.float64) / np.float64(np.float32(qscale))


# ---------------------------------------------------------------------------------------------------------------- float cells
def f32_cast(x):
    return np.asarray(x, np.float32)


def row_update_float(l, msg, alpha=0.75, beta=0.0, store=em.r16):
    """l, msg float32 [F, d] -> (lam' as stored, msg', odd [F], flip [F]): oracle/emulate_f16.py cn_minsum_f32 with the rule in
    place of its 3/4"""
    with np.errstate(over="ignore", invalid="ignore"):
        t = (l - msg).astype(np.float32)
        mag_t = np.abs(t)
        pos = t > 0
        par = np.logical_xor.reduce(pos, axis=1, keepdims=True)
        i1 = np.argmin(mag_t, axis=1)
        m1 = np.take_along_axis(mag_t, i1[:, None], axis=1)
        a2 = mag_t.copy()
        np.put_along_axis(a2, i1[:, None], np.float32(np.inf), axis=1)
        m2 = a2.min(axis=1, keepdims=True)
        n1, n2 = float_rule(m1, alpha, beta), float_rule(m2, alpha, beta)
        k = np.arange(t.shape[1])[None, :]
        mag = np.where(k == i1[:, None], n2, n1)
        nm = np.where(np.logical_xor(par, pos), mag, -mag).astype(np.float32)
        nw = store((t + nm).astype(np.float32))
    odd = np.logical_xor.reduce(l > 0, axis=1)
    flip = ((nw > 0) != (l > 0)).any(axis=1)
    return nw, nm, odd, flip


def decode_float(graph, llr, max_iters, alpha=0.75, beta=0.0, cell="f16"):
    """llr [F, N] -> bits [F, N] u8, sweeps [F] i32, converged [F] bool, final_lam [F, N] float32.  cell "f16": every lam write through
    emulate_f16.r16; "f32": lam as computed, with the non-finite veto"""
    store = {"f16": em.r16, "f32": f32_cast}[cell]
    llr = np.asarray(llr, np.float32)
    F = llr.shape[0]
    rows, E = _rows(graph)
    orig = store(llr)
    ok = np.ones(F, bool)
    for cols, _ in rows:
        ok &= ~np.logical_xor.reduce(orig[:, cols] > 0, axis=2).any(axis=1)
    out = orig.copy()
    conv = ok.copy()
    iters = np.zeros(F, np.int32)
    live = np.flatnonzero(~ok)
    lam = orig[live].copy()
    msg = np.zeros((len(live), E), np.float32)
    for n in range(1, max_iters + 1):
        if not len(live):
            break
        moved = np.zeros(len(live), bool)
        for cols, e0 in rows:
            moved |= _apply(row_update_float, lam, msg, cols, e0, alpha, beta, store)
        fin = ~moved
        if cell == "f32":       # the veto: stopped by the rule with a lam that left the float range -> failed (the channel's LLRs)
            fin_ok = fin & np.isfinite(lam).all(axis=1)
        else:
            fin_ok = fin
        out[live[fin_ok]] = lam[fin_ok]; conv[live[fin_ok]] = True; iters[live[fin_ok]] = n
        vetoed = live[fin & ~fin_ok]
        iters[vetoed] = max_iters
        live, lam, msg = live[moved], lam[moved], msg[moved]
    iters[live] = max_iters
    return (out > 0).astype(np.uint8), iters, conv, out


def decode(cell, graph, llr, max_iters, alpha=0.75, beta=0.0, qscale=4.0):
    """one entry for the three cell types: llr float [F, N] (int8 cells quantise it with `qscale`)"""
    if cell == "i8":
        return decode_i8(graph, quantize(llr, qscale), max_iters, qscale, alpha, beta)
    return decode_float(graph, llr, max_iters, alpha, beta, cell)
