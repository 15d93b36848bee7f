"""Specification of the int8 fixed-point layered min-sum decoder (LDPC_I8, csrc/layered_csr.hip layered_csr_kernel<DCLASS, int8_t>):
numpy, integers only.  The device kernel reproduces it bit for bit (tests/test_layered_i8_gpu.py).

Quantiser      q = clip(rint(float32(llr) * float32(qscale)), -127, 127): ONE float32 multiply, rint = round half to even;
               +inf -> 127, -inf -> -127, NaN -> 0; a double is converted to float32 first; native int8: q = max(v, -127).
State          lam: an int8 cell in -127..127 per column, hard(lam) = lam > 0; one message per edge, 0 at the start.
One row        of weight d, edges k in column order, plain integer arithmetic:
                 t_k = lam[c_k] - msg_k (not clamped), s_k = t_k < 0 (zero counts as non-negative), a_k = |t_k|
                 m1, m2 = the smallest and the second smallest a_k (with multiplicity)
                 n1 = (3 m1 + 2) >> 2, n2 = (3 m2 + 2) >> 2                  (the 3/4 of Min.hs:78, rounded half up)
                 |msg'_k| = n2 if a_k == m1 else n1; msg'_k < 0 iff (d odd) ^ (xor_j s_j) ^ s_k
                 lam'[c_k] = clip(t_k + msg'_k, -127, 127)
                 odd  |= parity of hard(lam[c_k]) before the update; flip |= hard(lam') != hard(lam), after the clip
Rows           in ascending order; layers only group them (the rows of a layer share no column).
Stopping rule  oracle/ldpc_oracle.c oracle_decode_layered: before sweep 1 the syndrome of hard(q) -- zero: converged, iters = 0;
               after a sweep: converged when no row was odd and no decision flipped; out of sweeps: bits = hard(q), flag 0,
               iters = max_iters.
final_lam      double(lam) / double(qscale) for a converged frame, double(q) / double(qscale) otherwise (qscale a float32).
"""
import numpy as np

QMAX = 127


def quantize(llr, qscale=4.0):
    """-> int32 array in -127..127"""
    a = np.asarray(llr)
    if a.dtype == np.int8:
        return np.maximum(a.astype(np.int32), -QMAX)
    with np.errstate(invalid="ignore", over="ignore"):
        x = a.astype(np.float32) * np.float32(qscale)            # one float32 multiply
        r = np.rint(x)                                           # half to even
    r = np.where(np.isnan(r), np.float32(0), np.clip(r, -QMAX, QMAX))
    return r.astype(np.int32)


def row_update(lam_c, msg):
    """one check row on F frames: lam_c, msg int [F, d] -> (lam' [F, d], msg' [F, d], odd [F], flip [F])"""
    lam_c, msg = np.asarray(lam_c, np.int32), np.asarray(msg, np.int32)
    d = lam_c.shape[1]
    t = lam_c - msg
    s = t < 0
    a = np.abs(t)
    two = np.sort(a, axis=1)[:, :2]
    m1, m2 = two[:, 0], two[:, 1]
    n1, n2 = (3 * m1 + 2) >> 2, (3 * m2 + 2) >> 2
    mag = np.where(a == m1[:, None], n2[:, None], n1[:, None])
    neg = bool(d & 1) ^ np.logical_xor.reduce(s, axis=1)[:, None] ^ s
    new_msg = np.where(neg, -mag, mag)
    new_lam = np.clip(t + new_msg, -QMAX, QMAX)
    odd = np.logical_xor.reduce(lam_c > 0, axis=1)
    flip = ((new_lam > 0) != (lam_c > 0)).any(axis=1)
    return new_lam, new_msg, odd, flip


def _rows(g):
    rp, ci = np.asarray(g.row_ptr, np.int64), np.asarray(g.col_idx, np.int64)
    return [(ci[rp[m]:rp[m + 1]], int(rp[m])) for m in range(len(rp) - 1)]


def decode_minsum_i8_layered(graph, q, max_iters, qscale=4.0):
    """q int [F][N] in -127..127 -> bits [F, N] u8, sweeps [F] i32, converged [F] bool, final_lam [F, N] float64"""
    q = np.asarray(q).astype(np.int32)
    assert q.ndim == 2 and np.abs(q).max(initial=0) <= QMAX
    F = q.shape[0]
    rows = _rows(graph)
    E = int(np.asarray(graph.row_ptr)[-1])
    ok = np.ones(F, bool)
    for cols, _ in rows:
        ok &= ~np.logical_xor.reduce(q[:, cols] > 0, axis=1)
    out = q.copy()
    conv = ok.copy()
    iters = np.zeros(F, np.int32)
    live = np.flatnonzero(~ok)                                   # the frames still being decoded
    lam = q[live].copy()
    msg = np.zeros((len(live), E), np.int32)
    for n in range(1, max_iters + 1):
        if not len(live):
            break
        moved = np.zeros(len(live), bool)
        for cols, e0 in rows:
            d = len(cols)
            new_lam, new_msg, odd, flip = row_update(lam[:, cols], msg[:, e0:e0 + d])
            lam[:, cols] = new_lam
            msg[:, e0:e0 + d] = new_msg
            moved |= odd | flip
        fin = ~moved
        out[live[fin]] = lam[fin]; conv[live[fin]] = True; iters[live[fin]] = n
        live, lam, msg = live[moved], lam[moved], msg[moved]
    iters[live] = max_iters                                      # out of sweeps: the channel's decisions, as stored
    return (out > 0).astype(np.uint8), iters, conv, out.astype(np.float64) / np.float64(np.float32(qscale))
