"""Specification of the soft demapper with a-priori input (ldpc_demap_dev_il_apriori, csrc/demap_apriori.hip): numpy.

Conventions    those of tests/modulation_spec.py: LLR = log P(1) / P(0) > 0 <=> bit 1, label bit j counted MSB first, table objects.
               La [B][N] float32 is in CODEWORD order; transmitted bit t of a frame has La[pos[t]], the pad bits of a ragged last symbol 0.
Rule           all float32, one operation at a time, nothing fused.  d_p the squared distances of modulation_spec.symbol_llrs
               (demap_logmap_spec.table_distances), inv_s = float32(1 / (2 sigma^2)), times the symbol's gain where one is given
               (fading_spec.inv_rule).
                 a_p   = the sum of La_j over the set label bits j of p, MSB first, left to right: a_0 = +0, a_p = a_q + La_j with j the
                         least significant set bit of p and q = p without it; one set bit: a_p = La_j, no addition
                 u_p   = fl(a_p - fl(d_p inv_s))
                 U1_j, U0_j = the max of u_p over the labels whose bit j is 1, 0 (a NaN is skipped unless all are NaN: fmax)
                 max-log   LLR_j = fl(fl(U1_j - U0_j) - La_j)      the EXTRINSIC value: the bit's own knowledge is taken out
                 log-MAP   ml = fl(U1_j - U0_j); corr = fl(log s1 - log s0), s_v = the float32 sum, in label order, of exp(fl(u_p - U_v))
                           over the subset; LLR_j = fl((corr != 0 ? fl(ml + corr) : ml) - La_j)      (demap_logmap_spec's convention)
La = 0         a_p = 0 for every p, u_p = -fl(d_p inv_s) exactly, U_v = -fl(m_v inv_s) (rounding is monotone), so the value is
               new = fl(fl(m0 inv_s) - fl(m1 inv_s)) where the shipped demapper has old = fl(fl(m0 - m1) inv_s): not the same bits.  With
               u = 2^-24: new = (m0 s (1 + e1) - m1 s (1 + e2)) (1 + e3), old = (m0 - m1) (1 + e4) s (1 + e5), |e| <= u, so to first order
               |new - old| <= u (m0 + m1) s + u |m0 - m1| s + 2 u |m0 - m1| s <= 4 u (m0 + m1) s = 2^-22 (m0 + m1) inv_s.
               The bar is twice that, zero_apriori_bar() = 2^-21 (m0 + m1) inv_s.
max-log bar    against the same formula in float64 on the same float32 inputs (brute_force()).  With T = max_p d_p inv_s, A = sum_j |La_j|:
               d_p carries 4 u relative (the difference, the squares, their sum), fl(d_p inv_s) 5 u; a_p at most (m - 1) u A; the
               subtraction u |u_p| <= u (A + T): |err u_p| <= u (6 T + m A).  A max moves by no more than its arguments; U1 - U0 adds
               u |U1 - U0| <= 2 u (A + T), the last subtraction u (3 A + 2 T): maxlog_bar() = u (16 T + (2 m + 5) A).
log-MAP bar    against brute_force() as well.  The project's bar for the exact rule, demap_logmap_spec.bound = 2^-14 + 2 ulp32, covers the
               exponentials, sums and logarithms and the last additions (derived there) -- against a reference that TAKES the float32 max-log
               term.  Here the reference is float64 throughout, and on the inputs of tests/demap_apriori_cases.py the float32 restatement
               itself leaves 2^-14 + 2 ulp32(max |u_p|) (1.27 times, "bpsk" at "collapse", where there is no correction at all: it is
               the max-log roundings above that the project's bar does not hold).  So they are added, from the operations: the max-log
               term's maxlog_bar(); and each exponential's argument fl(u_p - U_v) carries the errors of u_p and of U_v, 2 u (6 T + m A)
               -- a log of a sum of exponentials moves by no more than the largest move of an argument -- so c1 - c0 carries
               4 u (6 T + m A):  logmap_bar() = bound(want) + maxlog_bar() + u (24 T + 4 m A).  At "low" (T about 20) that is 1e-4,
               where a wrong subset or a missing term shows at 1e-2 or more.
Outputs        f32 as it is; f16 / i8: modulation_spec's converters; 0 at the punctured positions."""
import numpy as np

from tests import demap_logmap_spec as ls
from tests import fading_spec as fs
from tests import interleaver_spec as ils
from tests import modulation_spec as ms

MAXLOG, LOGMAP = ls.MAXLOG, ls.LOGMAP
U = 2.0 ** -24


def inv_scale(shape, nv, a=None):
    """inv_s [...] float32"""
    if a is None:
        return np.full(shape, np.float32(1.0 / (2.0 * float(nv))), np.float32)
    out = fs.inv_rule(nv, a)
    assert out.shape == tuple(shape)
    return out


def apriori_sums(la):
    """la [..., m] float32 -> a [..., 2^m] float32"""
    la = np.asarray(la, np.float32)
    m = la.shape[-1]
    a = np.zeros(la.shape[:-1] + (1 << m,), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(1, 1 << m):
            low = p & -p
            j, q = m - low.bit_length(), p ^ low              # label bit j (MSB first) is bit m - 1 - j of p
            a[..., p] = la[..., j] if q == 0 else a[..., q] + la[..., j]
    return a


def metrics(points, sym, inv_s, la):
    """-> u [..., 2^m] float32"""
    d = ls.table_distances(points, sym)
    with np.errstate(invalid="ignore", over="ignore"):
        t = d * np.asarray(inv_s, np.float32)[..., None]
        u = apriori_sums(la) - t
    assert t.dtype == np.float32 and u.dtype == np.float32
    return u


def symbol_llrs(points, sym, inv_s, la, rule=MAXLOG):
    """sym [..., 2], inv_s [...], la [..., m] float32 -> LLRs [..., m] float32"""
    la = np.asarray(la, np.float32)
    m = ms.bits_per_symbol(points)
    assert la.shape[-1] == m
    u = metrics(points, sym, inv_s, la)
    out = np.empty(la.shape, np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for j, one in enumerate(ls._masks(m)):
            U0, U1 = np.fmax.reduce(u[..., ~one], axis=-1), np.fmax.reduce(u[..., one], axis=-1)
            v = U1 - U0
            if rule == LOGMAP and m > 1:
                c = []
                for top, sel in ((U0, ~one), (U1, one)):
                    e = np.exp(u[..., sel] - top[..., None])
                    acc = e[..., 0]
                    for p in range(1, e.shape[-1]):
                        acc = acc + e[..., p]
                    assert acc.dtype == np.float32
                    c.append(np.log(acc))
                corr = c[1] - c[0]
                v = np.where(corr != 0, v + corr, v)
            out[..., j] = v - la[..., j]
    assert out.dtype == np.float32
    return out


def brute_force(points, sym, inv_s, la, rule=MAXLOG):
    """the same formula in float64 on the same float32 inputs -> (LLRs [..., m], T = max_p d_p inv_s [...], A = sum |La_j| [...],
    the largest |u_p| [...])"""
    pts = np.asarray(points, np.float32).astype(np.float64)
    m = ms.bits_per_symbol(points)
    sym, s, la = np.asarray(sym, np.float32).astype(np.float64), np.asarray(inv_s, np.float32).astype(np.float64), np.asarray(la, np.float32).astype(np.float64)
    lab = np.arange(1 << m)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = ((sym[..., None, 0] - pts[:, 0]) ** 2 + (sym[..., None, 1] - pts[:, 1]) ** 2) * s[..., None]
        a = np.zeros(t.shape)
        for j in range(m):
            a += np.where((lab >> (m - 1 - j)) & 1, la[..., j:j + 1], 0.0)
        x = a - t
        out = np.empty(la.shape)
        for j, one in enumerate(ls._masks(m)):
            l = []
            for sel in (~one, one):
                top = x[..., sel].max(axis=-1)
                l.append(top if rule == MAXLOG else top + np.log(np.exp(x[..., sel] - top[..., None]).sum(axis=-1)))
            out[..., j] = (l[1] - l[0]) - la[..., j]
    return out, t.max(axis=-1), np.abs(la).sum(axis=-1), np.abs(x).max(axis=-1)


def zero_apriori_bar(points, sym, inv_s):
    """2^-21 (m0_j + m1_j) inv_s [..., m] (float64)"""
    d = ls.table_distances(points, sym)
    m0, m1 = ls._mins(d, ms.bits_per_symbol(points))
    with np.errstate(invalid="ignore", over="ignore"):
        return 2.0 ** -21 * (m0.astype(np.float64) + m1.astype(np.float64)) * np.asarray(inv_s, np.float64)[..., None]


def maxlog_bar(m, T, A):
    """u (16 T + (2 m + 5) A), per symbol [...]"""
    return U * (16.0 * T + (2 * m + 5) * A)


def logmap_bar(want, m, T, A):
    """demap_logmap_spec.bound(want) + maxlog_bar + u (24 T + 4 m A), per element [..., m]"""
    T, A = np.asarray(T)[..., None], np.asarray(A)[..., None]
    return ls.bound(want) + maxlog_bar(m, T, A) + U * (24.0 * T + 4.0 * m * A)


def gather(la_cw, pos, m):
    """La [B][N] in codeword order -> [B][n_sym][m] in transmitted order, 0 for the pad bits"""
    la_cw = np.asarray(la_cw, np.float32)
    pos = ils.check(pos, la_cw.shape[1])
    B, n_tx = la_cw.shape[0], len(pos)
    ns = ms.symbols_per_frame(n_tx, m)
    out = np.zeros((B, ns * m), np.float32)
    out[:, :n_tx] = la_cw[:, pos]
    return out.reshape(B, ns, m)


def per_symbol(points, sym, a, pos, nv, la_cw, rule=MAXLOG):
    """-> (LLRs [B][n_sym][m] float32, inv_s [B][n_sym], La [B][n_sym][m])"""
    sym = np.asarray(sym, np.float32)
    la = gather(la_cw, pos, ms.bits_per_symbol(points))
    inv_s = inv_scale(sym.shape[:-1], nv, a)
    return symbol_llrs(points, sym, inv_s, la, rule), inv_s, la


def place(per, pos, N, fmt=ms.LLR_F32, qscale=4.0):
    """per [B][n_sym][m] float -> rows [B][N] in the output format, 0 at the punctured positions"""
    B, n_tx = per.shape[0], len(pos)
    tx = np.ascontiguousarray(per.reshape(B, -1)[:, :n_tx])
    return ils.deinterleave(fs._format(tx.astype(np.float32), fmt, qscale) if per.dtype == np.float32 else tx, pos, N)


def demap_il_apriori(points, sym, a, pos, N, nv, la_cw, rule=MAXLOG, fmt=ms.LLR_F32, qscale=4.0):
    """sym [B][ceil(n_tx / m)][2] float32, a [B][ceil(n_tx / m)] float32 or None, la_cw [B][N] float32 -> [B][N] float32 / float16 / int8"""
    return place(per_symbol(points, sym, a, pos, nv, la_cw, rule)[0], pos, N, fmt, qscale)
