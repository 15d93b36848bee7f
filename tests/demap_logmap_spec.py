"""Specification of the exact (log-MAP) LLR rule of the soft demappers (include/ldpc_hip.h THE LLR RULE, ldpc_modulation_with_rule;
csrc/demap.h demap_llrs_logmap, csrc/demap_product.h axis_llrs_logmap, csrc/demap_rm.hip): numpy.

Conventions    those of tests/modulation_spec.py: LLR > 0 <=> bit 1, label bit j counted MSB first.
Distances      the float32 d_p of modulation_spec.symbol_llrs (a table object: fl(fl(dx dx) + fl(dy dy))) or the e_l of
               product_modulation_spec.axis_mins (a product object, per axis: fl(dx dx)), m0_j / m1_j their minima over the labels whose
               bit j is 0 / 1, inv_s = float32(1 / (2 sigma^2)), times the symbol's gain where one is given (fading_spec.inv_rule).
Max-log term   ml_j = fl(fl(m0_j - m1_j) inv_s): TAKEN from those specifications by import (modulation_spec.symbol_llrs,
               product_modulation_spec.symbol_llrs, fading_spec.symbol_llrs / symbol_llrs_product).  The distances are written out once
               more here, and every call asserts that they give that imported term bit for bit, so the two cannot drift.
Rule           LLR_j = ml_j + (c1_j - c0_j),  c_v = log(sum over the labels p whose bit j is v of exp(-(d_p - m_v) inv_s)).
               c1 - c0 is computed in FLOAT64 from the float32 d_p, m_v and inv_s and added to the float32 ml_j: llrs() returns float64.
               Where c1 - c0 is zero the result is ml_j as it is, the sign of a zero included (-0 + 0 would be +0):
                 one label a subset (m = 1, or b = 1 per axis); every other (d_p - m_v) inv_s above 104 (collapsed(), below): the
                 kernels give ml_j bit for bit; inv_s = 0: both sums are the same integer.
               A NaN d_p or inv_s makes the LLR NaN: exactly the elements that are NaN under max-log.
Product        the rule per axis, on that axis's 2^b levels and b bits: exact, because the other axis's factor
               sum_q exp(-e_q inv_s) is common to both subsets and cancels (tests/test_demap_logmap_spec.py proves it against the sum over
               all 4^b points).
float32 form   llrs32(): the device's operation order in numpy float32 -- t = fl(fl(m_v - d_p) inv_s), exp, the sums in label order,
               log, fl(c1 - c0), fl(ml + that) -- with numpy's exp and log where the device has its base-2 instructions.
GPU bar        |device - llrs()| <= 2^-14 + 2 ulp32(result) per element (BAR, bound()): each exp term carries the rounding of its scaled
               argument and one hardware ulp, about 2^-22 absolute; a sum of 32 terms adds at most 31 * 2^-24 relative; the log about
               5 * 2^-22; doubled for c1 - c0: about 2e-5, and the bar is three times that.  A wrong subset, a missing term or a misplaced
               shift shows at 1e-2 or more at low SNR.
Outputs        f32 as it is; to_f16 / to_i8: modulation_spec's converters."""
import numpy as np

from tests import fading_spec as fs
from tests import layered_i8_spec
from tests import modulation_spec as ms
from tests import product_modulation_spec as ps

MAXLOG, LOGMAP = 0, 1
BAR = 2.0 ** -14
COLLAPSE = 104.0      # exp(-104) is below half the smallest float32 denormal


def _masks(m):
    lab = np.arange(1 << m)
    return [((lab >> (m - 1 - j)) & 1).astype(bool) for j in range(m)]


def _same_bits(a, b):
    an, bn = np.isnan(a), np.isnan(b)
    return a.dtype == b.dtype == np.float32 and np.array_equal(an, bn) and np.array_equal(np.where(an, 0, a.view(np.uint32)), np.where(bn, 0, b.view(np.uint32)))


def table_distances(points, sym):
    """sym [..., 2] float32 -> d [..., 2^m] float32, modulation_spec.symbol_llrs's"""
    pts, sym = np.asarray(points, np.float32), np.asarray(sym, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = sym[..., None, 0] - pts[:, 0]
        dy = sym[..., None, 1] - pts[:, 1]
        d = dx * dx + dy * dy
    assert d.dtype == np.float32
    return d


def axis_distances(levels, y):
    """y [...] float32 -> e [..., 2^b] float32, product_modulation_spec.axis_mins's"""
    lev, y = np.asarray(levels, np.float32), np.asarray(y, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = y[..., None] - lev
        e = dx * dx
    assert e.dtype == np.float32
    return e


def _mins(d, m):
    """-> (m0, m1) [..., m] float32"""
    m0, m1 = np.empty(d.shape[:-1] + (m,), np.float32), np.empty(d.shape[:-1] + (m,), np.float32)
    with np.errstate(invalid="ignore"):
        for j, one in enumerate(_masks(m)):
            m0[..., j], m1[..., j] = np.minimum.reduce(d[..., ~one], axis=-1), np.minimum.reduce(d[..., one], axis=-1)
    return m0, m1


def _checked_maxlog(d, inv_s, ml):
    """the imported max-log term ml, after the assertion that the distances written out here give it bit for bit"""
    m = ml.shape[-1]
    m0, m1 = _mins(d, m)
    with np.errstate(invalid="ignore", over="ignore"):
        own = (m0 - m1) * inv_s[..., None]
    assert own.dtype == np.float32 and _same_bits(own, np.ascontiguousarray(ml)), "the distances restated here are not the max-log specification's"
    return m0, m1


def correction(d, m0, m1, inv_s):
    """c1 - c0 [..., m] in float64 from the float32 distances d [..., 2^m], minima and scale"""
    m = m0.shape[-1]
    d64, s64 = d.astype(np.float64), inv_s.astype(np.float64)[..., None]
    out = np.empty(m0.shape, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j, one in enumerate(_masks(m)):
            c0 = np.log(np.exp(-(d64[..., ~one] - m0[..., j:j + 1].astype(np.float64)) * s64).sum(axis=-1))
            c1 = np.log(np.exp(-(d64[..., one] - m1[..., j:j + 1].astype(np.float64)) * s64).sum(axis=-1))
            out[..., j] = c1 - c0
    return out


def correction32(d, m0, m1, inv_s):
    """the same in float32, the device's operation order: t = fl(fl(m_v - d_p) inv_s), the sums in label order"""
    m = m0.shape[-1]
    out = np.empty(m0.shape, np.float32)
    s = inv_s[..., None]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for j, one in enumerate(_masks(m)):
            c = []
            for mv, sel in ((m0[..., j:j + 1], ~one), (m1[..., j:j + 1], one)):
                e = np.exp((mv - d[..., sel]) * s)
                acc = e[..., 0]
                for p in range(1, e.shape[-1]):
                    acc = acc + e[..., p]
                assert acc.dtype == np.float32
                c.append(np.log(acc))
            out[..., j] = c[1] - c[0]
    return out


def _add(ml, corr):
    """ml + corr, and ml as it is where corr is zero"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(corr != 0, ml + corr, ml)


def _table_parts(points, sym, nv, a):
    sym = np.asarray(sym, np.float32)
    m = ms.bits_per_symbol(points)
    if a is None:
        ml, inv_s = ms.symbol_llrs(points, sym, nv), np.full(sym.shape[:-1], np.float32(1.0 / (2.0 * float(nv))), np.float32)
    else:
        ml, inv_s = fs.symbol_llrs(points, sym, a, nv), fs.inv_rule(nv, a)
    d = table_distances(points, sym)
    m0, m1 = _checked_maxlog(d, inv_s, ml)
    assert ml.shape[-1] == m
    return [(ml, d, m0, m1, inv_s)]


def _product_parts(levels_i, levels_q, sym, nv, a):
    sym = np.asarray(sym, np.float32)
    b = ps.bits_per_axis(levels_i, levels_q)
    if a is None:
        ml, inv_s = ps.symbol_llrs(levels_i, levels_q, sym, nv), np.full(sym.shape[:-1], np.float32(1.0 / (2.0 * float(nv))), np.float32)
    else:
        ml, inv_s = fs.symbol_llrs_product(levels_i, levels_q, sym, a, nv), fs.inv_rule(nv, a)
    parts = []
    for k, lev in enumerate((levels_i, levels_q)):
        d = axis_distances(lev, sym[..., k])
        mlk = ml[..., k * b:(k + 1) * b]
        m0, m1 = _checked_maxlog(d, inv_s, mlk)
        parts.append((mlk, d, m0, m1, inv_s))
    return parts


def _llrs(parts, f32):
    if f32:
        out = [_add(ml, correction32(d, m0, m1, inv_s)) for ml, d, m0, m1, inv_s in parts]
        assert all(o.dtype == np.float32 for o in out)
    else:
        out = [_add(ml.astype(np.float64), correction(d, m0, m1, inv_s)) for ml, d, m0, m1, inv_s in parts]
    return np.concatenate(out, axis=-1)


def _collapsed(parts):
    out = []
    for ml, d, m0, m1, inv_s in parts:
        m = m0.shape[-1]
        ok = np.empty(m0.shape, bool)
        with np.errstate(invalid="ignore", over="ignore"):
            for j, one in enumerate(_masks(m)):
                ok[..., j] = True
                for mv, sel in ((m0[..., j:j + 1], ~one), (m1[..., j:j + 1], one)):
                    t = (d[..., sel].astype(np.float64) - mv.astype(np.float64)) * inv_s.astype(np.float64)[..., None]
                    ok[..., j] &= ((t > COLLAPSE).sum(axis=-1) == t.shape[-1] - 1)       # all but the one minimum (a tie fails)
        out.append(ok)
    return np.concatenate(out, axis=-1)


def _maxlog(parts):
    return np.concatenate([p[0] for p in parts], axis=-1)


def llrs(points, sym, nv, a=None):
    """a table object: sym [..., 2] float32, a [...] float32 gains or None -> LLRs [..., m] float64"""
    return _llrs(_table_parts(points, sym, nv, a), False)


def llrs32(points, sym, nv, a=None):
    """the float32 restatement -> [..., m] float32"""
    return _llrs(_table_parts(points, sym, nv, a), True)


def collapsed(points, sym, nv, a=None):
    """[..., m] bool: every (d_p - m_v) inv_s of both subsets but the minimum's exceeds 104 -- there the rule gives max-log's bits"""
    return _collapsed(_table_parts(points, sym, nv, a))


def maxlog(points, sym, nv, a=None):
    return _maxlog(_table_parts(points, sym, nv, a))


def llrs_product(levels_i, levels_q, sym, nv, a=None):
    """a product object: -> LLRs [..., 2 b] float64, the I bits, then the Q bits"""
    return _llrs(_product_parts(levels_i, levels_q, sym, nv, a), False)


def llrs32_product(levels_i, levels_q, sym, nv, a=None):
    return _llrs(_product_parts(levels_i, levels_q, sym, nv, a), True)


def collapsed_product(levels_i, levels_q, sym, nv, a=None):
    return _collapsed(_product_parts(levels_i, levels_q, sym, nv, a))


def maxlog_product(levels_i, levels_q, sym, nv, a=None):
    return _maxlog(_product_parts(levels_i, levels_q, sym, nv, a))


def bound(want, terms=1, mag=None):
    """the GPU bar per element for a value that sums `terms` LLRs (an array or 1): terms (2^-14 + 2 ulp32) + (terms - 1) ulp32 -- one ulp
    per addition -- the ulp that of mag + terms 2^-14, mag = the sum of the |LLR| (None: |want|, one term); inf where want is not finite"""
    want = np.asarray(want, np.float64)
    terms = np.asarray(terms, np.float64)
    mag = np.abs(want) if mag is None else np.asarray(mag, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ulp = np.spacing(np.where(np.isfinite(want), mag + terms * BAR, 0.0).astype(np.float32)).astype(np.float64)
        return np.where(np.isfinite(want), terms * (BAR + 2.0 * ulp) + np.maximum(terms - 1.0, 0.0) * ulp, np.inf)


def brute_force(points, sym, nv, a=None):
    """float64 log-sum-exp over ALL points from float64 distances -> (LLRs [..., m] float64, max_p d_p inv [...])"""
    pts = np.asarray(points, np.float32).astype(np.float64)
    m = len(pts).bit_length() - 1
    sym = np.asarray(sym, np.float32).astype(np.float64)
    inv = 1.0 / (2.0 * float(nv)) if a is None else fs.inv_rule(nv, a).astype(np.float64)
    inv = np.broadcast_to(np.float64(np.float32(inv)) if a is None else inv, sym.shape[:-1])[..., None]
    x = -((sym[..., None, 0] - pts[:, 0]) ** 2 + (sym[..., None, 1] - pts[:, 1]) ** 2) * inv
    out = np.empty(sym.shape[:-1] + (m,))
    lab = np.arange(1 << m)
    for j in range(m):
        one = ((lab >> (m - 1 - j)) & 1).astype(bool)
        l = []
        for sel in (~one, one):
            top = x[..., sel].max(axis=-1, keepdims=True)
            l.append(top[..., 0] + np.log(np.exp(x[..., sel] - top).sum(axis=-1)))
        out[..., j] = l[1] - l[0]
    return out, (-x).max(axis=-1)


def to_f16(llr32):
    return ms.round_f16(np.asarray(llr32, np.float32))


def to_i8(llr32, qscale):
    return layered_i8_spec.quantize(np.asarray(llr32, np.float32), qscale).astype(np.int8)


def place(per, n_tx, N):
    """per [B][n_sym][m] -> rows [B][N]: the LLRs of the first n_tx bits, then zeros (modulation_spec.demap's layout)"""
    B = per.shape[0]
    out = np.zeros((B, N), per.dtype)
    out[:, :n_tx] = per.reshape(B, -1)[:, :n_tx]
    return out
