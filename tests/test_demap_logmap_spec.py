"""CPU: the specification of the log-MAP LLR rule (tests/demap_logmap_spec.py).

  1. against a brute-force float64 log-sum-exp over ALL points, from float64 distances: table objects m = 1..6, and product objects
     b = 1..3 as the full two-dimensional sum over their 4^b materialised points -- the proof that the per-axis rule is exact.  The two
     differ by the float32 rounding of the distances only: the bound is 2^-20 (1 + max_p d_p inv) per element;
  2. the fixed points: m = 1 and b = 1 give max-log's bits; so does every element at the collapse point whose other terms lie past 104;
     a gain of 0 gives the max-log zero; a NaN sample or gain gives NaN where max-log does, and nowhere else;
  3. the float32 restatement stays inside the GPU bar (demap_logmap_spec.bound) of the float64 specification on every input of
     tests/test_demap_logmap_gpu.py: this is what justifies the bar;
  4. the corrections are what the bar is small against: at the low level they reach 0.1 and more."""
import numpy as np
import pytest

from tests import demap_logmap_cases as lc
from tests import demap_logmap_spec as ls
from tests import product_modulation_spec as ps


def _bits(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), 0, a.view(np.uint32))


ALL_POINTS = [(k, n) for k, n in lc.OBJECTS if k == "table" or n <= 3]       # the sum over 4^b points is run for b = 1..3


@pytest.mark.parametrize("kind,n", ALL_POINTS, ids=[f"{k}-{n}" for k, n in ALL_POINTS])
def test_spec_against_the_sum_over_all_points(kind, n):
    c = lc.case(kind, n)
    pts = c.pts if kind == "table" else ps.materialise(c.li, c.lq)
    for level in lc.LEVELS:
        for name, (sym, a) in lc.inputs(c, level).items():
            nv = c.noise_var(level)
            got = c.spec("llrs", sym, nv, a)
            want, dmax = ls.brute_force(pts, sym, nv, a)
            ok = np.isfinite(want)
            assert np.array_equal(np.isnan(got), np.isnan(want)) and ok.any()
            err = np.abs(got - want)[ok]
            lim = (2.0 ** -20 * (1.0 + dmax))[..., None] * np.ones(got.shape[-1])
            assert (err <= lim[ok]).all(), (level, name, err.max())


@pytest.mark.parametrize("kind,n", lc.OBJECTS, ids=lc.IDS)
def test_fixed_points_and_the_float32_restatement(kind, n):
    c = lc.case(kind, n)
    worst, biggest = 0.0, 0.0
    for level in lc.LEVELS:
        nv = c.noise_var(level)
        for name, (sym, a) in lc.inputs(c, level).items():
            want, got, ml = c.spec("llrs", sym, nv, a), c.spec("llrs32", sym, nv, a), c.spec("maxlog", sym, nv, a)
            nan = np.isnan(ml)
            assert np.array_equal(np.isnan(want), nan) and np.array_equal(np.isnan(got), nan)
            if a is not None:                                   # a NaN gain: its whole symbol; a gain of 0: the max-log zero
                assert np.array_equal(nan, np.broadcast_to(np.isnan(a)[..., None], nan.shape)) and nan.any()
                zero = np.broadcast_to((a == 0)[..., None], nan.shape)
                assert zero.any() and np.array_equal(_bits(got)[zero], _bits(ml)[zero]) and (want[zero] == 0).all()
            if c.single:
                assert np.array_equal(_bits(got), _bits(ml)) and np.array_equal(want[~nan], ml[~nan].astype(np.float64))
            fixed = c.spec("collapsed", sym, nv, a) & ~nan
            assert np.array_equal(_bits(got)[fixed], _bits(ml)[fixed]) and np.array_equal(want[fixed], ml[fixed].astype(np.float64))
            if level == "collapse":
                assert fixed.mean() > 0.5, (name, fixed.mean())
            gap = np.abs(got.astype(np.float64) - want)[~nan]
            assert (gap <= ls.bound(want)[~nan]).all(), (level, name, gap.max())
            worst = max(worst, float((gap / ls.bound(want)[~nan]).max()))
            if level == "low":
                biggest = max(biggest, float(np.abs(want - ml)[~nan].max()))
    print(f"{kind}-{n}: the float32 restatement uses at most {worst:.3f} of the bar; largest correction at the low level {biggest:.3f}")
    assert c.m <= 2 or biggest > 0.1             # (BPSK: no correction; QPSK, b = 1: the rule factors per axis and the correction cancels)


def test_the_separated_rule_on_a_nan_coordinate():
    """a NaN in one coordinate: the LLRs of that axis alone are NaN (a table object: all of them)"""
    c = lc.case("product", 3)
    sym = c.samples(4, "mid", 9)
    sym[0, 1, 0], sym[1, 2, 1], sym[2, 0, 0] = np.nan, np.nan, np.inf
    got = c.spec("llrs", sym, c.noise_var("mid"))
    want = np.zeros(got.shape, bool)
    want[0, 1, :3], want[1, 2, 3:], want[2, 0, :3] = True, True, True
    assert np.array_equal(np.isnan(got), want) and np.array_equal(np.isnan(c.spec("llrs32", sym, c.noise_var("mid"))), want)
    t = lc.case("table", "8psk")
    sym = t.samples(4, "mid", 9)
    sym[0, 1, 0] = np.nan
    assert np.isnan(t.spec("llrs", sym, t.noise_var("mid"))[0, 1]).all()


def test_converters():
    v = np.array([0.3, -0.3, 1e6, np.nan, -0.0], np.float32)
    assert ls.to_f16(v).dtype == np.float16 and ls.to_f16(v)[2] == 65504.0 and np.isnan(ls.to_f16(v)[3])
    assert ls.to_i8(v, 4.0).tolist() == [1, -1, 127, 0, 0]
