"""CPU: tests/demap_apriori_spec.py on the inputs of tests/demap_apriori_cases.py.  With La = 0 it is the shipped demapper up to the rounding its
docstring derives; the float32 max-log rule lies within its rounding count of the same formula in float64; the float32 log-MAP restatement
lies inside the bar that docstring derives (the project's bar for the exact rule plus the max-log roundings) of the float64 brute force
-- the bar the device is held to; knowledge that agrees with the sent labels strengthens every decision; the value is extrinsic."""
import numpy as np
import pytest

from tests import demap_apriori_cases as K
from tests import demap_apriori_spec as spec
from tests import demap_logmap_cases as cl
from tests import fading_spec as fs
from tests import modulation_spec as ms

ALL = [(n, lv, sh) for n in K.IDS for lv in K.LEVELS for sh in K.SHAPES]


def test_apriori_sums_by_hand():
    la = np.array([1.0, 10.0, 100.0], np.float32)           # label bits MSB first
    assert spec.apriori_sums(la).tolist() == [0.0, 100.0, 10.0, 110.0, 1.0, 101.0, 11.0, 111.0]
    # the order of the additions: ((La_0 + La_1) + La_2), not any other
    la = np.array([1.0, 2.0 ** -24, 2.0 ** -24], np.float32)
    assert spec.apriori_sums(la)[7] == np.float32(1.0) and np.float32(1.0) + (np.float32(2.0 ** -24) + np.float32(2.0 ** -24)) != np.float32(1.0)
    assert np.signbit(spec.apriori_sums(np.array([-0.0, 5.0], np.float32))[2]) and not np.signbit(spec.apriori_sums(np.array([-0.0, 5.0], np.float32))[0])


@pytest.mark.parametrize("name,level,shape", ALL, ids=["-".join(x) for x in ALL])
def test_zero_apriori_is_the_shipped_demapper_up_to_rounding(name, level, shape):
    c = cl.case("table", name)
    sym, a, pos, N, nv = K.inputs(name, level, shape)
    new, inv_s, la = K.reference(name, level, shape, "zero", spec.MAXLOG)
    assert not la.any()
    old = ms.symbol_llrs(c.pts, sym, nv) if a is None else fs.symbol_llrs(c.pts, sym, a, nv)
    bar = spec.zero_apriori_bar(c.pts, sym, inv_s)
    nan = np.isnan(old)
    assert np.array_equal(nan, np.isnan(new)) and (a is None or nan.any()) and (~nan).sum() > nan.sum()
    err = np.abs(new.astype(np.float64) - old.astype(np.float64))
    assert (err[~nan] <= bar[~nan]).all(), (name, level, shape, float((err[~nan] / np.maximum(bar[~nan], 1e-300)).max()))
    if a is not None:                                       # a gain of 0: an erasure under both
        assert not new[0, 1].any() and not old[0, 1].any()
    # the placed rows: zeros at the punctured positions, the formats
    rows = spec.demap_il_apriori(c.pts, sym, a, pos, N, nv, K.apriori(name, level, shape, "zero"))
    assert rows.shape == (K.B, N) and not rows[:, np.setdiff1d(np.arange(N), pos)].any()


@pytest.mark.parametrize("which", ["normal", "genie"])
@pytest.mark.parametrize("name,level,shape", ALL, ids=["-".join(x) for x in ALL])
def test_float32_rules_against_float64(name, level, shape, which):
    c = cl.case("table", name)
    for rule in (spec.MAXLOG, spec.LOGMAP):
        got, inv_s, la = K.reference(name, level, shape, which, rule)
        want, T, A, mag = K.brute(name, level, shape, which, rule)
        ok = np.isfinite(want)
        assert np.array_equal(ok, np.isfinite(got)) and ok.sum() > 0.9 * ok.size
        err = np.abs(got.astype(np.float64) - want)
        if rule == spec.MAXLOG:
            bar = np.broadcast_to(spec.maxlog_bar(c.m, T, A)[..., None], want.shape)
        else:
            bar = spec.logmap_bar(want, c.m, T, A)
        assert (err[ok] <= bar[ok]).all(), (name, level, shape, which, rule, float((err[ok] / bar[ok]).max()))
    # log-MAP is max-log plus a correction: none with one point a subset (m = 1); one that matters at "low" with moderate knowledge and
    # m >= 3 (QPSK's two subsets of a bit mirror each other: c1 = c0; +-30 on the other bits leaves one point a subset that counts)
    ml, lm = K.reference(name, level, shape, which, spec.MAXLOG)[0], K.reference(name, level, shape, which, spec.LOGMAP)[0]
    fin = np.isfinite(ml)
    if c.m == 1:
        assert np.array_equal(ml[fin], lm[fin])
    elif level == "low" and which == "normal" and c.m >= 3:
        assert np.abs(lm[fin] - ml[fin]).max() > 1e-2


@pytest.mark.parametrize("name,level", [(n, lv) for n in K.IDS for lv in K.LEVELS])
def test_genie_knowledge_helps_and_the_value_is_extrinsic(name, level):
    c = cl.case("table", name)
    shape = "aligned"
    sym, a, pos, N, nv = K.inputs(name, level, shape)
    ns = sym.shape[1]
    lab = K.sent_labels(c, ns, level, K.SEED[shape])
    sent = ((lab[..., None] >> (c.m - 1 - np.arange(c.m))) & 1).astype(bool)
    genie, _, la = K.reference(name, level, shape, "genie", spec.MAXLOG)
    assert np.array_equal(la > 0, sent) and (np.abs(la) == 30).all()
    zero = K.reference(name, level, shape, "zero", spec.MAXLOG)[0]
    if c.m > 1:
        # with the other bits of the label known, a bit's LLR is the distance difference of ONE pair of points: it points at the sent bit
        # whenever the sample is nearer to the sent point than to its neighbour across that bit -- more often than without knowledge
        assert ((genie > 0) == sent).mean() >= ((zero > 0) == sent).mean()
    # extrinsic: adding a constant to ONE bit's La changes the other bits' LLRs of its symbol, not its own (up to the roundings)
    la2 = la.copy()
    la2[..., 0] += np.float32(8.0)
    inv_s = spec.inv_scale(sym.shape[:-1], nv, a)
    moved = spec.symbol_llrs(c.pts, sym, inv_s, la2)
    assert np.abs(moved[..., 0] - genie[..., 0]).max() <= 1e-4 * max(1.0, float(np.abs(genie[..., 0]).max()))


def test_the_abi_declares_the_entry_point():
    import ecc_ldpc_amd as E
    assert "ldpc_demap_dev_il_apriori" in E.ABI_SYMBOLS and "ldpc_decode_batch_dev_soft" in E.ABI_SYMBOLS and callable(E.demap_il_apriori)
