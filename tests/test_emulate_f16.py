"""CPU: sanity of the fp16-storage emulation used as the checker of the LDPC_F16 contexts (oracle/emulate_f16.py)
against the double-precision oracle and the behavioural invariants of the reference loop (Min.hs:54-104)."""
import numpy as np

from oracle import emulate_f16 as em
from oracle import oracle
from tests.helpers import load


def test_r16_saturates_and_rounds_to_nearest_even():
    x = np.array([7e4, -7e4, 65504.0, 65520.0, 1e-9, 0.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 3.0e-8], np.float32)
    want = np.array([65504.0, -65504.0, 65504.0, 65504.0, 0.0, 0.0, 1.0, 1.0 + 2.0 ** -9, 0.0, 2.0 ** -24 * 1], np.float32)
    assert np.array_equal(em.r16(x), want)


def test_cn_minsum_matches_the_oracle_rule():
    c = load("moon.7.13")
    rng = np.random.default_rng(5)
    lam = em.r16(rng.normal(0, 4, (3, c.N)))
    ne = em.r16(rng.normal(0, 1, (3, c.E)))
    for f in range(3):
        o_ne, _, _ = oracle.step(c.graph, "min", np.zeros(c.N), lam[f].astype(np.float64), ne[f].astype(np.float64))
        e_ne, _, _ = em.step_minsum_f16_flood(c.graph, lam[f:f + 1] * 0, lam[f:f + 1], ne[f:f + 1])
        # same rule; the emulation subtracts in f32 and stores fp16
        t_ok = np.abs(e_ne[0] - o_ne) <= np.abs(o_ne) * 2.0 ** -10 + 1e-7
        assert t_ok.all()


def test_invariants_and_agreement_with_the_f64_oracle():
    c = load("jpl.1024.4.5")
    cws, llr = c.frames(6, 4.0, seed=31)
    llr = llr.astype(np.float32)
    bits, its, conv, trace = em.decode_minsum_f16_flood(c.graph, llr, 50)
    for f in range(len(llr)):                       # well above the waterfall: both decoders return the codeword
        o = oracle.decode(c.graph, "min", 50, llr[f].astype(np.float64))
        assert conv[f] and o["converged"] and np.array_equal(bits[f], o["bits"]) and np.array_equal(bits[f], cws[f])
        assert abs(int(its[f]) - o["iters"]) <= 2
    # noiseless codeword: 0 iterations, output = codeword; all-zero LLRs: 0 iterations, all False (hard 0 = False)
    clean = np.where(cws[:2] > 0, 8.0, -8.0).astype(np.float32)
    b, i, cv, _ = em.decode_minsum_f16_flood(c.graph, clean, 50)
    assert (i == 0).all() and cv.all() and np.array_equal(b, cws[:2])
    b, i, cv, _ = em.decode_minsum_f16_flood(c.graph, np.zeros((1, c.N), np.float32), 50)
    assert i[0] == 0 and cv[0] and not b.any()
    # out of turns -> hard(channel LLRs) (Min.hs:76)
    _, noisy = c.frames(2, 0.0, seed=32)
    b, i, cv, _ = em.decode_minsum_f16_flood(c.graph, noisy.astype(np.float32), 5)
    assert (i == 5).all() and not cv.any() and np.array_equal(b, (em.r16(noisy) > 0).astype(np.uint8))


# ---- non-finite channel LLRs (include/ldpc_hip.h, rule 1): a NaN is an erasure, +0; an infinity saturates like any other value
F16_PATTERNS = np.array([0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01], np.uint16).view(np.float16)   # +inf, -inf, NaN, -NaN, a signalling NaN


def _nans_f32():
    return np.array([0x7FC00000, 0xFFC00000], np.uint32).view(np.float32)       # NaN with the sign bit clear and set


def test_r16_takes_a_nan_as_plus_zero_and_saturates_infinities():
    nan = _nans_f32()
    assert np.isnan(nan).all() and np.signbit(nan).tolist() == [False, True]
    x = np.concatenate([nan, np.array([np.inf, -np.inf, 1e30, -1e30], np.float32)])
    got = em.r16(x)
    assert np.array_equal(got, np.array([0, 0, 65504, -65504, 65504, -65504], np.float32))
    assert not np.signbit(got[:2]).any()                     # +0, not -0
    assert np.isnan(F16_PATTERNS[2:]).all() and np.isinf(F16_PATTERNS[:2]).all()
    got = em.r16(F16_PATTERNS)                               # an fp16 input buffer holds them too
    assert np.array_equal(got, np.array([65504, -65504, 0, 0, 0], np.float32)) and not np.signbit(got[2:]).any()
    with np.errstate(over="ignore"):                          # a double beyond the float range is an infinity once it is a float
        assert np.array_equal(em.r16(np.array([1e300, -1e300]).astype(np.float32)), np.array([65504, -65504], np.float32))


def test_neg_llr16_takes_a_nan_as_plus_zero_and_saturates_infinities():
    x = np.concatenate([_nans_f32(), np.array([np.inf, -np.inf, 1e30, -1e30], np.float32)])
    got = em.neg_llr16(x)
    assert got.dtype == np.float16 and np.array_equal(got, np.array([0, 0, -16384, 16384, -16384, 16384], np.float16))
    assert not np.signbit(got[:2]).any()                     # L = -lam is never -0: its sign bit IS the hard decision
    got = em.neg_llr16(F16_PATTERNS)
    assert np.array_equal(got, np.array([-16384, 16384, 0, 0, 0], np.float16)) and not np.signbit(got[2:]).any()


def test_a_nan_decodes_like_a_zero_and_the_frame_is_an_ordinary_finite_frame():
    """every fp16 emulation: the frame with NaNs of both signs is the frame with +0 in their place -- bits, iters, flags, final lam --
    and an infinity is the frame with the format's largest value"""
    c = load("moon.7.13")
    _, llr = c.frames(6, 3.0, seed=77)
    llr = llr.astype(np.float32)
    poisoned, clean = llr.copy(), llr.copy()
    poisoned[0, 3], poisoned[1, 5], poisoned[2, :] = _nans_f32()[0], _nans_f32()[1], np.nan
    clean[0, 3], clean[1, 5], clean[2, :] = 0.0, 0.0, 0.0
    poisoned[3, 2], poisoned[4, 7] = np.inf, -np.inf
    # (decode_minsum_pk16, the flooding packed-fp16 kernel, is not under rule 1 yet: test_flooding_pk16_takes_a_nan_as_minus_16384)
    for emu, top in ((em.decode_minsum_f16_flood, 65504.0), (em.decode_minsum_f16_layered, 65504.0), (em.decode_minsum_pk16_layered, 16384.0)):
        clean[3, 2], clean[4, 7] = top, -top
        a, b = emu(c.graph, poisoned, 20), emu(c.graph, clean, 20)
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])), emu.__name__
        last_a, last_b = (a[3], b[3]) if isinstance(a[3], np.ndarray) else (np.stack(a[3]), np.stack(b[3]))
        assert np.isfinite(last_a).all() and np.array_equal(last_a, last_b), emu.__name__
        assert a[2][2] and a[1][2] == 0 and not a[0][2].any()       # all NaN = all erased: the all-zero word, before any turn


def test_flooding_pk16_takes_a_nan_as_minus_16384():
    """the flooding packed-fp16 kernel keeps the plain saturation in its load (csrc/fused_frame.h LamCellPk16Sat): fmaxf(NaN, -M) = -M, so
    a NaN of either sign is the LLR -16384 there; infinities saturate as everywhere.  The emulation says what the kernel does."""
    x = np.concatenate([_nans_f32(), np.array([np.inf, -np.inf], np.float32)])
    assert np.array_equal(em.neg_llr16(x, nan_is_erasure=False), np.array([16384, 16384, -16384, 16384], np.float16))
    c = load("moon.7.13")
    _, llr = c.frames(3, 3.0, seed=78)
    llr = llr.astype(np.float32)
    a, b = llr.copy(), llr.copy()
    a[0, 3], a[1, 5] = _nans_f32()
    b[0, 3], b[1, 5] = -16384.0, -16384.0
    ra, rb = em.decode_minsum_pk16(c.graph, a, 20), em.decode_minsum_pk16(c.graph, b, 20)
    assert all(np.array_equal(u, v) for u, v in zip(ra[:3], rb[:3]))
