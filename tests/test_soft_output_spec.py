"""CPU: tests/soft_output_spec.py against the specification it extends, tests/layered_rule_spec.py decode, on the three graphs of
tests/layered_shapes.py, the three cells and both rules: the same bits, sweeps and flags on every frame, P = final_lam where a frame
converged, P != the channel LLRs where it ran out of sweeps (the case final_lam does not give), E = P - C, and the output formats."""
import numpy as np
import pytest

from tests import soft_output_cases as K
from tests import soft_output_spec as spec

CASES = [(n, c, r) for n in K.NAMES for c in K.CELLS for r in (False, True)]
IDS = [f"{n}-{c}-{'ruled' if r else 'plain'}" for n, c, r in CASES]


@pytest.mark.parametrize("name,cell,ruled", CASES, ids=IDS)
def test_same_decisions_and_the_posterior(name, cell, ruled):
    rule = K.rule_of(name, cell, ruled)
    for mi in (0, 1, K.SWEEPS):
        bits, sweeps, conv, P, C = K.ref(name, cell, rule, mi)
        sb, ss, sc, sl = K.shipped(name, cell, rule, mi)
        what = (name, cell, rule, mi)
        assert np.array_equal(bits, sb) and np.array_equal(sweeps, ss) and np.array_equal(conv, sc), what
        lam = P.astype(np.float64) / K.QSCALE if cell == "i8" else P.astype(np.float64)        # (final_lam of int8 cells is q / qscale)
        assert conv.any() and np.array_equal(lam[conv], sl[conv]), what
        if mi == 0:
            assert np.array_equal(P, C), what
    bits, sweeps, conv, P, C = K.ref(name, cell, rule, K.SWEEPS)
    assert K.exercised(sweeps, conv), (name, cell, rule, sweeps, conv)
    out = ~conv
    assert out[:8].any() and (P[out] != C[out]).any(axis=1).all(), (name, cell, rule)         # every frame out of sweeps has moved
    assert np.array_equal(bits[out], (C[out] > 0).astype(np.uint8))                            # and still returns the channel's decisions
    assert conv[8] and conv[9] and sweeps[8] == 0 and sweeps[9] == 0 and np.array_equal(P[8:], C[8:])     # codewords before the first sweep


@pytest.mark.parametrize("cell", K.CELLS)
def test_extrinsic_and_formats(cell):
    name = "w20"
    _, _, conv, P, C = K.ref(name, cell, K.PLAIN, K.SWEEPS)
    E = spec.value(cell, P, C, "extrinsic")
    assert spec.value(cell, P, C, "posterior") is P
    if cell == "i8":
        assert E.dtype == np.int32 and np.array_equal(E, P - C) and np.abs(E).max() <= 254 and np.abs(E).max() > 127
        assert np.array_equal(spec.output(cell, E, "i8"), np.clip(E, -127, 127).astype(np.int8))
        assert np.array_equal(spec.output(cell, P, "f32"), (P / np.float32(K.QSCALE)).astype(np.float32))
        assert np.array_equal(spec.output(cell, P, "f16").astype(np.float32), spec.output(cell, P, "f32"))      # k / 4, |k| <= 127: exact
    else:
        assert E.dtype == np.float32 and np.array_equal(E, (P - C).astype(np.float32)) and np.any(E != 0)
        assert np.array_equal(E[8:], np.zeros_like(E[8:]))
        assert spec.output(cell, E, "f32") is E or np.array_equal(spec.output(cell, E, "f32"), E)
        h = spec.output(cell, P, "f16")
        assert h.dtype == np.float16
        if cell == "f16":
            assert np.array_equal(h.astype(np.float32), P)                                   # the cell's own bits
        q = spec.output(cell, P, "i8")
        assert q.dtype == np.int8 and np.array_equal(q, spec.quantize(P, 4.0)) and np.abs(q.astype(int)).max() == 127
        assert np.array_equal(spec.output(cell, P, "i8", 2.0), spec.quantize(P, 2.0))


def test_f16_output_saturates_and_keeps_a_nan():
    v = np.array([1e9, -1e9, np.inf, -np.inf, np.nan, 65520.0, 0.1], np.float32)
    h = spec.output("f32", v, "f16")
    assert np.array_equal(h[:4].astype(np.float32), [65504, -65504, 65504, -65504]) and np.isnan(h[4]) and h[5] == 65504 and h[6] == np.float16(0.1)
    q = spec.output("f32", v, "i8")
    assert q.tolist() == [127, -127, 127, -127, 0, 127, 0]


def test_the_veto_keeps_lam_as_it_stands():
    """an f32 frame with an infinity (at a column whose rows all have three edges or more: no inf - inf) converges, is failed by the veto and
    keeps the lam it stopped with; a NaN in the noiseless codeword stops the frame before the first sweep"""
    name = "w20"
    llr, f, col, (bits, sw, cv, P, C) = K.nonfinite(name)
    assert not cv[f] and sw[f] == K.SWEEPS and np.isneginf(P[f, col]) and not np.isnan(P[f]).any() and (P[f] != C[f]).any()
    assert np.array_equal(bits[f], (C[f] > 0).astype(np.uint8))
    assert not cv[9] and sw[9] == K.SWEEPS and np.array_equal(P[9].view(np.uint32), llr[9].view(np.uint32)) and np.isnan(P[9, 5])
    others = [i for i in range(10) if i not in (f, 9)]
    for got, want in zip((bits, sw, cv, P, C), K.ref(name, "f32", K.PLAIN, K.SWEEPS)):
        assert np.array_equal(got[others], want[others])
