"""CPU: what tests/test_real_codewords_gpu.py rests on, asserted on the references alone (no GPU).

1. tests/codewords.py gives real codewords of every code that module decodes: H c = 0, and -- but for the two degenerate codes, whose
   only words are the zero word (latin-18x9-sz40, rank N) or the zero and the all-ones word (latin-24x16-sz64, rank N - 1) -- between
   0.35 N and 0.65 N ones in every drawn word.
2. On the exact frames of every case the reference of its family has the two kinds of frame the case is there for (one that converges
   after more than one turn, one that runs out), and it is SYMMETRIC: the mirror images (LLRs negated where the codeword is 1) stop at the
   same turn with the same flag, with final_lam negated at those positions bit for bit and the bits XOR the codeword wherever
   final_lam != 0.  The Double oracle with the min rule is symmetric in its whole trajectory; with the tanh rule its final LLRs move in the
   last places (0.5 log((1 + p) / (1 - p)) is not odd in floating point), so bits, turns and flags only, and final_lam to 1e-9.
3. For the f32 contexts whose only reference is the Double oracle, no LLR of the oracle's trajectory is exactly zero within the turns run
   (a float and the Double could then decide a bit differently with neither being wrong), and for the layered f32 kernels the
   specification they are held to bit for bit (tests/layered_rule_spec.py, cell "f32") gives the Double oracle's bits and flags, turn
   counts within helpers.iters_agree.

Frames that break a premise are replaced here, by another seed for the whole case (tests/real_codeword_cases.py Case.seed), never skipped on
the GPU.  Two cases needed it, both of the int8 cell, whose quantised lam is often exactly zero -- and hard(0) = 0 is the all-zero word's
bit, so the stop rule of a frame and of its mirror image can fire a sweep apart ON THE SPECIFICATION: layered_csr-i8-plain-w20 (seed 1:
frame 1 of 10) and layered_csr-i8-ruled-half-w8 (seed 1: frame 5 of 10) use seed 2, under which all ten frames are symmetric.  Every
other case uses seed 1 with no frame dropped."""
import numpy as np
import pytest

from tests import codewords as cwm
from tests import real_codeword_cases as R
from tests.helpers import iters_agree

CODE_NAMES = sorted({c.code for c in R.CASES})
UNIQUE = list({c.ref_key: c for c in R.CASES}.values())          # one case per (frames, reference)


def _syndrome(g, cw):
    s = np.zeros((len(cw), g.M), np.int64)
    rows = np.repeat(np.arange(g.M), np.diff(g.row_ptr))
    for f in range(len(cw)):
        np.add.at(s[f], rows, cw[f][g.col_idx])
    return s & 1


@pytest.mark.parametrize("name", CODE_NAMES)
def test_every_code_yields_codewords(name):
    c = R.code(name)
    if R.DEGENERATE.get(name) == 0:
        assert cwm.dimension(c.graph) == 0 and not cwm.codewords(c.graph, 3, 5).any()
        return
    cw = c.codewords(8, 5)
    assert cw.shape == (8, c.N) and cw.dtype == np.uint8 and not _syndrome(c.graph, cw).any()
    if name in R.DEGENERATE:
        assert cwm.dimension(c.graph) == 1 and set(cw.sum(1).tolist()) == {0, c.N}            # both words are drawn
        return
    ones = cw.sum(1)
    assert (ones >= 0.35 * c.N).all() and (ones <= 0.65 * c.N).all(), ones
    assert len({w.tobytes() for w in cw}) == 8
    assert np.array_equal(cw, c.codewords(8, 5)) and not np.array_equal(cw, c.codewords(8, 6))


def test_flip_and_the_frames():
    c = R.code("small-2x4-sz32")
    cw = c.codewords(4, 9)
    llr = cwm.noisy(cw, 3.0, c.k, c.N, 10)
    assert llr.dtype == np.float64 and np.array_equal(llr, llr.astype(np.float32)) and (llr != 0).all()
    f = cwm.flip(llr, cw)
    assert np.array_equal(f[cw == 1], -llr[cw == 1]) and np.array_equal(f[cw == 0], llr[cw == 0]) and np.array_equal(cwm.flip(f, cw), llr)
    assert cwm.flip(llr.astype(np.float16), cw).dtype == np.float16
    # most decisions of a frame at 3 dB are the codeword's: the mirror image is a frame of the all-zero word
    assert ((llr > 0) == cw).mean() > 0.8 and (f > 0).mean() < 0.2
    two = cwm.noiseless(cw[0])
    assert np.array_equal(two[0] > 0, cw[0] == 1) and (np.abs(two) == 8).all() and (two[1] == -8).all()
    with pytest.raises(AssertionError):
        cwm.noisy(cw, 3.0, c.k, c.N + 1, 10)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_frames_of_every_case(case):
    llr, cws = R.frames_of(case)
    c = R.code(case.code)
    assert llr.shape == cws.shape == (case.F + 2, c.N) and 4 <= case.F <= 16 and not _syndrome(c.graph, cws).any()
    assert np.isfinite(llr).all() and (llr != 0).all() and np.array_equal(llr, llr.astype(np.float32))
    assert (np.abs(llr[case.F:]) == 8).all() and np.array_equal(llr[case.F] > 0, cws[case.F] == 1) and (llr[case.F + 1] < 0).all()
    if case.code not in R.DEGENERATE:
        assert cws.any(axis=1).all()


@pytest.mark.parametrize("case", UNIQUE, ids=lambda c: c.id)
def test_the_reference_is_exercised_and_symmetric(case):
    llr, cws = R.frames_of(case)
    ref = R.reference_of(case)
    assert R.exercised(case, ref), (ref[1], ref[2])
    assert ref[2][case.F:].all() and (ref[1][case.F:] == 0).all()                  # the noiseless frames: codewords before the first turn
    assert np.array_equal(ref[0][case.F], cws[case.F]) and not ref[0][case.F + 1].any()
    mir = R.compute_reference(case, cwm.flip(llr, cws))
    assert np.array_equal(mir[1], ref[1]) and np.array_equal(mir[2], ref[2]), (mir[1], ref[1])
    want = R.mirrored(ref, cws)
    if case.ref in ("oracle", "oracle-layered") and case.variant == "tanh":
        assert np.array_equal(mir[0], want[0])
        assert (np.abs(mir[3] - want[3]) <= 1e-9 * np.maximum(1, np.abs(want[3]))).all()
        return
    assert np.array_equal(mir[3], want[3])                                          # final_lam, bit for bit (-0 == +0: no bit hangs on it)
    decided = ref[3] != 0
    assert np.array_equal(mir[0][decided], want[0][decided])
    if case.ref in ("oracle", "oracle-layered"):                                    # the Double oracle, min: the whole trajectory
        assert np.array_equal(mir[0], want[0])
        for f, (a, b) in enumerate(zip(mir[4], ref[4])):
            assert np.array_equal(a["trace_lam"], cwm.flip(b["trace_lam"], np.tile(cws[f], (len(b["trace_lam"]), 1))))
    elif ref[4] is not None:                                                        # the fp16 emulations: every turn of the trajectory
        assert len(mir[4]) == len(ref[4])
        for a, b in zip(mir[4], ref[4]):
            assert np.array_equal(a, cwm.flip(b, cws))


F32_VS_DOUBLE = [c for c in R.CASES if c.dtype == "f32" and (c.ref == "oracle" or c.ref == ("spec", "f32")) and c.rule is None]


@pytest.mark.parametrize("case", list({(c.ref_key): c for c in F32_VS_DOUBLE}.values()), ids=lambda c: c.id)
def test_premises_of_f32_against_the_double_oracle(case):
    llr, _ = R.frames_of(case)
    layered = case.schedule == "layered"
    o = R._oracle(R.code(case.code), case.variant, llr, layered)
    for x in o[4]:
        assert (x["trace_lam"] != 0).all()
    if layered:
        ref = R.reference_of(case)
        assert np.array_equal(ref[0], o[0]) and np.array_equal(ref[2], o[2]) and iters_agree(ref[1], o[1]), (ref[1], o[1])
        assert R.exercised(case, o)
