"""CPU: the specification of the two-stage decode, tests/cascade_spec.py -- compose on toy stage functions (no failure, every frame fails,
more failures than capacity), and on the two shipped specifications it was written for: 3/4 min-sum first, A-min* on the frames that did not
converge, on the AR4JA code at 3.0 dB."""
import functools

import numpy as np

from oracle import channel
from tests import cascade_spec as spec
from tests import layered_aminstar_spec as aminstar
from tests import layered_rule_spec as rule
from tests.helpers import load

N = 6


def _toy(fail, tag):
    """a stage that fails the frames whose first LLR is in `fail`: bits = tag for a converged frame, llr > 0 for a failed one; iters = tag
    or 10 * tag.  It records the rows it was given"""
    calls = []

    def stage(llr):
        calls.append(np.array(llr))
        bad = np.isin(llr[:, 0], list(fail))
        bits = np.where(bad[:, None], llr > 0, tag).astype(np.uint8)
        return bits, np.where(bad, 10 * tag, tag).astype(np.int32), (~bad).astype(np.uint8), "ignored"
    stage.calls = calls
    return stage


def _llr(F):
    llr = np.tile(np.float32([0, 1, -1, 2, -2, 3]), (F, 1))
    llr[:, 0] = np.arange(F)                                   # the frame's number rides in its first LLR
    return llr


def test_no_failure_leaves_stage_one_alone():
    s1, s2 = _toy((), 1), _toy((), 2)
    bits, iters, conv, stage, stats = spec.compose(s1, s2, _llr(5), 3)
    assert (bits == 1).all() and (iters == 1).all() and conv.all() and (stage == 1).all()
    assert stats.dtype == np.uint32 and stats.tolist() == [0, 0, 0] and not s2.calls
    assert (bits.dtype, iters.dtype, conv.dtype, stage.dtype) == (np.uint8, np.int32, np.uint8, np.uint8)


def test_every_frame_fails_and_goes_on():
    F = 5
    llr = _llr(F)
    s1, s2 = _toy(range(F), 1), _toy((1, 3), 2)               # stage 2 fails frames 1 and 3 again
    bits, iters, conv, stage, stats = spec.compose(s1, s2, llr, F)
    assert len(s2.calls) == 1 and np.array_equal(s2.calls[0], llr)                       # the channel LLRs, in frame order
    assert (stage == 2).all() and stats.tolist() == [5, 5, 2]
    assert conv.tolist() == [1, 0, 1, 0, 1] and iters.tolist() == [2, 20, 2, 20, 2]
    assert (bits[[0, 2, 4]] == 2).all() and np.array_equal(bits[[1, 3]], (llr[[1, 3]] > 0).astype(np.uint8))   # what stage 2 returns for a failed frame


def test_failures_above_capacity_keep_stage_one():
    F = 9
    llr = _llr(F)
    s1, s2 = _toy((1, 2, 5, 7, 8), 1), _toy((5,), 2)
    bits, iters, conv, stage, stats = spec.compose(s1, s2, llr, 3)
    assert np.array_equal(s2.calls[0], llr[[1, 2, 5]])                                   # the first three in frame order
    assert stage.tolist() == [1, 2, 2, 1, 1, 2, 1, 1, 1] and stats.tolist() == [5, 3, 1]
    assert conv.tolist() == [1, 1, 1, 1, 1, 0, 1, 0, 0] and iters.tolist() == [1, 2, 2, 1, 1, 20, 1, 10, 10]
    assert np.array_equal(bits[[7, 8]], (llr[[7, 8]] > 0).astype(np.uint8)) and (bits[[1, 2]] == 2).all() and (bits[[0, 3, 4, 6]] == 1).all()
    assert spec.select(conv, 1).tolist() == [5] and spec.select(np.ones(4), 2).tolist() == []
    # the input is not written
    assert np.array_equal(llr, _llr(F))


@functools.lru_cache(maxsize=None)
def _real():
    """codes/jpl.1024.4.5 H as CSR, fp16 cells, 20 sweeps, the first 256 all-zero frames at 3.0 dB of the stream
    tests/test_layered_aminstar_spec.py draws (seed 5) -> stage 1 alone, the cascade"""
    c = load("jpl.1024.4.5")
    llr = channel.frames(np.zeros((600, c.N), np.uint8), 3.0, 1024, 1280, 1408, seed=5).astype(np.float32)[:256]
    s1 = lambda x: rule.decode_float(c.graph, x, 20, 0.75, 0.0, "f16")   # noqa: E731
    s2 = lambda x: aminstar.decode_float(c.graph, x, 20, "f16")          # noqa: E731
    first = s1(llr)
    return first, spec.compose(lambda x: first, s2, llr, len(llr))


def test_three_quarter_min_sum_then_aminstar_on_the_ar4ja_code():
    """the figures this was written against: 53 of 256 frames fail stage 1, all 53 in error; the cascade leaves 14 frame errors"""
    (b1, i1, c1, _), (bits, iters, conv, stage, stats) = _real()
    F = len(b1)
    failed = ~c1.astype(bool)
    err1 = (b1[:, :1024] != 0).any(axis=1)
    err = (bits[:, :1024] != 0).any(axis=1)
    print("failed stage 1:", int(failed.sum()), "frame errors stage 1:", int(err1.sum()), "cascade:", int(err.sum()), "stats:", stats.tolist())
    assert 0.05 * F <= failed.sum() <= 0.60 * F                  # both branches of the cascade are exercised
    assert err1[failed].all()                                     # a frame stage 1 gives up on is in error in its message bits
    assert err.sum() < err1.sum()
    assert stats[0] == stats[1] == failed.sum() and stats[2] == (~conv.astype(bool)).sum()
    assert np.array_equal(stage == 2, failed) and np.array_equal(bits[~failed], b1[~failed]) and np.array_equal(iters[~failed], i1[~failed])
