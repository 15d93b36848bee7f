"""Phase B's stores of the headline kernel -- fused_split_kernel<float, min-sum, PlanAR4JA45, 128, TabJpl4096> -- where the kernel may
address them by lane id (csrc/fused_split_body.h SPLIT_STORE_ADDTID: ds_write_addtid_b32, address = M0 + immediate + 4 * lane, for
the edges a wave cannot wrap), and the paths that read lam right behind phase B.  Everything is held EQUAL, bit for bit, to
flood_qc_kernel on the same context (path "flood": state in HBM, one thread per row and per column, the same float arithmetic in the
same order, no LDS): trace rows, final lam, hard bits, iteration counts and flags.  The test holds whichever store form the build ships.

What a misplaced or late store would show in:
  - random frames (5 at 2 dB, 5 at 3 dB) make every cell of lam a different float, so a value stored to another cell, or read by the
    next round before it has landed, changes a trace row: turn 1 shows round 0's stores (lam = message + channel LLR), turns 2 and 3
    the read-add-write rounds; max_iters 1, 2 and 7 end the loop right behind a phase B;
  - a frame that converges early: its snapshot (hard bits) and its final lam are read from LDS behind the last phase B;
  - a frame with infinite channel LLRs whose hard decisions become a codeword: the non-finite veto reads lam behind phase B
    (the poison is tests/test_nonfinite_llr_gpu.py's "inf_right");
  - a teacher-forced step from a GIVEN lam and given messages: one phase B on a state that is not the kernel's own;
  - a batch of 1 and a batch of 61.
"""
import functools

import numpy as np
import pytest

from tests.helpers import load
from tests.test_nonfinite_llr_gpu import Case

pytestmark = pytest.mark.gpu

NAME = "jpl.4096.4.5"


@functools.lru_cache(maxsize=None)
def _frames():
    """-> (codewords [10, N], LLRs [10, N] float64 holding float32 values): 5 frames at 2 dB, then 5 at 3 dB"""
    c = load(NAME)
    lo, hi = c.frames(5, 2.0, 9101), c.frames(5, 3.0, 9102)
    llr = np.concatenate([lo[1], hi[1]]).astype(np.float32).astype(np.float64)
    llr.setflags(write=False)
    return np.concatenate([lo[0], hi[0]]), llr


@functools.lru_cache(maxsize=None)
def _decoders(hip, batch):
    code = load(NAME).hip_code(hip)
    s, fl = hip.Decoder(code, "min", "f32", batch, path="fused"), hip.Decoder(code, "min", "f32", batch, path="flood")
    assert "fused_split_kernel" in s.kernel_name and load(NAME).sz == 128, s.kernel_name
    assert "flood" in fl.kernel_name, fl.kernel_name
    return s, fl


def _equal(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y, equal_nan=True), (what, i, int((np.asarray(x) != np.asarray(y)).sum()))


def test_edge_placement_trace_and_final_lam_equal_the_flood_kernel(hip):
    _, llr = _frames()
    s, fl = _decoders(hip, len(llr))
    ta, tb = s.decode_trace(llr, 3), fl.decode_trace(llr, 3)
    lam = tb[3]
    # the premise: every frame ran its three turns, and within a turn's row the floats differ from cell to cell and from turn to turn
    assert (tb[1] == 3).all() and not tb[2].any()
    # (turn 1 moves the punctured columns alone -- every check holds one, at lam = 0, so the other columns' first messages are zero --
    #  but round 0 rewrites every cell with message + channel LLR, and the channel LLRs differ from cell to cell)
    c = load(NAME)
    for n in (1, 2, 3):
        changed = (lam[:, n] != lam[:, n - 1]).mean()
        assert changed == (c.N - c.n_tx) / c.N if n == 1 else changed > 0.99, (n, changed)
        assert min(len(np.unique(lam[f, n])) for f in range(len(llr))) > 3000
    for n in (0, 1, 2, 3):
        assert np.array_equal(ta[3][:, n], lam[:, n]), (n, int((ta[3][:, n] != lam[:, n]).sum()))
    _equal(ta, tb, "trace")
    for turns in (1, 2, 7):
        a, b = s.decode_batch(llr, turns, want_lam=True), fl.decode_batch(llr, turns, want_lam=True)
        print(f"max_iters {turns}: iters {b[1].tolist()} converged {b[2].tolist()}")
        _equal(a, b, turns)


def test_early_convergence_snapshot_and_final_lam(hip):
    _, llr = _frames()
    s, fl = _decoders(hip, len(llr))
    a, b = s.decode_batch(llr, 50, want_lam=True), fl.decode_batch(llr, 50, want_lam=True)
    print(f"iters {b[1].tolist()} converged {b[2].tolist()}")
    early = b[2].astype(bool) & (b[1] >= 2) & (b[1] < 50)
    assert early.sum() >= 3 and not b[2].all()          # frames stopped behind a phase B, next to frames that ran out of turns
    _equal(a, b, "50 turns")


def test_veto_path_reads_lam_behind_phase_b(hip):
    cws, llr = _frames()
    s, fl = _decoders(hip, len(llr))
    x = llr.copy()
    for f in (5, 9):     # 3 dB frames: +inf on three columns whose sign is right
        x[f] = Case.poison(None, "inf_right", cws[f], llr[f])
        assert np.isinf(x[f]).sum() == 3
    with np.errstate(all="ignore"):
        a, b = s.decode_batch(x, 50, want_lam=True), fl.decode_batch(x, 50, want_lam=True)
    print(f"iters {b[1].tolist()} converged {b[2].tolist()}")
    assert not b[2][[5, 9]].any() and (b[1][[5, 9]] == 50).all()     # vetoed: failed, never "converged"
    assert np.array_equal(b[0][[5, 9]], (x[[5, 9]] > 0).astype(np.uint8))
    _equal(a, b, "poisoned batch")
    clean = fl.decode_batch(llr, 50, want_lam=True)
    keep = [f for f in range(len(llr)) if f not in (5, 9)]
    _equal([v[keep] for v in a], [v[keep] for v in clean], "the frames around the poisoned ones")


def test_teacher_forced_step_from_a_given_lam(hip):
    c = load(NAME)
    _, llr = _frames()
    rng = np.random.default_rng(9103)
    lam = rng.normal(0.0, 6.0, llr.shape).astype(np.float32).astype(np.float64)
    ne = rng.normal(0.0, 3.0, (len(llr), c.E)).astype(np.float32).astype(np.float64)
    s, fl = _decoders(hip, len(llr))
    a, b = s.debug_step(llr, lam, ne), fl.debug_step(llr, lam, ne)
    assert (b[1] != lam).mean() > 0.9 and (b[0] != ne).mean() > 0.9
    _equal(a, b, "step")


@pytest.mark.parametrize("batch", [1, 61])
def test_batch_sizes(hip, batch):
    _, llr = _frames()
    x = np.concatenate([llr] * 7)[:batch]
    s, fl = _decoders(hip, batch)
    _equal(s.decode_batch(x, 7, want_lam=True), fl.decode_batch(x, 7, want_lam=True), batch)
    _equal(s.decode_trace(x, 2), fl.decode_trace(x, 2), (batch, "trace"))
