"""Specification of a continuing decode (ldpc_decode_state_*, ldpc_decode_batch_dev_continue; csrc/layered_csr.hip
layered_csr_cont_kernel<DCLASS, cell>): numpy, the three lam cell types, the 3/4 or a per-context check-node rule.  The device kernels
reproduce it bit for bit (tests/test_decode_continue_gpu.py).

The channel, the syndrome and the output formats are tests/soft_output_spec.py's channel, _syndrome_ok and output; the sweeps are those of
tests/layered_rule_spec.py -- its _rows, _apply, row_update_float and row_update_i8 -- all used as they are.

THE STATE of one frame slot
  msg [E]   the check-to-variable message on every edge (the device holds it as the row records {mag1, mag2, signs | arg-min})
  S [N]     what the checks have told column j so far: float32 for fp16 and f32 cells, an integer in -254 .. 254 for int8 cells
A reset slot has msg = 0 and S = 0.

ONE CALL takes channel LLRs llr' for `batch` frames; frame f uses slot first + f.
  1. C' = channel(cell, llr'): fp16 cells saturated and rounded with a NaN as +0, f32 cells the float, int8 cells the quantised integer.
  2. The starting lam:   f32 cells   lam0 = fl32(C' + S)
                         fp16 cells  lam0 = r16(fl32(float(C') + S))
                         int8 cells  lam0 = clip(C' + S, -127, 127)
  3. The stopping rule before the first sweep is the syndrome of hard(lam0), not of the channel's decisions: a frame that had converged in
     the previous call and gets compatible LLRs stops here with 0 sweeps.
  4. The sweeps of layered_rule_spec, up to max_iters; the first one subtracts the STORED messages.  The stop rule after a sweep, the f32
     non-finite veto (here on lam0 as well, as soft_output_spec has it on C) and the per-context rule are unchanged.
  5. bits, sweeps and flags follow soft_output_spec.decode with C' as "the channel": a frame out of sweeps or vetoed returns hard(C') and
     max_iters as its count.  The receiver's best guess is hard(P).
  6. P = lam as it stands when the frame stops (lam0 for a frame that stops before its first sweep); E = P - C'.
  7. The new state: S <- P - C' (ONE float32 subtraction, an integer one for int8 cells), for every frame however it stopped;
     msg <- the messages as the last sweep left them; a frame that ran no sweep keeps its msg.

CONSEQUENCES (tests/test_decode_continue_spec.py asserts the first; the others are stated, not tested for equality)
  * From a reset slot a call IS soft_output_spec.decode on the same LLRs: bits, sweeps, flags, P and E by bit pattern -- t = lam - (+0) is lam
    bit for bit.  The one exception is a channel LLR of -0.0, which enters as +0.0: x + (+0) is x for every x but -0.
  * A split decode is NOT an unsplit one: n1 sweeps and then n2 more on the same LLRs are not n1 + n2 sweeps in one call.
    fl(C + fl(P - C)) is not P in general, and the full syndrome before the first sweep of the second call can stop a frame that the
    "nothing moved" rule would have sent round once more.
  * f32 cells: a slot whose frame diverged holds an S that is not finite and stays failed until it is reset.  fp16 and int8 cells cannot
    get there: the cell saturates.
What is NOT specified is what soft_output_spec leaves open: a NaN that a sweep takes in."""
import numpy as np

from oracle import emulate_f16 as em
from tests import layered_rule_spec as rule
from tests import soft_output_spec as soft
from tests.layered_i8_spec import QMAX


class State:
    """msg [frames, E], S [frames, N] of `frames` slots, all reset"""

    def __init__(self, cell, graph, frames):
        _, E = rule._rows(graph)
        t = np.int32 if cell == "i8" else np.float32
        self.cell, self.msg, self.S = cell, np.zeros((frames, E), t), np.zeros((frames, graph.N), t)

    def copy(self):
        s = State.__new__(State)
        s.cell, s.msg, s.S = self.cell, self.msg.copy(), self.S.copy()
        return s

    def reset(self, first=0, count=None):
        last = len(self.S) if count is None else first + count
        self.msg[first:last] = 0
        self.S[first:last] = 0


def start(cell, C, S):
    """lam0 of step 2"""
    if cell == "i8":
        return np.clip(C + S, -QMAX, QMAX).astype(np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (C + S).astype(np.float32)
    return em.r16(v) if cell == "f16" else v


def call(cell, graph, state, llr, max_iters, alpha=0.75, beta=0.0, qscale=4.0, first=0):
    """llr [F, N] on slots first .. first + F - 1 of `state`, which is not written -> (bits [F, N] u8, sweeps [F] i32, converged [F] bool,
    P [F, N], C' [F, N]), the new state"""
    rows, E = rule._rows(graph)
    C = soft.channel(cell, llr, qscale)
    F = C.shape[0]
    assert 0 <= first and first + F <= len(state.S) and state.cell == cell
    new = state.copy()
    sl = slice(first, first + F)
    if cell == "i8":
        update, args = rule.row_update_i8, rule.int_params(alpha, beta, qscale)
    else:
        update, args = rule.row_update_float, (alpha, beta, {"f16": em.r16, "f32": rule.f32_cast}[cell])
    lam0 = start(cell, C, state.S[sl])
    ok = soft._syndrome_ok(rows, lam0)
    P = lam0.copy()
    conv = ok.copy()
    iters = np.zeros(F, np.int32)
    if cell == "f32":
        conv &= np.isfinite(lam0).all(axis=1)
        iters[ok & ~conv] = max_iters
    live = np.flatnonzero(~ok)
    lam = lam0[live].copy()
    msg = state.msg[sl][live].copy()
    for n in range(1, max_iters + 1):
        if not len(live):
            break
        moved = np.zeros(len(live), bool)
        for cols, e0 in rows:
            moved |= rule._apply(update, lam, msg, cols, e0, *args)
        P[live] = lam
        new.msg[first + live] = msg                     # the messages as the last sweep left them
        fin = ~moved
        fin_ok = fin & np.isfinite(lam).all(axis=1) if cell == "f32" else fin
        conv[live[fin_ok]] = True
        iters[live[fin_ok]] = n
        iters[live[fin & ~fin_ok]] = max_iters
        live, lam, msg = live[moved], lam[moved], msg[moved]
    iters[live] = max_iters
    bits = (np.where(conv[:, None], P, C) > 0).astype(np.uint8)
    new.S[sl] = soft.value(cell, P, C, "extrinsic")
    return (bits, iters, conv, P, C), new
