"""The cases the soft-output tests share (tests/test_soft_output_spec.py on the CPU, tests/test_soft_output_gpu.py on the device): the three
graphs of tests/layered_shapes.py, the ten frames of tests/test_layered_i8_gpu._llr at the Eb/N0 pairs of tests/test_layered_csr_shapes_gpu.py,
its two rules (and (1/2, 0) where (1, 0.5) on "w8" int8 converges on nothing), and each reference computed once and never written."""
import functools

import numpy as np

from tests import layered_rule_spec as rule_spec
from tests import layered_shapes as S
from tests import soft_output_spec as spec
from tests.test_layered_i8_gpu import _llr

NAMES = list(S.CASES)
CELLS = ["f16", "f32", "i8"]
DBS = {"w8": (2.5, 5.0), "w20": (5.0, 7.0), "w27": (3.0, 5.0)}
PLAIN, RULED = (0.75, 0.0), (1.0, 0.5)
ALSO = {("w8", "i8"): (0.5, 0.0)}
SWEEPS = 25
QSCALE = 4.0


def rule_of(name, cell, ruled):
    """the rule a (case, cell, plain | ruled) is decoded with: the one that meets the condition of `exercised`"""
    return PLAIN if not ruled else ALSO.get((name, cell), RULED)


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def frames(name):
    return _frozen((_llr(S.case(name), DBS[name]),))[0]


@functools.lru_cache(maxsize=None)
def ref(name, cell, rule, max_iters):
    """bits, sweeps, converged, P, C of the ten frames"""
    return _frozen(spec.decode(cell, S.case(name), frames(name), max_iters, rule[0], rule[1], QSCALE))


@functools.lru_cache(maxsize=None)
def shipped(name, cell, rule, max_iters):
    """tests/layered_rule_spec.py decode of the same: bits, sweeps, converged, final_lam"""
    r = rule_spec.decode(cell, S.case(name), frames(name), max_iters, rule[0], rule[1], QSCALE)
    return _frozen((r[0], r[1], np.asarray(r[2], bool), np.asarray(r[3], np.float64)))


def inf_column(g):
    """the first column none of whose rows has fewer than three edges: an infinity there never meets one it sent out (no inf - inf)"""
    w = np.repeat(np.diff(g.row_ptr), np.diff(g.row_ptr))
    light, used = np.zeros(g.N, bool), np.zeros(g.N, bool)
    light[g.col_idx[w < 3]] = True
    used[g.col_idx] = True
    return int(np.flatnonzero(used & ~light)[0])


@functools.lru_cache(maxsize=None)
def nonfinite(name):
    """the ten frames with -inf in a noisy frame that converges after more than one sweep (f32 cells, the 3/4) and a NaN in the noiseless
    codeword -> llr, the frame with the infinity, its column, the specification's (bits, sweeps, converged, P, C) for f32 cells"""
    _, sweeps, conv, _, _ = ref(name, "f32", PLAIN, SWEEPS)
    f, col = int(np.flatnonzero(conv[:8] & (sweeps[:8] > 1))[0]), inf_column(S.case(name))
    llr = frames(name).copy()
    llr[f, col] = -np.inf
    llr[9, 5] = np.nan
    return _frozen((llr,))[0], f, col, _frozen(spec.decode("f32", S.case(name), llr, SWEEPS, PLAIN[0], PLAIN[1], QSCALE))


def exercised(sweeps, conv):
    """of the eight noisy frames one converges after more than one sweep and one runs out of sweeps"""
    sweeps, conv = sweeps[:8], np.asarray(conv, bool)[:8]
    return bool((conv & (sweeps > 1)).any() and (~conv).any())
