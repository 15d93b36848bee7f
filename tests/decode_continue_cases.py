"""The cases the continuing-decode tests share (tests/test_decode_continue_spec.py on the CPU, tests/test_decode_continue_gpu.py on the
device): the graphs, frames, cells and rules of tests/soft_output_cases.py, and THE CHAIN of three calls on one state of ten slots --
  call 1   the ten frames, 2 sweeps, from reset
  call 2   llr' = float32(1.25) * llr, 25 sweeps, from call 1's state
  call 3   llr'' = llr, 25 sweeps, from call 2's state
each reference computed once and never written."""
import functools

import numpy as np

from tests import decode_continue_spec as cspec
from tests import layered_shapes as S
from tests import soft_output_cases as K
from tests import soft_output_spec as sspec

FIRST_SWEEPS = 2
GAIN = np.float32(1.25)


@functools.lru_cache(maxsize=None)
def chain_llrs(name):
    """the LLRs and sweep limits of the three calls"""
    llr = K.frames(name)
    scaled = (GAIN * llr).astype(np.float32)
    scaled.setflags(write=False)
    return ((llr, FIRST_SWEEPS), (scaled, K.SWEEPS), (llr, K.SWEEPS))


def run_chain(name, cell, rule, calls, state=None, first=0):
    """-> [(bits, sweeps, converged, P, C') per call], [the state after each call]"""
    g = S.case(name)
    st = cspec.State(cell, g, len(calls[0][0])) if state is None else state
    res, states = [], []
    for llr, mi in calls:
        r, st = cspec.call(cell, g, st, llr, mi, rule[0], rule[1], K.QSCALE, first)
        res.append(r)
        states.append(st)
    return res, states


@functools.lru_cache(maxsize=None)
def chain(name, cell, rule):
    res, states = run_chain(name, cell, rule, chain_llrs(name))
    for r in res:
        K._frozen(r)
    for s in states:
        K._frozen((s.msg, s.S))
    return res, states


@functools.lru_cache(maxsize=None)
def restarted(name, cell, rule):
    """soft_output_spec.decode of call 2's LLRs: what a decoder that forgets gives"""
    return K._frozen(sspec.decode(cell, S.case(name), chain_llrs(name)[1][0], K.SWEEPS, rule[0], rule[1], K.QSCALE))


def bits_of(a):
    """the bit patterns of an array, for comparison with np.array_equal"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])
