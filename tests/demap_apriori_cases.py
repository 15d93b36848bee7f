"""The inputs of tests/test_demap_apriori_gpu.py, built once and shared with tests/test_demap_apriori_spec.py: the table objects, levels and
shapes of tests/demap_logmap_cases.py with three a-priori sets on top.

Shapes         batch 3.  "ragged": N = 67, n_tx = 61 through that module's interleaver (6 punctured positions, a ragged last symbol for
               every m > 1), with its gains (a 0 and a NaN);  "aligned": N = n_tx = 120 with the identity, no gains (a NULL d_gain).
A-priori sets  "zero": all +0.  "normal": N(0, 4^2) in float32, a NaN at every punctured position (never read).  "genie": +-30 in
               agreement with the labels that were sent (the first draw of Case.samples, made again here), 0 at the punctured positions."""
import functools

import numpy as np

from tests import demap_apriori_spec as spec
from tests import demap_logmap_cases as cl
from tests import interleaver_spec as ils
from tests import modulation_spec as ms

B = cl.B
OBJECTS = [o for o in cl.OBJECTS if o[0] == "table"]
IDS = [n for _, n in OBJECTS]
LEVELS = cl.LEVELS
SHAPES = ("ragged", "aligned")
SETS = ("zero", "normal", "genie")
SEED = {"ragged": 3, "aligned": 2}


@functools.lru_cache(maxsize=None)
def positions(shape):
    pos = cl.interleaver() if shape == "ragged" else np.arange(cl.N_ALIGNED, dtype=np.int32)
    pos.setflags(write=False)
    return pos


def n_codeword(shape):
    return cl.N if shape == "ragged" else cl.N_ALIGNED


def sent_labels(c, n_sym, level, seed):
    """the labels Case.samples(n_sym, level, seed) drew: its generator's first call"""
    rng = np.random.default_rng([seed, c.m, LEVELS.index(level)])
    return rng.integers(0, len(c.pts), (B, n_sym))


@functools.lru_cache(maxsize=None)
def inputs(name, level, shape):
    """-> sym [B][n_sym][2], gains [B][n_sym] or None, pos, N, noise variance"""
    c = cl.case("table", name)
    pos, N = positions(shape), n_codeword(shape)
    ns = ms.symbols_per_frame(len(pos), c.m)
    sym = c.samples(ns, level, SEED[shape])
    a = cl.gains(ns, 31) if shape == "ragged" else None
    for x in (sym, a):
        if x is not None:
            x.setflags(write=False)
    return sym, a, pos, N, c.noise_var(level)


@functools.lru_cache(maxsize=None)
def apriori(name, level, shape, which):
    """La [B][N] float32, codeword order"""
    c = cl.case("table", name)
    pos, N = positions(shape), n_codeword(shape)
    holes = ils.holes(pos, N)
    if which == "zero":
        la = np.zeros((B, N), np.float32)
    elif which == "normal":
        la = np.random.default_rng([77, c.m, LEVELS.index(level), N]).normal(0.0, 4.0, (B, N)).astype(np.float32)
        la[:, holes] = np.nan
    else:
        ns = ms.symbols_per_frame(len(pos), c.m)
        lab = sent_labels(c, ns, level, SEED[shape])
        bits = ((lab[..., None] >> (c.m - 1 - np.arange(c.m))) & 1).reshape(B, ns * c.m)[:, :len(pos)]
        la = np.zeros((B, N), np.float32)
        la[:, pos] = np.where(bits, np.float32(30.0), np.float32(-30.0))
    la.setflags(write=False)
    return la


@functools.lru_cache(maxsize=None)
def reference(name, level, shape, which, rule):
    """the float32 restatement per symbol: (LLRs [B][n_sym][m], inv_s [B][n_sym], La [B][n_sym][m])"""
    c = cl.case("table", name)
    sym, a, pos, N, nv = inputs(name, level, shape)
    out = spec.per_symbol(c.pts, sym, a, pos, nv, apriori(name, level, shape, which), rule)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def brute(name, level, shape, which, rule):
    """the float64 brute force per symbol: (LLRs, T, A, the largest |u_p|)"""
    c = cl.case("table", name)
    sym, a, pos, N, nv = inputs(name, level, shape)
    _, inv_s, la = reference(name, level, shape, which, rule)
    out = spec.brute_force(c.pts, sym, inv_s, la, rule)
    for x in out:
        x.setflags(write=False)
    return out
