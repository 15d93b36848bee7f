"""(CPU) tests/layered_shapes.py: the synthetic matrices of tests/test_layered_csr_shapes_gpu.py ARE what that module needs them to be --
the preconditions of its GPU tests, asserted where no GPU is needed."""
import zlib

import numpy as np
import pytest

from tests import layered_shapes as S

NAMES = list(S.CASES)
# what the draws gave (numpy's default_rng from zlib.crc32 of the name): rows, edges, barrier steps of the drawn layers
DRAWN = {"w8": (1587, 8316, 10), "w20": (801, 10123, 7), "w27": (615, 12430, 7)}
# the declared layers of case(): threads per workgroup by default, and the rows of the largest step.  The split changes no step (its halves
# merge again); the three rows without edges of "w8" join the steps around them: the largest grows from 200 rows to 201, still four waves
THREADS = {"w8": (256, 201), "w20": (256, 200), "w27": (192, 130)}


@pytest.mark.parametrize("name", NAMES)
def test_drawn_graph(name):
    g = S.drawn(name)
    N, layers = S.CASES[name]
    assert (g.M, len(g.col_idx), len(S.steps_of(g, g.layer_ptr))) == DRAWN[name]
    assert g.N == N and g.k == N - g.M and not g.cw.any() and len(g.layer_ptr) == len(layers) + 1
    assert g.col_idx.min() >= 0 and g.col_idx.max() < N
    for (rows, weights), a, b in zip(layers, g.layer_ptr[:-1], g.layer_ptr[1:]):
        assert b - a == rows and set(g.weights[a:b].tolist()) <= set(weights)
        assert all((np.diff(g.col_idx[g.row_ptr[m]:g.row_ptr[m + 1]]) > 0).all() for m in range(a, b))       # each row sorted
    # every declared layer except the single rows clashes with its neighbour: as many steps as drawn layers
    assert len(S.steps_of(g, g.layer_ptr)) == len(layers)
    again = S.layered_graph(zlib.crc32(name.encode()), N, layers)                    # the seed alone decides the draw
    assert np.array_equal(again.row_ptr, g.row_ptr) and np.array_equal(again.col_idx, g.col_idx)


@pytest.mark.parametrize("name", NAMES)
def test_declared_layers_are_column_disjoint(name):
    g = S.case(name)
    lp = g.layer_ptr
    assert lp[0] == 0 and lp[-1] == g.M and (np.diff(lp) > 0).all()
    for a, b in zip(lp[:-1], lp[1:]):
        cols = g.col_idx[g.row_ptr[a]:g.row_ptr[b]]
        assert len(np.unique(cols)) == len(cols), (name, a, b)


@pytest.mark.parametrize("name", NAMES)
def test_weights(name):
    g = S.case(name)
    count = np.bincount(g.weights, minlength=28)
    lo, hi = {"w8": (2, 8), "w20": (9, 20), "w27": (21, 27)}[name]
    assert (count[lo:hi + 1] >= 2).all(), count                 # every weight of the class, each in at least two rows
    assert g.weights.max() == hi and S.DCLASS[name] == (8 if hi <= 8 else 20 if hi <= 20 else 32)
    assert count[1] == 0                                        # (min-sum refuses weight 1)
    if name == "w27":
        assert (count[2:28] > 0).all()                          # all 26 weights
    if name == "w20":
        assert (count[2:21] > 0).all()
    # rows without edges: "w8" alone -- the first row, the last row and one inside the drawn layer of 128 rows of weight 3
    empty = np.flatnonzero(g.weights == 0)
    if name == "w8":
        assert len(empty) == 3 and empty[0] == 0 and empty[2] == g.M - 1
        m = int(empty[1])
        assert (g.weights[m - 64:m] == 3).all() and (g.weights[m + 1:m + 65] == 3).all()
        for e in empty:                                         # each a layer of its own
            assert e in g.layer_ptr and e + 1 in g.layer_ptr
        d = S.drawn(name)                                       # and nothing else changed
        assert np.array_equal(g.col_idx, d.col_idx) and np.array_equal(g.weights[g.weights > 0], d.weights)
    else:
        assert len(empty) == 0 and np.array_equal(g.row_ptr, S.drawn(name).row_ptr)


@pytest.mark.parametrize("name", NAMES)
def test_steps(name):
    g = S.case(name)
    lp = g.layer_ptr
    steps = S.steps_of(g, lp)
    assert np.array_equal(np.concatenate(steps), np.arange(g.M))
    for s in steps:                                             # a step's rows are column-disjoint (what makes it a step)
        cols = np.concatenate([g.col_idx[g.row_ptr[m]:g.row_ptr[m + 1]] for m in s])
        assert len(np.unique(cols)) == len(cols)
    # the variations change no step count, and some step spans two or more declared layers
    assert len(steps) == DRAWN[name][2]
    spans = [int(np.sum((lp[:-1] >= s[0]) & (lp[:-1] <= s[-1]))) for s in steps]
    assert max(spans) >= 2, spans
    assert sum(spans) == len(lp) - 1
    # the default thread count
    assert (S.default_threads(g, lp), max(len(s) for s in steps)) == THREADS[name]
    # 128 threads: some step's last slab has at most 64 rows -- its second wave is idle
    assert any(S.slabs(s, 128)[1] <= 64 for s in steps if len(s) > 1)
    # 64 threads: at least five steps span several slabs
    assert sum(S.slabs(s, 64)[0] > 1 for s in steps) >= 5
    # one row per layer (no set_layers): other step boundaries
    own = S.steps_of(g, np.arange(g.M + 1))
    assert [int(s[0]) for s in own] != [int(s[0]) for s in steps]
    # waves whose lanes all hold heavy rows, at the default thread count (a step's rows are sorted heaviest first)
    if name == "w27":
        T = THREADS[name][0]
        assert any((np.sort(g.weights[s])[::-1][:64] > 20).all() and len(s) >= 64 for s in steps)
        assert any(len(set(np.sort(g.weights[s])[::-1][64 * w:64 * w + 64].tolist())) > 1 for s in steps for w in range(min(T, len(s)) // 64))
