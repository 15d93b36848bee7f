"""Small synthetic parity-check matrices built to reach, on purpose, the structural paths of the on-chip layered min-sum kernel for any H
(csrc/layered_csr.hip) that the named codes leave to chance: every row weight of each of the three row-weight classes (8, 20, 32), waves
whose lanes all hold heavy rows, uniform waves next to mixed ones, many barrier steps of mixed weights, steps of several slabs, a last
slab that leaves a whole wave idle, a step that merges declared layers, and rows without edges.  No GPU is needed here:
tests/test_layered_shapes.py asserts what the graphs are, tests/test_layered_csr_shapes_gpu.py decodes on them.

layered_graph(seed, N, layers) draws one matrix: for each (rows, weights) of `layers`, w = rng.choice(weights, rows), a fresh
rng.permutation(N), consecutive chunks of it to the rows, each sorted -- the rows of a drawn layer are column-disjoint by construction.
case(name) is a drawn matrix of CASES with two variations on top: one drawn layer DECLARED as two (the halves are disjoint, so the step
builder has to merge them) and, in "w8", three rows without edges, each a layer of its own.  The codeword is the all-zero word."""
import functools
import zlib

import numpy as np

from oracle import channel


def _r(a, b):
    return list(range(a, b + 1))


# name -> (N, [(rows, weights)]); the generator's seed is zlib.crc32(name)
CASES = {
    "w8": (2048, [(200, _r(2, 8))] * 4 + [(128, [3]), (200, _r(2, 8)), (128, [8]), (130, [6]), (1, [5]), (200, _r(2, 8))]),
    "w20": (4099, [(150, _r(9, 20)), (130, [12]), (70, [13]), (100, _r(2, 20)), (1, [20]), (150, _r(9, 20)), (200, _r(2, 20))]),
    "w27": (3000, [(100, _r(21, 27)), (64, [27]), (110, _r(2, 27)), (1, [24]), (100, _r(21, 27)), (130, [21]), (110, _r(2, 27))]),
}
DCLASS = {"w8": 8, "w20": 20, "w27": 32}
# the drawn layer that is declared as two halves; ("w8") the drawn layer that gets a row without edges in its middle
SPLIT_LAYER = {"w8": 0, "w20": 0, "w27": 0}
EMPTY_IN_LAYER = 4          # (128, [3]): its step becomes 128 rows of weight 3 and one of weight 0 -- at 256 threads a wave of idle lanes and an empty row


class Graph:
    """a CSR matrix with what the specifications, the frames and the library need"""

    def __init__(self, rp, ci, N, layer_ptr=None):
        self.row_ptr, self.col_idx, self.N = np.asarray(rp, np.int32), np.asarray(ci, np.int32), int(N)
        self.M = len(self.row_ptr) - 1
        self.k = self.N - self.M
        self.cw = np.zeros(self.N, np.uint8)
        self.layer_ptr = None if layer_ptr is None else np.asarray(layer_ptr, np.int32)

    @property
    def weights(self):
        return np.diff(self.row_ptr)

    def frames(self, F, db, seed):
        return channel.frames(np.tile(self.cw, (F, 1)), db, self.k, self.N, self.N, seed).astype(np.float32)

    def permuted(self, hip):
        """-> the matrix in the row order ldpc_csr_layer_order proposes, that order's layers declared"""
        perm, lp = hip.Code.csr_layer_order(self.row_ptr, self.col_idx, self.N, 0)
        prp, pci = hip.Code.permute_rows(self.row_ptr, self.col_idx, perm)
        return Graph(prp, pci, self.N, lp)

    def code(self, hip, layer_ptr=None):
        c = hip.Code.from_csr(self.row_ptr, self.col_idx, self.N)
        if layer_ptr is not None:
            c.set_layers(layer_ptr)
        return c


def layered_graph(seed, N, layers):
    rng = np.random.default_rng(seed)
    rows, lp = [], [0]
    for n, weights in layers:
        w = rng.choice(weights, n)
        perm = rng.permutation(N)
        assert int(w.sum()) <= N
        ends = np.cumsum(w)
        rows += [np.sort(perm[e - d:e]) for d, e in zip(w, ends)]
        lp.append(len(rows))
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return Graph(rp, np.concatenate(rows), N, lp)


def _with_empty_rows(g, at):
    """g with a row without edges put BEFORE each row index of `at` (M: after the last row), each such row a layer of its own"""
    rp, lp = g.row_ptr.tolist(), g.layer_ptr.tolist()
    for a in sorted(at, reverse=True):
        rp.insert(a, rp[a])
        lp = sorted(set([x for x in lp if x <= a] + [x + 1 for x in lp if x >= a] + [a, a + 1]))
    return Graph(rp, g.col_idx, g.N, lp)


@functools.lru_cache(maxsize=None)
def drawn(name):
    N, layers = CASES[name]
    return layered_graph(zlib.crc32(name.encode()), N, layers)


@functools.lru_cache(maxsize=None)
def case(name):
    """the drawn matrix with its variations; .layer_ptr are the DECLARED layers"""
    g = drawn(name)
    lp = g.layer_ptr.tolist()
    a, b = lp[SPLIT_LAYER[name]], lp[SPLIT_LAYER[name] + 1]
    g = Graph(g.row_ptr, g.col_idx, g.N, sorted(lp + [(a + b) // 2]))
    if name == "w8":
        mid = (lp[EMPTY_IN_LAYER] + lp[EMPTY_IN_LAYER + 1]) // 2
        g = _with_empty_rows(g, [0, mid, g.M])
    return g


def steps_of(g, layer_ptr):
    """the barrier steps of layered_csr_create, restated: a new step begins when a layer shares a column with the step being built.
    -> a list of row-index arrays"""
    steps, stamp = [], np.full(g.N, -1)
    for a, b in zip(layer_ptr[:-1], layer_ptr[1:]):
        cols = g.col_idx[g.row_ptr[a]:g.row_ptr[b]]
        if not steps or (stamp[cols] == len(steps) - 1).any():
            steps.append([])
        steps[-1] += range(a, b)
        stamp[cols] = len(steps) - 1
    return [np.asarray(s) for s in steps]


def default_threads(g, layer_ptr):
    """min(the instance's bound, the largest step rounded up to whole waves)"""
    rmax = max(len(s) for s in steps_of(g, layer_ptr))
    return min(512 if g.weights.max() > 20 else 1024, 64 * -(-rmax // 64))


def slabs(step, T):
    """a step of len(step) rows at T threads -> (number of slabs, rows of the last one)"""
    n = -(-len(step) // T)
    return n, len(step) - (n - 1) * T
