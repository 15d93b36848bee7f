"""The inputs of tests/test_demap_logmap_gpu.py, built once and shared with tests/test_demap_logmap_spec.py, which checks on the CPU that
the float32 restatement of the rule stays inside the GPU bar on every one of them.

Objects        table objects m = 1..6 (the built-ins, a 32-point APSK, an 8 x 8 grid with natural labels) and one irregular 8-point
               table; product objects b = 1..6 with unequal, non-uniform I / Q level sets and shuffled labels.
Levels         three noise variances per object: "low" (per-symbol SNR Es / (2 sigma^2) = 0 dB: the corrections are large), "mid"
               (3 m dB) and "collapse" (sigma^2 = dmin^2 / 4000, dmin the smallest distance between two points: nearly every other term
               underflows).  The samples are points plus noise of that variance; at "collapse" the noise is drawn at (0.2 dmin)^2
               instead, so that a sample does not sit on its point, where two points of the other subset may tie.
Shapes         batch 3; N = 67, n_tx = 61 (a ragged last symbol for every m > 1, a zero tail, element stores); N = n_tx = 120 (every m
               divides it: the vector stores); an interleaver of 61 entries into 67 positions (6 punctured); gains with a 0 and a NaN;
               a rate-matching table into 67 positions with fan-in 0 (5 positions), 1, 2 and 3, E = 118 > N."""
import functools

import numpy as np

from tests import demap_logmap_spec as ls
from tests import modulation_spec as ms
from tests import product_modulation_spec as ps
from tests.test_modulation_gpu import TABLES
from tests.test_product_modulation_gpu import _uneven

B, N, N_TX, N_ALIGNED = 3, 67, 61, 120
LEVELS = ("low", "mid", "collapse")


def irregular8():
    """eight points in no pattern, unit energy"""
    pts = np.random.default_rng(808).uniform(-1.0, 1.0, (8, 2))
    return (pts / np.sqrt((pts ** 2).sum() / 8.0)).astype(np.float32)


OBJECTS = [("table", "bpsk"), ("table", "qpsk"), ("table", "8psk"), ("table", "16qam"), ("table", "apsk32"), ("table", "grid64"), ("table", "irregular8")] \
    + [("product", b) for b in range(1, 7)]
IDS = [f"{k}-{n}" for k, n in OBJECTS]


class Case:
    """one object: its tables, and the spec's functions bound to them"""

    def __init__(self, kind, n):
        self.kind, self.n = kind, n
        if kind == "table":
            self.pts = irregular8() if n == "irregular8" else TABLES[n]()
            self.m = ms.bits_per_symbol(self.pts)
            self.single = self.m == 1
            p64 = self.pts.astype(np.float64)
            d = ((p64[:, None] - p64[None]) ** 2).sum(-1)
            d[np.arange(len(p64)), np.arange(len(p64))] = np.inf
            self.dmin = float(np.sqrt(d.min()))
            self.es = ms.energy(self.pts)
            self._f = {"llrs": ls.llrs, "llrs32": ls.llrs32, "collapsed": ls.collapsed, "maxlog": ls.maxlog}
            self._args = (self.pts,)
        else:
            self.li, self.lq = _uneven(n, 160 + n), (_uneven(n, 170 + n) * np.float32(0.6)).astype(np.float32)
            self.pts = None
            self.m = 2 * n
            self.single = n == 1
            self.dmin = float(min(np.diff(np.sort(self.li.astype(np.float64))).min(), np.diff(np.sort(self.lq.astype(np.float64))).min()))
            self.es = float((self.li.astype(np.float64) ** 2).mean() + (self.lq.astype(np.float64) ** 2).mean())
            self._f = {"llrs": ls.llrs_product, "llrs32": ls.llrs32_product, "collapsed": ls.collapsed_product, "maxlog": ls.maxlog_product}
            self._args = (self.li, self.lq)

    def make(self, hip):
        return hip.Modulation(self.pts) if self.kind == "table" else hip.Modulation.product(self.li, self.lq)

    def spec(self, what, sym, nv, a=None):
        return self._f[what](*self._args, sym, nv, a)

    def noise_var(self, level):
        if level == "low":
            return self.es / 2.0
        if level == "mid":
            return self.es / 2.0 / 10.0 ** (0.3 * self.m)
        return self.dmin ** 2 / 4000.0

    def samples(self, n_sym, level, seed):
        """[B][n_sym][2] float32"""
        rng = np.random.default_rng([seed, self.m, LEVELS.index(level)])
        sd = 0.2 * self.dmin if level == "collapse" else np.sqrt(self.noise_var(level))
        if self.kind == "table":
            c = self.pts[rng.integers(0, len(self.pts), (B, n_sym))].astype(np.float64)
        else:
            c = np.stack([self.li[rng.integers(0, len(self.li), (B, n_sym))], self.lq[rng.integers(0, len(self.lq), (B, n_sym))]], axis=-1).astype(np.float64)
        return (c + rng.normal(0.0, sd, (B, n_sym, 2))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(kind, n):
    return Case(kind, n)


def gains(n_sym, seed):
    """[B][n_sym] float32 in 0.3 .. 3, with one 0 (an erasure) and one NaN"""
    a = np.random.default_rng(seed).uniform(0.3, 3.0, (B, n_sym)).astype(np.float32)
    a[0, 1], a[B - 1, n_sym - 2] = 0.0, np.nan
    return a


@functools.lru_cache(maxsize=None)
def interleaver():
    """pos [61] into 67 positions: 6 punctured"""
    return np.ascontiguousarray(np.random.default_rng(6761).permutation(N)[:N_TX], np.int32)


@functools.lru_cache(maxsize=None)
def rm_table():
    """pos [E] into 67 positions: 5 left out, the others named once, twice or three times, in shuffled order"""
    rng = np.random.default_rng(6711)
    fan = rng.integers(1, 4, N)
    fan[rng.permutation(N)[:5]] = 0
    pos = np.ascontiguousarray(rng.permutation(np.repeat(np.arange(N), fan)), np.int32)
    assert len(pos) > N and sorted(set(fan.tolist())) == [0, 1, 2, 3]
    return pos


def inputs(c, level):
    """every per-symbol input of the GPU test for object c at one level: {name: (sym, gains or None)}"""
    ns, na, nr = ms.symbols_per_frame(N_TX, c.m), ms.symbols_per_frame(N_ALIGNED, c.m), ms.symbols_per_frame(len(rm_table()), c.m)
    return {"ragged": (c.samples(ns, level, 1), None), "aligned": (c.samples(na, level, 2), None), "csi": (c.samples(ns, level, 3), gains(ns, 31)),
            "rm": (c.samples(nr, level, 4), None), "rm-gains": (c.samples(nr, level, 5), gains(nr, 51)), "rm-round2": (c.samples(nr, level, 6), gains(nr, 61))}


def per_position(per_bit, pos, n_pos):
    """per_bit [B][E] -> ([B][n_pos]: the sum of the values of the bits that name each position, fan-in [n_pos])"""
    out = np.zeros((per_bit.shape[0], n_pos), per_bit.dtype)
    for t, p in enumerate(pos):
        out[:, p] += per_bit[:, t]
    return out, np.bincount(pos, minlength=n_pos)
