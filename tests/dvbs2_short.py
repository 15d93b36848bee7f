"""A parity-check matrix with the STRUCTURE of a DVB-S2 short frame (EN 302 307 section 5.3.2, n = 16 200), in natural order.

The construction rule of tests/dvbs2_natural.py at the short-frame size; the standard's address tables are not reproduced here, so
this is the rule on pseudo-random tables: the shape, the degrees and the irregularities of a real short-frame matrix, not its BER.
  * N = 16 200, K = 7 200, M = 9 000, q = 25, period 360: 20 column groups of 360 information bits, 8 groups of weight 8 and 12
    of weight 3;
  * information bit m of column group g goes to checks (x + m q) mod 9 000 for each address x of the group;
  * the 100 addresses' residues mod q are dealt so that every check gets the same number (4) of information edges;
  * at least three groups hold two addresses of equal residue: in the quasi-cyclic view (rows permuted by residue) their blocks
    carry TWO circulants;
  * the parity part is dual-diagonal WITHOUT wrap: check i sees parity bits i - 1 and i; check 0 sees parity bit 0 only.
A frame is 64 800 B as f32: it fits the LDS in either lam type.  Deterministic; built in memory (shared by
tests/test_layered_csr_f32_gpu.py and tools/layered_csr_rate.py)."""
from __future__ import annotations

import functools

import numpy as np

N, K, Q, PERIOD = 16200, 7200, 25, 360
M = N - K
GROUP_WEIGHTS = [8] * 8 + [3] * 12


def address_tables(seed=2025):
    """-> list of 20 int arrays: the addresses x (0 <= x < M) of each column group"""
    rng = np.random.default_rng(seed)
    res = np.repeat(np.arange(Q), sum(GROUP_WEIGHTS) // Q)       # every residue 4 times: 100 addresses
    while True:
        rng.shuffle(res)
        groups, i = [], 0
        for w in GROUP_WEIGHTS:
            groups.append(res[i:i + w].copy())
            i += w
        if sum(len(set(g.tolist())) < len(g) for g in groups) >= 3:
            break
    tables = []
    for r in groups:
        while True:
            x = r + Q * rng.integers(0, PERIOD, len(r))
            if len(set(x.tolist())) == len(x):
                break
        tables.append(np.sort(x).astype(np.int64))
    return tables


@functools.lru_cache(maxsize=None)
def csr(seed=2025):
    """-> (row_ptr [M + 1], col_idx [E]) int32, columns ascending inside a row; information bits are columns 0..K-1 (group g, bit m
    at g * 360 + m), parity bits K..N-1"""
    rows_c, cols_c = [], []
    m = np.arange(PERIOD)
    for g, xs in enumerate(address_tables(seed)):
        for x in xs:
            rows_c.append((x + m * Q) % M)
            cols_c.append(g * PERIOD + m)
    p = np.arange(M)
    rows_c += [p, p[1:]]                                           # check i: parity bit i, and parity bit i - 1 for i >= 1
    cols_c += [K + p, K + p[:-1]]
    r = np.concatenate(rows_c)
    c = np.concatenate(cols_c)
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    assert not np.any((np.diff(r) == 0) & (np.diff(c) == 0)), "duplicate edge"
    row_ptr = np.zeros(M + 1, np.int32)
    np.add.at(row_ptr, r + 1, 1)
    return np.cumsum(row_ptr).astype(np.int32), c.astype(np.int32)


def qc_blocks(seed=2025):
    """the information part in the quasi-cyclic view: check c -> block row c mod q, position c div q; -> dict
    (block row, column group) -> list of circulant rotations"""
    blocks = {}
    for g, xs in enumerate(address_tables(seed)):
        for x in xs:
            blocks.setdefault((int(x % Q), g), []).append(int(x // Q))
    return blocks
