"""The rule of the encoder from H (ldpc_csr_triangular_order, ldpc_sim_create_sparse_on; csrc/sim_sparse.hip), restated in numpy.

H is M x N as CSR, 0 < M < N, K = N - M: columns 0..K-1 carry the message, K..N-1 the parity bits; last(i) = the largest column of
row i.  H qualifies iff no row is empty, last(i) >= K for every row, and i -> last(i) - K is a bijection onto 0..M-1; then
order[j] = the row with last = K + j, and
    c[0..K) = msg;   for j = 0 .. M-1:  c[K + j] = XOR of c[col] over the OTHER columns of row order[j]   (all of them < K + j).
TEST INFRASTRUCTURE: nothing under ecc_ldpc_amd/ imports it, and it shares no code with the library."""
from __future__ import annotations

import numpy as np


class Refused(ValueError):
    """H does not qualify; .rows: the offending row, or the two rows that end in one column (.column)"""

    def __init__(self, msg, rows, column=None):
        super().__init__(msg)
        self.rows, self.column = tuple(rows), column


def triangular_order(row_ptr, col_idx, N):
    """-> order [M] int32; Refused when H does not qualify (the first offending row in storage order)"""
    rp, ci = np.asarray(row_ptr, np.int64), np.asarray(col_idx, np.int64)
    M = len(rp) - 1
    K = N - M
    if not 0 < M < N:
        raise Refused(f"M = {M}, N = {N}: no message columns", ())
    owner = {}
    for i in range(M):
        if rp[i + 1] == rp[i]:
            raise Refused(f"row {i} is empty", (i,))
        last = int(ci[rp[i]:rp[i + 1]].max())
        if last < K:
            raise Refused(f"row {i} ends in column {last} < K = {K}", (i,), last)
        if last in owner:
            raise Refused(f"rows {owner[last]} and {i} end in column {last}", (owner[last], i), last)
        owner[last] = i
    return np.array([owner[K + j] for j in range(M)], np.int32)


def encode(row_ptr, col_idx, N, order, msg):
    """msg [F][K] 0/1 -> codewords [F][N] uint8, by the rule above, all frames at once"""
    rp, ci = np.asarray(row_ptr, np.int64), np.asarray(col_idx, np.int64)
    msg = np.asarray(msg, np.uint8)
    M = len(rp) - 1
    K = N - M
    assert msg.ndim == 2 and msg.shape[1] == K
    c = np.zeros((msg.shape[0], N), np.uint8)
    c[:, :K] = msg
    for j, i in enumerate(np.asarray(order)):
        cols = ci[rp[i]:rp[i + 1]]
        others = cols[cols != K + j]
        assert len(others) == len(cols) - 1 and (others < K + j).all()
        c[:, K + j] = np.bitwise_xor.reduce(c[:, others], axis=1) if len(others) else 0
    return c


def syndrome(row_ptr, col_idx, codewords):
    """-> [F][M] uint8: H c over GF(2)"""
    rp, ci = np.asarray(row_ptr, np.int64), np.asarray(col_idx, np.int64)
    c = np.asarray(codewords, np.uint8)
    s = np.zeros((c.shape[0], len(rp) - 1), np.uint8)
    for i in range(len(rp) - 1):
        s[:, i] = np.bitwise_xor.reduce(c[:, ci[rp[i]:rp[i + 1]]], axis=1) if rp[i + 1] > rp[i] else 0
    return s


def _csr(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rp, (np.concatenate(rows) if len(rows) else np.zeros(0)).astype(np.int32)


def toy(M=70, K=45, seed=1):
    """-> (row_ptr, col_idx, N): a random H with a unit lower-triangular parity part, rows shuffled.  Row j (before the shuffle) ends
    in column K + j, holds up to two earlier parity bits at RANDOM distance (j - 1 among them for some rows, not for all), and
    one to six message bits -- except every seventh row, which holds none: row 0 is then the parity bit alone, a row of weight 1."""
    rng = np.random.default_rng(seed)
    rows = []
    for j in range(M):
        cols = {K + j}
        if j % 7:
            cols |= set(rng.choice(K, int(rng.integers(1, 7)), replace=False).tolist())
        for _ in range(int(rng.integers(0, 3)) if j else 0):
            cols.add(K + (j - 1 if rng.random() < 0.4 else int(rng.integers(0, j))))
        rows.append(np.sort(np.fromiter(cols, np.int64)))
    assert len(rows[0]) == 1
    rows = [rows[i] for i in rng.permutation(M)]
    rp, ci = _csr(rows)
    return rp, ci, K + M


def toy_decodable(M=70, K=45, seed=2):
    """the same shape with every row weight in 2..27 (what the on-chip layered decoder for any H takes) and every column in a row"""
    rng = np.random.default_rng(seed)
    rows = []
    for j in range(M):
        cols = {K + j, j % K} | set(rng.choice(K, int(rng.integers(1, 6)), replace=False).tolist())   # j % K: every message column is used
        for _ in range(int(rng.integers(0, 3))):
            if j:
                cols.add(K + int(rng.integers(0, j)))
        if j and j % 3:
            cols.add(K + j - 1)
        rows.append(np.sort(np.fromiter(cols, np.int64)))
    assert all(2 <= len(r) <= 27 for r in rows)
    rows = [rows[i] for i in rng.permutation(M)]
    rp, ci = _csr(rows)
    return rp, ci, K + M


def ring(row_ptr, col_idx, N):
    """the staircase closed into a ring: row 0 also sees column N - 1 (a DVB-S2-shaped H in natural order no longer qualifies)"""
    rp, ci = np.asarray(row_ptr, np.int64), np.asarray(col_idx, np.int64)
    assert ci[rp[1] - 1] != N - 1
    ci2 = np.concatenate([ci[:rp[1]], [N - 1], ci[rp[1]:]]).astype(np.int32)
    rp2 = rp.copy()
    rp2[1:] += 1
    return rp2.astype(np.int32), ci2
