"""The rule of the encoder from ANY parity-check matrix (ldpc_csr_systematic_form, ldpc_sim_create_systematic_on;
csrc/systematic.cc, csrc/sim_systematic.hip), restated in numpy.

H is M x N over GF(2); rows may be redundant or empty.  Visit the columns from N - 1 down to 0:
    column c is a PARITY position iff it is not in the span of the parity positions already chosen (all of them > c).
par_pos[0..r) are the parity positions in ascending order, r = rank H; every other column is a MESSAGE position, msg_pos[0..K)
ascending, K = N - r.  The codeword of a message m has c[msg_pos[i]] = m[i] and c[par_pos[.]] the unique solution of H c = 0
(unique: H restricted to the parity positions has full column rank), i.e. c[par_pos[j]] = XOR_i m[i] P[i][j], P a K x r bit matrix.
TEST INFRASTRUCTURE: nothing under ecc_ldpc_amd/ imports it, and it shares no code with the library."""
from __future__ import annotations

import functools

import numpy as np


def systematic_form(H):
    """H [M][N] 0/1 -> (msg_pos [K], par_pos [r], P [K][r] uint8).  With the columns reversed the parity positions are the pivot
    columns of the reduced row echelon form (a column gets a pivot iff it is independent of the columns before it), and the pivot
    row of parity position p reads c[p] = XOR of c[n] over its other columns n -- all of them message positions."""
    H = np.asarray(H, np.uint8)
    M, N = H.shape
    A = np.packbits(H[:, ::-1], axis=1)                               # bit q of a row = column N - 1 - q
    piv, r = [], 0
    for q in range(N):
        if r == M:
            break
        byte, sh = q >> 3, 7 - (q & 7)
        below = np.flatnonzero((A[r:, byte] >> sh) & 1)
        if not len(below):
            continue
        p = r + int(below[0])
        if p != r:
            A[[r, p]] = A[[p, r]]
        rows = np.flatnonzero((A[:, byte] >> sh) & 1)
        A[rows[rows != r]] ^= A[r]
        piv.append(q)
        r += 1
    R = np.unpackbits(A[:r], axis=1)[:, :N][:, ::-1][::-1]            # H's column order; row j = the pivot row of par_pos[j]
    par_pos = np.array([N - 1 - q for q in piv[::-1]], np.int32)
    msg_pos = np.setdiff1d(np.arange(N, dtype=np.int32), par_pos).astype(np.int32)
    assert (R[np.arange(r), par_pos] == 1).all() and R[:, par_pos].sum() == r
    return msg_pos, par_pos, np.ascontiguousarray(R[:, msg_pos].T)


def encode(N, msg_pos, par_pos, P, msg):
    """msg [F][K] 0/1 -> codewords [F][N] uint8"""
    msg = np.asarray(msg, np.uint8)
    assert msg.ndim == 2 and msg.shape[1] == len(msg_pos)
    c = np.zeros((msg.shape[0], N), np.uint8)
    c[:, msg_pos] = msg
    c[:, par_pos] = (msg.astype(np.int64) @ P.astype(np.int64)) & 1
    return c


def syndrome(H, codewords):
    """-> [F][M] uint8: H c over GF(2)"""
    return ((np.asarray(codewords, np.int64) @ np.asarray(H, np.int64).T) & 1).astype(np.uint8)


def csr(H):
    H = np.asarray(H, np.uint8)
    rp = np.zeros(H.shape[0] + 1, np.int32)
    rp[1:] = np.cumsum(H.sum(1))
    return rp, np.nonzero(H)[1].astype(np.int32)


def random_matrix(M, N, seed, density=0.3, dup_rows=0, empty_rows=0, zero_cols=0, equal_cols=0, dependent_tail=False):
    """a random M x N matrix with the named defects put in at random places (dependent_tail: the last column is the sum of the two
    before it, so the last r columns cannot all be parity positions)"""
    rng = np.random.default_rng(seed)
    H = (rng.random((M, N)) < density).astype(np.uint8)
    for _ in range(dup_rows):
        a, b = rng.choice(M, 2, replace=False)
        H[a] = H[b]
    for _ in range(empty_rows):
        H[rng.integers(0, M)] = 0
    if dependent_tail:
        H[:, N - 1] = H[:, N - 2] ^ H[:, N - 3]
    for _ in range(equal_cols):
        a, b = rng.choice(N - 3, 2, replace=False)
        H[:, a] = H[:, b]
    for _ in range(zero_cols):
        H[:, rng.integers(0, N - 3)] = 0
    return H


@functools.lru_cache(maxsize=None)
def cases():
    """name -> H, from 3 x 5 to 40 x 90: every defect alone at least once, and several at once"""
    out = {
        "3x5": random_matrix(3, 5, 1, 0.5),
        "4x9-dup-rows": random_matrix(4, 9, 2, 0.4, dup_rows=1),
        "6x11-empty-row": random_matrix(6, 11, 3, 0.4, empty_rows=1),
        "7x13-zero-col": random_matrix(7, 13, 4, 0.4, zero_cols=1),
        "8x17-equal-cols": random_matrix(8, 17, 5, 0.4, equal_cols=1),
        "9x20-dependent-tail": random_matrix(9, 20, 6, 0.4, dependent_tail=True),
        "12x12-square": random_matrix(12, 12, 7, 0.3, dup_rows=2),
        "20x33-tall-rank": random_matrix(20, 33, 8, 0.2, dup_rows=3, empty_rows=1, zero_cols=1),
        "30x64-all": random_matrix(30, 64, 9, 0.15, dup_rows=4, empty_rows=2, zero_cols=2, equal_cols=2, dependent_tail=True),
        "50x21-more-rows-than-cols": random_matrix(50, 21, 10, 0.3, dup_rows=30, zero_cols=1),
        "40x90": toy_40x90(),
    }
    for H in out.values():
        H.setflags(write=False)
    return out


def toy_40x90():
    """40 x 90 (N no multiple of 4 or 32) with duplicated rows, a zero column and dependent tail columns"""
    return random_matrix(40, 90, 11, 0.12, dup_rows=5, zero_cols=1, dependent_tail=True)
