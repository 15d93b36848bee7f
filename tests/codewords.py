"""Real codewords for the decoder tests (TEST INFRASTRUCTURE, numpy only): random words c with H c = 0 for any parity-check matrix the
suite knows, the channel frames of such words, and the negation that maps the frame of a codeword onto the frame of the all-zero word.

Why: with the all-zero word and hard(x) = x > 0 a converged frame's output is all zeros -- right for any bit written to the wrong place,
any bit order of a packed result and any stop rule that reads the wrong columns -- and almost every lam - ne is negative, so the sign
and parity code of a kernel runs on one half of its input space.

The symmetry (tests/test_codewords.py holds it on every reference, tests/test_real_codewords_gpu.py on every kernel): for a codeword c,
negate the channel LLRs where c is 1.  A min-sum decoder in any IEEE format then stops at the same turn with the same flag, returns its
bits XOR c and its final LLRs negated at those positions, bit for bit: negation commutes with every rounding, min and |.| do not see it,
and the product of the signs along a row changes by (-1)^(row . c) = 1.  Where a final LLR is exactly zero hard(0) = 0 for both frames,
so bits are compared where final_lam != 0.

codewords() goes through tests/systematic_encoder_spec.py (any H, Gaussian elimination over GF(2): at most 0.1 s up to 1024 x 10240) and,
where that would take many seconds (M >= 4000: dvbs2_short, dvbs2_natural, dvbs2short-20x45-sz360), through tests/sparse_encoder_spec.py,
which takes an H with a triangular parity part as those are."""
from __future__ import annotations

import numpy as np

from oracle import channel
from tests import sparse_encoder_spec as sparse
from tests import systematic_encoder_spec as systematic

ELIMINATION_ROWS = 4000          # from this many rows on the elimination takes seconds: the triangular encoder instead
_forms = {}


def _csr(H_or_graph):
    """-> (row_ptr, col_idx, N) of a dense 0/1 matrix or of anything with row_ptr / col_idx (or rp / ci) and N"""
    g = H_or_graph
    if isinstance(g, np.ndarray):
        rp, ci = systematic.csr(g)
        return rp, ci, g.shape[1]
    rp = g.row_ptr if hasattr(g, "row_ptr") else g.rp
    ci = g.col_idx if hasattr(g, "col_idx") else g.ci
    return np.asarray(rp, np.int32), np.asarray(ci, np.int32), int(g.N)


def _dense(rp, ci, N):
    H = np.zeros((len(rp) - 1, N), np.uint8)
    H[np.repeat(np.arange(len(rp) - 1), np.diff(rp)), ci] = 1
    return H


def _form(rp, ci, N):
    """the encoder of one matrix, computed once: ("sparse", order) or ("systematic", msg_pos, par_pos, P)"""
    key = (N, rp.tobytes(), ci.tobytes())
    if key not in _forms:
        form = None
        if len(rp) - 1 >= ELIMINATION_ROWS:
            try:
                form = ("sparse", sparse.triangular_order(rp, ci, N))
            except sparse.Refused:          # (1920.1280.A: 5760 redundant rows of 1920 columns, eliminated in 0.1 s)
                pass
        _forms[key] = form or ("systematic",) + systematic.systematic_form(_dense(rp, ci, N))
    return _forms[key]


def dimension(H_or_graph):
    """K = N - rank H, the number of message bits"""
    rp, ci, N = _csr(H_or_graph)
    f = _form(rp, ci, N)
    return N - (len(rp) - 1) if f[0] == "sparse" else len(f[1])


def codewords(H_or_graph, F, seed):
    """-> [F][N] uint8: the codewords of F random messages (each bit 0 or 1 with probability 1/2); H c = 0 is asserted on every word"""
    rp, ci, N = _csr(H_or_graph)
    f = _form(rp, ci, N)
    rng = np.random.default_rng(seed)
    if f[0] == "sparse":
        cw = sparse.encode(rp, ci, N, f[1], rng.integers(0, 2, (F, N - (len(rp) - 1))).astype(np.uint8))
    else:
        cw = systematic.encode(N, f[1], f[2], f[3], rng.integers(0, 2, (F, len(f[1]))).astype(np.uint8))
    assert cw.shape == (F, N) and cw.dtype == np.uint8 and cw.max(initial=0) <= 1
    assert not sparse.syndrome(rp, ci, cw).any(), "a drawn word is no codeword"
    return cw


def flip(llr, cw):
    """llr negated where cw is 1 (the dtype is kept; a zero becomes -0 in a float format)"""
    llr, cw = np.asarray(llr), np.asarray(cw)
    assert llr.shape == cw.shape
    return np.where(cw != 0, -llr, llr).astype(llr.dtype)


def noisy(cws, ebn0_db, k, N, seed):
    """-> [F][N] float64 holding float32 values: oracle/channel.py frames of the words, UNPUNCTURED (n_tx = N), so that no channel LLR
    is zero -- asserted: a zero is decided in the all-zero word's favour"""
    cws = np.asarray(cws, np.uint8)
    assert cws.ndim == 2 and cws.shape[1] == N
    llr = channel.frames(cws, ebn0_db, k, N, N, seed)
    assert np.isfinite(llr).all() and (llr != 0).all()
    return llr


def noiseless(cw, amp=8.0):
    """-> [2][N] float32: the word at +-amp and its flip (the all-zero word at -amp)"""
    l = np.where(np.asarray(cw) != 0, amp, -amp).astype(np.float32)
    return np.stack([l, flip(l, cw)])
