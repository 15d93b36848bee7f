"""CPU: the rule of the encoder from any H (tests/systematic_encoder_spec.py) against brute force -- rank computations and H c = 0 --
and the library's host helper ldpc_csr_systematic_form against that restatement, on random matrices with every defect the rule
must survive and on the five shipped matrices, with the known answers of the shipped ones pinned."""
import os
import re
import time

import numpy as np
import pytest

import ecc_ldpc_amd as E
from oracle import formats
from tests import dvbs2_natural
from tests import sparse_encoder_spec as sparse_spec
from tests import systematic_encoder_spec as spec
from tests.helpers import ROOT, load

SHIPPED = ["moon.7.13", "jpl.1024.4.5", "jpl.4096.4.5", "1920.1280.3.303", "1920.1280.A"]
LOW_PARITY_1920 = [447, 504, 558, 571, 590, 616, 622, 626]


def _all_cases():
    out = dict(spec.cases())
    rp, ci, N = sparse_spec.toy(12, 9)                     # triangular parity part: the rule must give msg ++ parity
    H = np.zeros((12, N), np.uint8)
    for i in range(12):
        H[i, ci[rp[i]:rp[i + 1]]] = 1
    out["toy-triangular"] = H
    return out


def _greedy_from_the_right(H):
    """the parity positions by the rule's own words: one rank computation per column"""
    N = H.shape[1]
    chosen, r = [], 0
    for c in range(N - 1, -1, -1):
        r2 = formats.gf2_rank(H[:, chosen + [c]])
        if r2 > r:
            chosen, r = chosen + [c], r2
    return np.array(sorted(chosen), np.int32)


def _messages(K, seed=5):
    if K <= 7:
        return ((np.arange(2 ** K)[:, None] >> np.arange(K)) & 1).astype(np.uint8)
    m = np.random.default_rng(seed).integers(0, 2, (40, K)).astype(np.uint8)
    m[0], m[1] = 0, 1
    return m


def test_moon_equals_its_shipped_generator_for_all_128_messages():
    c = load("moon.7.13")
    mp, pp, P = spec.systematic_form(c.H)
    assert np.array_equal(mp, np.arange(7)) and np.array_equal(pp, np.arange(7, 20))
    msgs = _messages(7)
    assert len(msgs) == 128
    want = np.stack([c.encode(m) for m in msgs])
    assert np.array_equal(spec.encode(20, mp, pp, P, msgs), want)


@pytest.mark.parametrize("name", list(_all_cases()))
def test_restatement_against_brute_force(name):
    H = _all_cases()[name]
    M, N = H.shape
    mp, pp, P = spec.systematic_form(H)
    K, r = len(mp), len(pp)
    assert K + r == N and r == formats.gf2_rank(H) and P.shape == (K, r)
    assert np.array_equal(pp, _greedy_from_the_right(H))
    assert formats.gf2_rank(H[:, pp]) == r                                # full column rank: the parity bits are unique
    assert np.array_equal(np.sort(np.concatenate([mp, pp])), np.arange(N)) and (np.diff(mp) > 0).all() and (np.diff(pp) > 0).all()
    msgs = _messages(K)
    c = spec.encode(N, mp, pp, P, msgs)
    assert not spec.syndrome(H, c).any()
    assert np.array_equal(c[:, mp], msgs)


def test_the_cases_hold_every_defect():
    cs = _all_cases()
    has = lambda f: [n for n, H in cs.items() if f(H)]
    dup = lambda H: len(np.unique(H[H.any(1)], axis=0)) < H.any(1).sum()
    eqc = lambda H: len(np.unique(H.T[H.any(0)], axis=0)) < H.any(0).sum()
    dep = lambda H: formats.gf2_rank(H[:, H.shape[1] - formats.gf2_rank(H):]) < formats.gf2_rank(H)
    empty = lambda H: (~H.any(1)).any()
    zero = lambda H: (~H.any(0)).any()
    for f in (dup, empty, zero, eqc, dep):
        assert has(f)
    assert [n for n, H in cs.items() if sum(bool(f(H)) for f in (dup, empty, zero, eqc, dep)) >= 3]
    shapes = [H.shape for H in cs.values()]
    assert (3, 5) in shapes and (40, 90) in shapes
    assert not dep(cs["toy-triangular"])


def test_tail_parity_gives_msg_then_parity_like_the_triangular_rule():
    rp, ci, N = sparse_spec.toy(12, 9)
    H = _all_cases()["toy-triangular"]
    mp, pp, P = spec.systematic_form(H)
    assert np.array_equal(mp, np.arange(9)) and np.array_equal(pp, np.arange(9, N))
    msgs = _messages(9)
    assert np.array_equal(spec.encode(N, mp, pp, P, msgs), sparse_spec.encode(rp, ci, N, sparse_spec.triangular_order(rp, ci, N), msgs))


def _library(H):
    rp, ci = spec.csr(H)
    return E.Code.csr_systematic_form(rp, ci, H.shape[1])


@pytest.mark.parametrize("name", list(_all_cases()))
def test_library_helper_equals_the_restatement(name):
    H = _all_cases()[name]
    mp, pp, P = spec.systematic_form(H)
    lm, lp, LP = _library(H)
    assert np.array_equal(lm, mp) and np.array_equal(lp, pp) and np.array_equal(LP, P)
    perm = np.random.default_rng(3).permutation(H.shape[0])                  # the rule does not see how the rows are stored
    lm2, lp2, LP2 = _library(H[perm])
    assert np.array_equal(lm2, mp) and np.array_equal(lp2, pp) and np.array_equal(LP2, P)


@pytest.mark.parametrize("name", SHIPPED)
def test_library_helper_on_the_shipped_matrices(name):
    c = load(name)
    mp, pp, P = spec.systematic_form(c.H)
    lm, lp, LP = E.Code.csr_systematic_form(c.graph.row_ptr, c.graph.col_idx, c.N)
    assert np.array_equal(lm, mp) and np.array_equal(lp, pp) and np.array_equal(LP, P)
    lm2, lp2, none = E.Code.csr_systematic_form(c.graph.row_ptr, c.graph.col_idx, c.N, want_P=False)
    assert none is None and np.array_equal(lm2, lm) and np.array_equal(lp2, lp)
    K, r = {"moon.7.13": (7, 13), "jpl.1024.4.5": (1024, 384), "jpl.4096.4.5": (4096, 1536)}.get(name, (640, 1280))
    assert (len(lm), len(lp)) == (K, r)
    if name.startswith("1920"):
        assert lp[:8].tolist() == LOW_PARITY_1920 and lp[8:10].tolist() == [640, 643] and (lp[8:] >= 640).all()
        assert abs(LP.mean() - 0.376) < 0.0005
    else:
        assert np.array_equal(lp, np.arange(c.N - r, c.N)) and np.array_equal(lm, np.arange(K))
        if name.startswith("jpl"):
            assert abs(LP.mean() - 0.50) < 0.005
    if name == "moon.7.13":
        assert np.array_equal(LP, c.G[:, :13])


def test_redundant_checks_change_nothing():
    a, b = load("1920.1280.3.303"), load("1920.1280.A")
    fa = E.Code.csr_systematic_form(a.graph.row_ptr, a.graph.col_idx, a.N)
    fb = E.Code.csr_systematic_form(b.graph.row_ptr, b.graph.col_idx, b.N)
    for x, y in zip(fa, fb):
        assert np.array_equal(x, y)


def test_error_paths():
    with pytest.raises(E.LdpcError) as e:
        E.Code.csr_systematic_form([0, 2, 3], [1, 1, 0], 3)                  # columns not ascending
    assert e.value.code == -1 and "ascending" in str(e.value)
    with pytest.raises(E.LdpcError) as e:
        E.Code.csr_systematic_form([0, 2, 1], [0, 1], 3)                     # row_ptr decreases
    assert e.value.code == -1 and "row_ptr decreases" in str(e.value)
    with pytest.raises(E.LdpcError) as e:
        E.Code.csr_systematic_form([0, 1, 2], [0, 1], 2)                     # the 2 x 2 identity
    assert e.value.code == -5 and "no message bits" in str(e.value)
    rp, ci = dvbs2_natural.csr()
    t = time.perf_counter()
    with pytest.raises(E.LdpcError) as e:
        E.Code.csr_systematic_form(rp, ci, dvbs2_natural.N)
    assert time.perf_counter() - t < 1.0                                     # refused before any elimination
    assert e.value.code == -5 and "2^28" in str(e.value) and "ldpc_sim_create_sparse_on" in str(e.value)


def test_header_names_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    for s in ("ldpc_csr_systematic_form", "ldpc_sim_create_systematic_on", "ldpc_sim_message_length", "ldpc_sim_positions"):
        assert re.search(r"\b" + s + r"\s*\(", hdr), s
        assert s in E.ABI_SYMBOLS and hasattr(E.lib(), s)
    assert re.search(r"LDPC_ENCODER_SYSTEMATIC\s*=\s*4\b", hdr)
    assert "2^28" in hdr
