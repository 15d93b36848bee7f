"""CPU: the rule of the encoder from H.  The numpy restatement (tests/sparse_encoder_spec.py) against H itself (H c = 0) and, on
codes/moon.7.13, against the shipped generator for all 128 messages; the library's ldpc_csr_triangular_order (host code, no GPU)
against the restatement's order, and its refusals: which row, or which two rows and which column."""
import os

import numpy as np
import pytest

import ecc_ldpc_amd as E
from oracle import oracle
from tests import dvbs2_natural, dvbs2_short
from tests import sparse_encoder_spec as spec
from tests.helpers import CODES, load


def _moon():
    c = load("moon.7.13")
    return c.graph.row_ptr, c.graph.col_idx, c.N


def _mackay(name):
    c = load(name)
    return c.graph.row_ptr, c.graph.col_idx, c.N


def _jpl1024():
    c = load("jpl.1024.4.5")
    return c.graph.row_ptr, c.graph.col_idx, c.N


def _short_in_layer_order():
    rp, ci = dvbs2_short.csr()
    perm, _ = E.Code.csr_layer_order(rp, ci, dvbs2_short.N)
    assert not np.array_equal(perm, np.arange(len(perm)))
    return (*E.Code.permute_rows(rp, ci, perm), dvbs2_short.N), perm


def test_the_restatement_satisfies_H():
    rng = np.random.default_rng(5)
    for what, (rp, ci, N), F in (("toy", spec.toy(70, 45), 40), ("toy for the decoder", spec.toy_decodable(), 40),
                                 ("dvbs2_short", (*dvbs2_short.csr(), dvbs2_short.N), 5)):
        M = len(rp) - 1
        order = spec.triangular_order(rp, ci, N)
        assert sorted(order.tolist()) == list(range(M)), what
        msg = rng.integers(0, 2, size=(F, N - M), dtype=np.uint8)
        cw = spec.encode(rp, ci, N, order, msg)
        assert np.array_equal(cw[:, :N - M], msg) and not spec.syndrome(rp, ci, cw).any(), what
        assert 0.3 < cw[:, N - M:].mean() < 0.7, what
    assert np.array_equal(spec.triangular_order(*dvbs2_short.csr(), dvbs2_short.N), np.arange(dvbs2_short.M))   # natural order: identity
    rp, ci, N = spec.toy(70, 45)
    assert (np.diff(rp) == 1).sum() >= 1                                        # rows of weight 1: a parity bit that is always 0


def test_moon_equals_its_shipped_generator_for_every_message():
    rp, ci, N = _moon()
    c = load("moon.7.13")
    assert (c.M, c.N, c.G.shape) == (13, 20, (7, 13))
    order = spec.triangular_order(rp, ci, N)
    msg = ((np.arange(128)[:, None] >> np.arange(7)) & 1).astype(np.uint8)
    cw = spec.encode(rp, ci, N, order, msg)
    assert not spec.syndrome(rp, ci, cw).any()
    assert np.array_equal(cw[:, 7:], np.stack([oracle.encode_dense(c.G, m) for m in msg]))


def test_row_storage_order_does_not_change_the_codewords():
    rp, ci = dvbs2_short.csr()
    (prp, pci, N), perm = _short_in_layer_order()
    msg = np.random.default_rng(6).integers(0, 2, size=(3, dvbs2_short.K), dtype=np.uint8)
    a = spec.encode(rp, ci, N, spec.triangular_order(rp, ci, N), msg)
    b = spec.encode(prp, pci, N, spec.triangular_order(prp, pci, N), msg)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["moon.7.13", "toy", "dvbs2_short", "dvbs2_natural", "dvbs2_short in csr_layer_order order"])
def test_library_order_equals_the_restatement(name):
    rp, ci, N = {"moon.7.13": _moon, "toy": lambda: spec.toy(70, 45), "dvbs2_short": lambda: (*dvbs2_short.csr(), dvbs2_short.N),
                 "dvbs2_natural": lambda: (*dvbs2_natural.csr(), dvbs2_natural.N),
                 "dvbs2_short in csr_layer_order order": lambda: _short_in_layer_order()[0]}[name]()
    got = E.Code.csr_triangular_order(rp, ci, N)
    assert got.dtype == np.int32 and np.array_equal(got, spec.triangular_order(rp, ci, N))
    if name == "dvbs2_short in csr_layer_order order":                         # order undoes the permutation: row perm[i] sits at place i
        perm = _short_in_layer_order()[1]
        assert np.array_equal(perm[got], np.arange(len(perm)))


def _refused(rp, ci, N):
    with pytest.raises(spec.Refused) as want:
        spec.triangular_order(rp, ci, N)
    with pytest.raises(E.LdpcError) as got:
        E.Code.csr_triangular_order(rp, ci, N)
    assert got.value.code == -5                                                  # LDPC_EUNSUPPORTED
    return want.value, str(got.value)


@pytest.mark.parametrize("name", ["1920.1280.3.303", "jpl.1024.4.5"])
def test_refuses_two_rows_that_end_in_one_column(name):
    rp, ci, N = _mackay(name) if name.startswith("1920") else _jpl1024()
    want, text = _refused(rp, ci, N)
    assert len(want.rows) == 2 and f"rows {want.rows[0]} and {want.rows[1]} end in column {want.column}" in text, (want, text)


def test_refuses_more_rows_than_columns():
    rp, ci, N = _mackay("1920.1280.A")
    assert len(rp) - 1 == 5760 and N == 1920
    _, text = _refused(rp, ci, N)
    assert "5760" in text and "1920" in text, text


def test_refuses_the_staircase_closed_into_a_ring():
    rp, ci = spec.ring(*dvbs2_short.csr(), dvbs2_short.N)
    want, text = _refused(rp, ci, dvbs2_short.N)
    assert (want.rows, want.column) == ((0, 8999), 16199)
    assert "rows 0 and 8999 end in column 16199" in text, text


def test_refuses_an_empty_row_and_a_row_inside_the_message_part():
    rp, ci, N = spec.toy(70, 45)
    rows = [ci[rp[i]:rp[i + 1]] for i in range(70)]
    empty = rows[:11] + [rows[11][:0]] + rows[12:]
    want, text = _refused(*spec._csr(empty), N)
    assert want.rows == (11,) and "row 11 is empty" in text, text
    order = spec.triangular_order(rp, ci, N)
    i = int(order[20])                                                          # a row with message bits: cut it back to them
    assert (rows[i] < 45).any()
    inside = rows[:i] + [rows[i][rows[i] < 45]] + rows[i + 1:]
    want, text = _refused(*spec._csr(inside), N)
    assert want.rows == (i,) and f"row {i} ends in column {want.column}" in text, text


def test_malformed_csr_is_an_argument_error():
    for rp, ci, N in (([0, 2], [1, 1], 3), ([0, 1], [5], 3), ([0, 2, 1], [0, 1], 3), ([1, 2], [0, 1], 3)):
        with pytest.raises(E.LdpcError) as e:
            E.Code.csr_triangular_order(rp, ci, N)
        assert e.value.code == -1, (rp, ci)                                      # LDPC_EINVAL


def test_abi_keeps_its_version_and_names_the_new_encoder():
    assert E.lib().ldpc_abi_version() == 3
    hdr = open(os.path.join(os.path.dirname(CODES), "include", "ldpc_hip.h")).read()
    assert "LDPC_ENCODER_SPARSE = 3" in hdr
    for s in ("ldpc_csr_triangular_order", "ldpc_sim_create_sparse_on"):
        assert s in E.ABI_SYMBOLS and hasattr(E.lib(), s)
