"""CPU: ldpc_csr_layer_order (host code, no GPU) -- an order of the rows of any H in which consecutive rows form few column-disjoint
layers, for the on-chip layered kernel of any H (csrc/layered_csr.hip)."""
import numpy as np
import pytest

import ecc_ldpc_amd as E
from tests import dvbs2_natural
from tests.helpers import load


def _graph(name):
    if name == "dvbs2-natural":
        rp, ci = dvbs2_natural.csr()
        return rp, ci, dvbs2_natural.N
    c = load(name)
    return c.graph.row_ptr.astype(np.int32), c.graph.col_idx.astype(np.int32), c.N


def _check_layers(rp, ci, N, perm, lp):
    M = len(rp) - 1
    assert np.array_equal(np.sort(perm), np.arange(M))                      # a permutation of the rows
    assert lp[0] == 0 and lp[-1] == M and np.all(np.diff(lp) > 0)           # strictly increasing from 0 to M
    prp, pci = E.Code.permute_rows(rp, ci, perm)
    layer_of_row = np.repeat(np.arange(len(lp) - 1), np.diff(lp))
    layer_of_edge = np.repeat(layer_of_row, np.diff(prp))
    key = layer_of_edge.astype(np.int64) * N + pci
    assert len(np.unique(key)) == len(key), "two rows of a layer share a column"
    return prp, pci


@pytest.mark.parametrize("name", ["moon.7.13", "1920.1280.3.303", "1920.1280.A", "dvbs2-natural"])
def test_layers_are_column_disjoint_and_few(name):
    rp, ci, N = _graph(name)
    perm, lp = E.Code.csr_layer_order(rp, ci, N)
    prp, pci = _check_layers(rp, ci, N, perm, lp)
    max_col = np.bincount(ci, minlength=N).max()
    assert len(lp) - 1 <= 3 * max_col, (name, len(lp) - 1, max_col)
    perm2, lp2 = E.Code.csr_layer_order(rp, ci, N)                          # deterministic
    assert np.array_equal(perm, perm2) and np.array_equal(lp, lp2)
    code = E.Code.from_csr(prp, pci, N)                                     # what the permuted code's set_layers takes
    code.set_layers(lp)
    assert np.array_equal(code.layers(), lp)


def test_first_fit_counts_on_the_shipped_codes():
    """first fit in file order: 11, 6 and 35 layers (bounds 3 x heaviest column: 27, 9, 54)"""
    got = [len(E.Code.csr_layer_order(*_graph(n))[1]) - 1 for n in ("moon.7.13", "1920.1280.3.303", "1920.1280.A")]
    assert got == [11, 6, 35], got


@pytest.mark.parametrize("max_rows", [1, 2, 7, 100])
def test_max_rows_is_honoured(max_rows):
    rp, ci, N = _graph("1920.1280.3.303")
    perm, lp = E.Code.csr_layer_order(rp, ci, N, max_rows=max_rows)
    _check_layers(rp, ci, N, perm, lp)
    assert np.diff(lp).max() <= max_rows
    if max_rows == 1:
        assert np.array_equal(perm, np.arange(len(rp) - 1))                 # one row per layer: file order


def test_irregular_random_graph():
    rng = np.random.default_rng(7)
    M, N = 300, 500
    rows = [np.sort(rng.choice(N, int(rng.integers(2, 15)), replace=False)) for _ in range(M)]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    perm, lp = E.Code.csr_layer_order(rp, ci, N)
    _check_layers(rp, ci, N, perm, lp)
    # rows of a layer keep their file order
    for a, b in zip(lp[:-1], lp[1:]):
        assert np.all(np.diff(perm[a:b]) > 0)


def test_bad_arguments():
    rp, ci, N = _graph("moon.7.13")
    bad = [
        (rp, ci, N, -1),                                       # negative cap
        (rp, ci, 0, 0),                                        # no columns
        (rp[:1], ci[:0], N, 0),                                # no rows
        (rp, np.where(ci == ci.max(), N, ci), N, 0),           # column out of range
        (rp, ci[::-1].copy(), N, 0),                           # columns not ascending inside a row
        (np.concatenate([[1], rp[1:]]), ci, N, 0),             # row_ptr[0] != 0
    ]
    for args in bad:
        with pytest.raises(E.LdpcError) as e:
            E.Code.csr_layer_order(args[0], args[1], args[2], max_rows=args[3])
        assert e.value.code == -1
