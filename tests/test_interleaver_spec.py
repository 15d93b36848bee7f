"""CPU: the bit interleaver's host side (csrc/interleaver.cc, the checks of ldpc_interleaver_create_on) against tests/interleaver_spec.py,
and the spec's own properties.  Nothing here needs a device: a table is checked before the device is touched, so on a machine with a
GPU the refusals are the same and a VALID table is not tried here at all."""
import ctypes as C

import numpy as np
import pytest

import ecc_ldpc_amd as E
from tests import interleaver_spec as ils
from tests import modulation_spec as ms

EINVAL = -1
NEW_SYMBOLS = ["ldpc_interleaver_create_on", "ldpc_interleaver_destroy", "ldpc_interleaver_dims", "ldpc_interleaver_positions", "ldpc_interleaver_block_positions",
               "ldpc_demap_dev_il", "ldpc_sim_transmit_il", "ldpc_sim_generate_mod_il", "ldpc_interleave_bits_dev", "ldpc_deinterleave_llr_dev"]
SHAPES = [(1, 1), (7, 1), (1, 6), (640, 3), (160, 12)]


def _i32(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


def _twists(rows, cols):
    rng = np.random.default_rng(100 * rows + cols)
    tw = rng.integers(0, rows, cols)
    tw[cols - 1] = rows - 1                                  # the largest twist
    return [None, tw, (np.arange(cols) * 7) % rows]


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_block_builder_equals_the_spec(rows, cols):
    rev = np.arange(cols)[::-1]
    shuffled = np.random.default_rng(cols).permutation(cols)
    for tw in _twists(rows, cols):
        for od in (None, rev, shuffled):
            want = ils.block_positions(rows, cols, tw, od)
            got = E.Interleaver.block_positions(rows, cols, tw, od)
            assert got.dtype == np.int32 and np.array_equal(got, want), (rows, cols, tw, od)
            assert sorted(got.tolist()) == list(range(rows * cols))            # a permutation
            # the rule read the other way: codeword bit c rows + u sits at row (u + twist[c]) mod rows of column c, read at column slot j
            t = int(np.random.default_rng(1).integers(0, rows * cols))
            r, j = divmod(t, cols)
            c = int((np.arange(cols) if od is None else od)[j])
            u = int(got[t]) - c * rows
            assert 0 <= u < rows and (u + (0 if tw is None else int(tw[c]))) % rows == r
    plain = E.Interleaver.block_positions(rows, cols)
    assert np.array_equal(plain, np.arange(rows * cols).reshape(cols, rows).T.reshape(-1))      # no twist, identity order: the transpose
    assert ils.holes(plain, rows * cols).size == 0


def test_block_builder_refusals():
    L = E.lib()
    out, po = _i32(np.zeros(64))

    def refused(rows, cols, tw=None, od=None, pos=po):
        t = None if tw is None else _i32(tw)[1]
        o = None if od is None else _i32(od)[1]
        assert L.ldpc_interleaver_block_positions(rows, cols, t, o, pos) == EINVAL
        assert L.ldpc_last_error_code() == EINVAL and E.last_error()

    for rows, cols in ((0, 4), (4, 0), (-1, 4), (4, -3), (0, 0)):
        refused(rows, cols)
    refused(1 << 16, 1 << 15)                                # rows * cols = 2^31 does not fit an int
    refused(1 << 30, 4)
    refused(5, 3, tw=[0, 5, 1])                              # a twist outside 0 .. rows - 1
    refused(5, 3, tw=[0, -1, 1])
    for od in ([0, 1, 1], [0, 1, 3], [-1, 0, 1], [2, 2, 2]):  # not a permutation of 0 .. cols - 1
        refused(5, 3, od=od)
    refused(5, 3, pos=None)
    assert (out == 0).all()                                  # a refused call writes nothing
    assert L.ldpc_interleaver_block_positions(5, 3, _i32([4, 0, 2])[1], _i32([2, 0, 1])[1], po) == 0
    assert np.array_equal(out[:15], ils.block_positions(5, 3, [4, 0, 2], [2, 0, 1]))
    with pytest.raises(E.LdpcError) as e:
        E.Interleaver.block_positions(5, 3, twist=[0, 1])    # a twist of the wrong length never reaches the library
    assert e.value.code == EINVAL


def test_create_refusals_need_no_device():
    L = E.lib()

    def refused(n_tx, N, pos):
        p = None if pos is None else _i32(pos)[1]
        for device in (0, -1, 3):                            # whatever the device: the table is judged first
            assert not L.ldpc_interleaver_create_on(device, n_tx, N, p)
            assert L.ldpc_last_error_code() == EINVAL and E.last_error()

    refused(4, 8, None)                                      # a null table
    refused(0, 8, [0])                                       # n_tx < 1
    refused(-2, 8, [0])
    refused(9, 8, list(range(9)))                            # n_tx > N
    refused(3, 8, [0, 8, 1])                                 # an entry outside 0 .. N - 1
    refused(3, 8, [0, -1, 1])
    refused(4, 8, [5, 2, 7, 2])                              # a repeated entry
    refused(8, 8, [0, 1, 2, 3, 4, 5, 6, 0])
    for pos, N in (([0, 8, 1], 8), ([3, 3], 4), (list(range(9)), 8), ([], 4)):
        with pytest.raises(E.LdpcError) as e:
            E.Interleaver(np.asarray(pos, np.int64), N)
        assert e.value.code == EINVAL
    with pytest.raises(E.LdpcError) as e:
        E.Interleaver(np.array([0.0, 1.0]), 4)               # no integers
    assert e.value.code == EINVAL
    # the other entry points refuse a null object before anything else
    assert L.ldpc_interleaver_dims(None, None, None) == EINVAL and L.ldpc_interleaver_positions(None, None) == EINVAL
    assert L.ldpc_demap_dev_il(None, None, 1, None, 0.1, None, 0, 0.0, None) == EINVAL
    assert L.ldpc_interleave_bits_dev(None, 1, None, 0, None, 0, None) == EINVAL
    assert L.ldpc_deinterleave_llr_dev(None, 1, None, None, 0, None) == EINVAL
    L.ldpc_interleaver_destroy(None)                         # as free(NULL)


@pytest.mark.skipif(E.lib().ldpc_device_count() > 0, reason="this check is for GPU-less hosts")
def test_a_valid_table_without_a_device_is_enodevice():
    with pytest.raises(E.LdpcError) as e:
        E.Interleaver(np.arange(8, dtype=np.int32)[::-1], 8)
    assert e.value.code == -4
    with pytest.raises(E.LdpcError) as e:
        E.Interleaver.block(4, 2)
    assert e.value.code == -4


def test_spec_round_trip_and_holes():
    rng = np.random.default_rng(5)
    for n_tx, N in ((13, 13), (13, 20), (1280, 1408), (1, 5)):
        pos = rng.permutation(N)[:n_tx].astype(np.int32)
        h = ils.holes(pos, N)
        assert h.dtype == np.int32 and (np.diff(h) > 0).all()
        assert sorted(h.tolist() + pos.tolist()) == list(range(N))              # exactly the complement
        x = rng.normal(size=(3, N)).astype(np.float32)
        x[x == 0] = 1.0
        tx = ils.interleave(x, pos)                          # data in interleave order ...
        assert tx.shape == (3, n_tx) and all(tx[1, t] == x[1, pos[t]] for t in range(n_tx))
        back = ils.deinterleave(tx, pos, N)                  # ... comes back to its places; the punctured ones are 0
        assert back.dtype == x.dtype and np.array_equal(back[:, pos], x[:, pos]) and (back[:, h] == 0).all()
        if n_tx == N:
            assert np.array_equal(back, x)
        for dt in (np.float16, np.int8):
            assert ils.deinterleave(tx.astype(dt), pos, N).dtype == dt
        bits = rng.integers(0, 2, (3, N)).astype(np.uint8)
        assert np.array_equal(np.unpackbits(ils.pack(ils.interleave(bits, pos)), axis=1, bitorder="little")[:, :n_tx], bits[:, pos])
    with pytest.raises(AssertionError):
        ils.holes([0, 0], 4)
    with pytest.raises(AssertionError):
        ils.holes([0, 4], 4)


def test_identity_table_is_the_demapper_of_the_modulation_spec():
    rng = np.random.default_rng(9)
    for pts, n_tx, N in ((ms.builtin(ms.PSK8), 13, 20), (ms.builtin(ms.QAM16), 16, 16), (ms.grid64(), 31, 40)):
        m = ms.bits_per_symbol(pts)
        ns = ms.symbols_per_frame(n_tx, m)
        sym = (pts[rng.integers(0, len(pts), (4, ns))] + rng.normal(0, 0.2, (4, ns, 2))).astype(np.float32)
        sym[0, 0] = (np.nan, 0.5)
        ident = np.arange(n_tx, dtype=np.int32)
        for fmt, qs in ((ms.LLR_F32, 4.0), (ms.LLR_F16, 4.0), (ms.LLR_I8, 2.5)):
            got, want = ils.demap_il(pts, sym, ident, N, 0.05, fmt, qs), ms.demap(pts, sym, n_tx, N, 0.05, fmt, qs)
            assert got.dtype == want.dtype and (got[:, n_tx:] == 0).all()                        # the tail zeros
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.nan_to_num(got), np.nan_to_num(want))
        # and a real table only moves those values
        pos = rng.permutation(N)[:n_tx].astype(np.int32)
        moved, flat = ils.demap_il(pts, sym, pos, N, 0.05), ms.demap(pts, sym, n_tx, n_tx, 0.05)
        assert np.array_equal(np.nan_to_num(moved[:, pos]), np.nan_to_num(flat)) and (moved[:, ils.holes(pos, N)] == 0).all()


def test_iq_alternating_table():
    m, b = 8, 4
    pos = ils.block_positions(6, m)
    alt = ils.iq_alternating(pos, m)
    assert sorted(alt.tolist()) == sorted(pos.tolist())
    for s in range(6):
        for j in range(b):
            assert alt[m * s + 2 * j] == pos[m * s + j] and alt[m * s + 2 * j + 1] == pos[m * s + b + j]


def test_abi_symbols_and_version():
    L = C.CDLL(E.SO_PATH)
    for s in NEW_SYMBOLS:
        assert s in E.ABI_SYMBOLS and hasattr(L, s), s
    assert E.lib().ldpc_abi_version() == 3
    for name in ("Interleaver", "demap_il", "interleave_bits", "deinterleave_llr"):
        assert hasattr(E, name)
    assert hasattr(E.Sim, "transmit_il") and hasattr(E.Sim, "generate_mod_il")
    from ecc_ldpc_amd import _lib
    assert "Interleaver" in _lib._CLOSE_ORDER
