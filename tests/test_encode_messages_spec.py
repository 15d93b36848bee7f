"""CPU: the bit layouts of tests/encode_messages_spec.py are inverses of each other on ragged sizes and agree with numpy's own
little-endian packing; the built library exports the three entry points for caller-supplied messages and Sim has their methods."""
import ctypes

import numpy as np
import pytest

import ecc_ldpc_amd as E
from tests import encode_messages_spec as spec


@pytest.mark.parametrize("n,kind", [(7, "message"), (648, "message"), (17, "codeword")])
def test_pack_and_unpack_are_inverses(n, kind):
    rng = np.random.default_rng(n)
    bits = rng.integers(0, 2, (5, n)).astype(np.uint8)
    bits[0], bits[1] = 0, 1
    rb = spec.message_row_bytes(n) if kind == "message" else spec.codeword_row_bytes(n)
    assert rb == {7: 4, 648: 84, 17: 3}[n]
    packed = (spec.pack_messages if kind == "message" else spec.pack_codewords)(bits)
    assert packed.shape == (5, rb) and packed.dtype == np.uint8
    assert np.array_equal(spec.unpack(packed, n), bits)
    # numpy's LSB-first packing, padded with zero bytes to the row: the same bytes, so the pad bits are zero
    want = np.zeros((5, rb), np.uint8)
    nb = np.packbits(bits, axis=1, bitorder="little")
    want[:, :nb.shape[1]] = nb
    assert np.array_equal(packed, want)
    # read as little-endian 32-bit words, bit i of word w is message bit 32 w + i
    if kind == "message":
        words = packed.view("<u4")
        i = np.arange(n)
        assert np.array_equal(((words[:, i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(np.uint8), bits)
    # only bit 0 of an input byte counts; pad bits are ignored on the way back
    assert np.array_equal(spec.pack(bits | 0xFE, rb), packed)
    dirty = packed.copy()
    if 8 * rb > n:
        dirty[:, -1] |= np.uint8((0xFF << (n & 7)) & 0xFF) if (n & 7) and (n + 7) // 8 == rb else np.uint8(0xFF)
        assert not np.array_equal(dirty, packed)
    assert np.array_equal(spec.unpack(dirty, n), bits)


def test_library_exports_the_three_entry_points():
    L = ctypes.CDLL(E.SO_PATH)
    for s in ("ldpc_sim_encode_messages", "ldpc_sim_generate_from", "ldpc_sim_extract_messages"):
        assert s in E.ABI_SYMBOLS and hasattr(L, s), s


def test_sim_has_the_three_methods():
    for m in ("encode_messages", "generate_from", "extract_messages"):
        assert callable(getattr(E.Sim, m, None)), m
