"""The two bit layouts of ldpc_sim_encode_messages / _generate_from / _extract_messages (include/ldpc_hip.h ldpc_bit_format), in numpy.

bytes: one byte per bit; a reader takes bit 0 of a byte.  packed: bit i of a row sits in byte i / 8 at bit i % 8.  A packed MESSAGE row
is 4 * ceil(k / 32) bytes (whole little-endian 32-bit words), a packed CODEWORD row ceil(n_tx / 8) bytes; pad bits are 0.
TEST INFRASTRUCTURE: nothing under ecc_ldpc_amd/ imports it, and it shares no code with the library."""
from __future__ import annotations

import numpy as np


def message_row_bytes(k):
    return 4 * ((k + 31) // 32)


def codeword_row_bytes(n_tx):
    return (n_tx + 7) // 8


def pack(bits, row_bytes):
    """bits [F][n] (bit 0 of each byte counts) -> packed [F][row_bytes] uint8, pad bits 0"""
    bits = np.asarray(bits, np.uint8) & 1
    F, n = bits.shape
    assert 8 * row_bytes >= n
    out = np.zeros((F, row_bytes), np.uint8)
    for i in range(n):
        out[:, i >> 3] |= bits[:, i] << (i & 7)
    return out


def unpack(packed, n):
    """packed [F][row_bytes] -> bits [F][n] uint8 0/1; whatever sits in the pad bits is ignored"""
    packed = np.asarray(packed, np.uint8)
    assert 8 * packed.shape[1] >= n
    i = np.arange(n)
    return (packed[:, i >> 3] >> (i & 7).astype(np.uint8)) & 1


def pack_messages(msg):
    return pack(msg, message_row_bytes(np.asarray(msg).shape[1]))


def pack_codewords(cw):
    return pack(cw, codeword_row_bytes(np.asarray(cw).shape[1]))
