"""CPU: the host side of the CRC (csrc/crc.cc, the checks of ldpc_crc_create_on in csrc/api.cc) against tests/crc_spec.py, and the spec
against anchors it does not share code with: the check values of the built-in parameter sets and zlib's crc32.  Nothing here needs a
device: arguments are checked before the device is touched, so on a machine with a GPU the refusals are the same and a VALID object is
not created here at all."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import ecc_ldpc_amd as E
from tests import crc_spec as cs

EINVAL, ENODEVICE = E.EINVAL, -4
NEW_SYMBOLS = ["ldpc_crc_builtin", "ldpc_crc_bits_host", "ldpc_crc_table", "ldpc_crc_create_on", "ldpc_crc_destroy", "ldpc_crc_params", "ldpc_crc_attach_dev",
               "ldpc_crc_check_dev", "ldpc_sim_crc_check", "ldpc_sim_tally_crc"]

# (L, (w, poly, init, xorout)): the shapes of tests/test_crc_gpu.py -- the smallest at which the kernels can go wrong
SHAPES = [
    (1, cs.builtin("crc6")),
    (26, cs.builtin("crc6")),                 # k = 32 < 64: idle lanes
    (31, (1, 1, 0, 0)),                       # parity; k = 32 exactly
    (8, cs.builtin("crc32")),                 # the CRC bits span two words
    (40, cs.builtin("crc24a")),               # k = 64
    (57, (11, 0x621, 0x155, 0x7FF)),          # CRC bits 57..67 straddle a word; init and xorout not zero
    (1000, cs.builtin("crc24b")),
    (4072, cs.builtin("crc24c")),
]
SHAPE_IDS = [f"L{L}-w{p[0]}" for L, p in SHAPES]


def random_rows(B, L, w):
    """the random messages [.][k] of tests/test_crc_gpu.py; for w <= 6 at least 512 of them, so that at a pass rate of 2^-w both outcomes
    occur (the seeds are fixed: test_random_rows_give_both_outcomes)"""
    return np.random.default_rng(250 * L + w + B).integers(0, 2, (max(B, 512) if w <= 6 else B, L + w), dtype=np.uint8)


def test_random_rows_give_both_outcomes():
    for L, (w, poly, init, xorout) in SHAPES:
        for B in (1, 7):
            flags = cs.check_bytes(random_rows(B, L, w), L, w, poly, init, xorout)
            assert (flags.any() and not flags.all()) or w > 6, (L, w, B)


def _u8(a):
    a = np.ascontiguousarray(a, np.uint8)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint8))


def test_abi_symbols():
    L = C.CDLL(E.SO_PATH)
    for s in NEW_SYMBOLS:
        assert s in E.ABI_SYMBOLS and hasattr(L, s), s
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ldpc_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr, s
    assert hdr.index("ldpc_crc_builtin(") > hdr.index("int ldpc_sim_transmit_rm(")          # the section follows rate matching


# ---- the spec against anchors outside it
def test_spec_meets_the_check_values():
    bits = cs.check_string_bits()
    assert bits.shape == (72,) and bits[:8].tolist() == [0, 0, 1, 1, 0, 0, 0, 1]          # '1' = 0x31, MSB first
    for kind, (name, w, poly, init, xorout, want) in cs.BUILTINS.items():
        assert int(cs.crc_bits(bits, w, poly, init, xorout)) == want, name
    assert int(cs.crc_bits(bits, 24, 0x864CFB, 0xB704CE, 0)) == 0x21CF02


def test_zlib_identity_on_random_byte_strings():
    """(w = 32, poly 0x04C11DB7, init = xorout = 0xFFFFFFFF) over a packed row (bit i in byte i/8 at bit i%8) is zlib.crc32 of the bytes with
    its 32 bits reversed: zlib's CRC is the reflected form of the same generator, and the packed layout feeds the LSB of a byte first"""
    rng = np.random.default_rng(32)
    for n in (1, 2, 3, 4, 5, 9, 64, 257):
        data = rng.integers(0, 256, (6, n), dtype=np.uint8)
        bits = np.unpackbits(data, axis=-1, bitorder="little")
        got = cs.crc_bits(bits, *cs.builtin("crc32"))
        want = [cs.bitrev32(zlib.crc32(row.tobytes())) for row in data]
        assert got.tolist() == want, n
    # the same through the packed helpers: a row of the layout IS the byte string
    bits = rng.integers(0, 2, (3, 96), dtype=np.uint8)
    rows = cs.pack(bits)
    assert rows.shape == (3, 12) and np.array_equal(cs.unpack(rows, 96), bits)
    assert cs.crc_bits(bits, *cs.builtin("crc32")).tolist() == [cs.bitrev32(zlib.crc32(r.tobytes())) for r in rows]


# ---- the library's host functions against the spec
def test_builtin_parameters():
    for kind, (name, w, poly, init, xorout, _) in cs.BUILTINS.items():
        assert E.Crc.builtin_params(kind) == (w, poly, init, xorout) and E.Crc.builtin_params(name) == (w, poly, init, xorout)
        assert E.CRC_KINDS[name] == kind
    assert len(E.CRC_KINDS) == len(cs.BUILTINS) == 7
    L = E.lib()
    assert L.ldpc_crc_builtin(3, None, None, None, None) == 0               # any pointer may be NULL
    for kind in (-1, 7, 1000):
        assert L.ldpc_crc_builtin(kind, None, None, None, None) == EINVAL and L.ldpc_last_error_code() == EINVAL and E.last_error()


def test_bits_host_meets_the_check_values():
    bits = cs.check_string_bits()
    for kind, (name, w, poly, init, xorout, want) in cs.BUILTINS.items():
        assert E.Crc.bits_host(w, poly, init, xorout, bits) == want, name
    assert E.Crc.bits_host(24, 0x864CFB, 0xB704CE, 0, bits) == 0x21CF02
    assert E.Crc.bits_host(24, 0x864CFB, 0xB704CE, 0, bits | 0xFE) == 0x21CF02     # only bit 0 of a byte is read


@pytest.mark.parametrize("L,params", SHAPES, ids=SHAPE_IDS)
def test_bits_host_and_table_equal_the_spec(L, params):
    w, poly, init, xorout = params
    rng = np.random.default_rng(1000 * w + L)
    bits = rng.integers(0, 2, (5, L), dtype=np.uint8)
    bits[0], bits[1] = 0, 1
    want = cs.crc_bits(bits, w, poly, init, xorout)
    assert [E.Crc.bits_host(w, poly, init, xorout, row) for row in bits] == want.tolist()
    T = E.Crc.table(w, poly, L)
    assert T.dtype == np.uint32 and np.array_equal(T, cs.table(w, poly, L))
    assert (T < 2 ** w).all() and T[L - 1] == poly                           # the last payload bit sees one step of an empty register


@pytest.mark.parametrize("L,params", SHAPES + [(200, (24, 0x864CFB, 0xB704CE, 0x5A5A5A)), (77, (32, 0x04C11DB7, 0x12345678, 0x9ABCDEF0))],
                         ids=SHAPE_IDS + ["L200-w24-init-xorout", "L77-w32-init-xorout"])
def test_linear_form_equals_the_serial_form(L, params):
    """crc = C0 ^ XOR T[i]: what the kernels compute.  The shapes with init and xorout not zero are the ones where a wrong C0 shows"""
    w, poly, init, xorout = params
    bits = np.random.default_rng(7 * L + w).integers(0, 2, (9, L), dtype=np.uint8)
    bits[0] = 0
    serial = cs.crc_bits(bits, w, poly, init, xorout)
    assert np.array_equal(cs.crc_linear(bits, w, poly, init, xorout), serial)
    T = E.Crc.table(w, poly, L)                                              # and with the library's table and the library's C0
    c0 = E.Crc.bits_host(w, poly, init, xorout, np.zeros(L, np.uint8))
    lin = np.bitwise_xor.reduce(np.where(bits != 0, T, np.uint32(0)).astype(np.uint32), axis=-1) ^ np.uint32(c0)
    assert np.array_equal(lin, serial)


@pytest.mark.parametrize("L,params", SHAPES, ids=SHAPE_IDS)
def test_appending_the_crc_leaves_a_constant_residue(L, params):
    """the register run over payload ++ CRC (init as given, no xorout) ends in a value that depends on the parameters alone -- the
    register after w zero bits from xorout -- and a message with one bit flipped does not reach it"""
    w, poly, init, xorout = params
    rng = np.random.default_rng(13 * L + w)
    msg = np.zeros((6, L + w), np.uint8)
    msg[:, :L] = rng.integers(0, 2, (6, L))
    full = cs.attach_bytes(msg, L, w, poly, init, xorout)
    assert np.array_equal(full[:, :L], msg[:, :L]) and cs.check_bytes(full, L, w, poly, init, xorout).all()
    residue = cs.crc_bits(full, w, poly, init, 0)
    assert (residue == residue[0]).all()
    assert int(residue[0]) == int(cs.crc_bits(np.zeros(w, np.uint8), w, poly, xorout, 0))
    for at in (0, L - 1, L, L + w - 1):
        bad = full.copy()
        bad[:, at] ^= 1
        assert not cs.check_bytes(bad, L, w, poly, init, xorout).any()
        assert (cs.crc_bits(bad, w, poly, init, 0) != residue[0]).all()
    rows = cs.pack(full)                                                     # the packed forms agree with the byte forms
    junk = rows.copy()
    junk[:, (L + w) // 8:] |= np.uint8((0xFF << ((L + w) % 8)) & 0xFF) if (L + w) % 8 else 0
    if (L + w) % 32:
        junk[:, -1] |= 0x80
    assert np.array_equal(cs.attach_packed(junk, L, w, poly, init, xorout), rows) and cs.check_packed(rows, L, w, poly, init, xorout).all()


# ---- refusals, all before a device is needed
BAD = [
    ("width 0", (0, 1, 0, 0, 8)), ("width 33", (33, 1, 0, 0, 8)), ("width -1", (-1, 1, 0, 0, 8)),
    ("even poly", (8, 0x06, 0, 0, 8)), ("poly 0", (8, 0, 0, 0, 8)),
    ("poly >= 2^w", (6, 0x41, 0, 0, 8)), ("poly = 2^w + 1", (24, 0x1000001, 0, 0, 8)),
    ("init >= 2^w", (6, 0x21, 0x40, 0, 8)), ("xorout >= 2^w", (11, 0x621, 0, 0x800, 8)), ("init >= 2^1", (1, 1, 2, 0, 8)),
    ("n_bits 0", (24, 0x864CFB, 0, 0, 0)), ("n_bits -5", (24, 0x864CFB, 0, 0, -5)),
    ("k = 2^24 + 1", (24, 0x864CFB, 0, 0, 2 ** 24 - 23)), ("n_bits = 2^31 - 1", (32, 0x04C11DB7, 0, 0, 2 ** 31 - 1)),
]


@pytest.mark.parametrize("what,args", BAD, ids=[b[0] for b in BAD])
def test_create_refuses_before_a_device_is_needed(what, args):
    w, poly, init, xorout, n = args
    L = E.lib()
    for device in (-1, 0):                                                   # -1: no device at all would be LDPC_ENODEVICE, were it reached
        assert not L.ldpc_crc_create_on(device, w, poly, init, xorout, n), what
        assert L.ldpc_last_error_code() == EINVAL and E.last_error(), what
    with pytest.raises(E.LdpcError) as e:
        E.Crc(w, poly, init, xorout, n_bits=n, device=-1)
    assert e.value.code == EINVAL


def test_valid_parameters_reach_the_device_check():
    """the largest message (k = 2^24), w = 32 with every bit of poly, init and xorout set: accepted, so device -1 is the refusal"""
    L = E.lib()
    for w, poly, init, xorout, n in ((24, 0x864CFB, 0, 0, 2 ** 24 - 24), (32, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 1), (1, 1, 1, 1, 1)):
        assert not L.ldpc_crc_create_on(-1, w, poly, init, xorout, n)
        assert L.ldpc_last_error_code() == ENODEVICE


def test_host_functions_refuse_bad_arguments():
    L = E.lib()
    bits, pb = _u8(np.ones(8))
    out = C.c_uint32(77)
    tab = np.full(8, 77, np.uint32)
    pt = tab.ctypes.data_as(C.POINTER(C.c_uint32))
    for w, poly, init, xorout, n in [a for _, a in BAD]:
        if n >= 2 ** 31 - 1 or n > 8:
            continue                                                         # (the buffers here hold 8)
        assert L.ldpc_crc_bits_host(w, poly, init, xorout, n, pb, C.byref(out)) == EINVAL
        if init < 2 ** max(w, 0) and xorout < 2 ** max(w, 0):
            assert L.ldpc_crc_table(w, poly, n, pt) == EINVAL
    assert L.ldpc_crc_bits_host(8, 0x07, 0, 0, 8, None, C.byref(out)) == EINVAL
    assert L.ldpc_crc_bits_host(8, 0x07, 0, 0, 8, pb, None) == EINVAL
    assert L.ldpc_crc_table(8, 0x07, 8, None) == EINVAL
    assert out.value == 77 and (tab == 77).all()
    assert L.ldpc_crc_params(None, None, None, None, None, None) == EINVAL
    for call in (lambda: L.ldpc_crc_attach_dev(None, 1, None, 0, None), lambda: L.ldpc_crc_check_dev(None, 1, None, 0, None, None),
                 lambda: L.ldpc_sim_crc_check(None, None, 1, None, 0, None, None), lambda: L.ldpc_sim_tally_crc(None, 1, None, None, None, None)):
        assert call() == EINVAL and L.ldpc_last_error_code() == EINVAL
    with pytest.raises(E.LdpcError):
        E.Crc(8, 0x07, device=-1)                                            # n_bits is required
    with pytest.raises(E.LdpcError):
        E.Crc(8, 2 ** 32 + 7, n_bits=8, device=-1)                           # would wrap to a valid poly in a uint32


def test_crc_kernels_need_no_scratch():
    """the build refuses a csrc/crc.hip kernel with scratch or spills (ecc_ldpc_amd/build.py check_no_spills); here: that it looked at them"""
    from ecc_ldpc_amd import build
    objdir = os.path.join(os.path.dirname(E.SO_PATH), "build")
    res = build.crc_resources(objdir)
    assert res, f"no device assembly of csrc/crc.hip in {objdir}: build first (python ecc_ldpc_amd/build.py)"
    names = " ".join(res)
    assert "crc_attach_kernel" in names and "crc_check_kernel" in names and "crc_tally_kernel" in names and len(res) == 7
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
