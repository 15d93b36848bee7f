"""CPU: tests/bch_spec.py against the definition it restates, and the host side of the BCH code (csrc/bch.cc, the checks of
ldpc_bch_create_on in csrc/api.cc) against the spec.  Nothing here needs a device: the objects are host-only (device = -1).

  * the spec's parity lengths are the table of PARITY_LENGTHS; g divides x^N0 - 1; every encoded row has zero syndromes; g(x) and x g(x)
    are codewords;
  * the spec's decoder (Berlekamp-Massey + Chien with its acceptance rule) IS bounded-distance decoding: against a brute-force search for
    the nearest codeword over EVERY word of six small codes, shortened ones included;
  * ldpc_bch_encode_host / ldpc_bch_decode_host / ldpc_bch_generator equal the spec on the shapes the GPU tests use;
  * the refusals, each naming its argument."""
import ctypes as C
import os

import numpy as np
import pytest

import ecc_ldpc_amd as E
from tests import bch_spec as bs

EINVAL = E.EINVAL
NEW_SYMBOLS = ["ldpc_bch_create_on", "ldpc_bch_destroy", "ldpc_bch_builtin", "ldpc_bch_params", "ldpc_bch_generator", "ldpc_bch_encode_host", "ldpc_bch_decode_host",
               "ldpc_bch_encode_dev", "ldpc_bch_decode_dev", "ldpc_sim_bch_decode"]

# (prim_poly, m, t, n): the shapes of tests/test_bch_gpu.py -- the smallest at which the kernels can go wrong
SHAPES = [
    (0xB, 3, 1, 7),                           # the smallest code
    (0x13, 4, 3, 13),                         # shortened, p = 10 inside one word
    (0x11D, 8, 4, 100),                       # p = 32, exactly one word
    (0x11D, 8, 16, 255),                      # t at its cap, p = 124, unshortened
    (0x402B, 14, 12, 601),                    # p = 168: a partial sixth word, n odd
    (0x1002D, 16, 12, 700),                   # p = 192
    (0x1002D, 16, 16, 300),                   # p = 256, the widest remainder, k = 44
]
SHAPE_IDS = [f"m{m}-t{t}-n{n}" for _, m, t, n in SHAPES]
# (m, prim_poly, t, n) of the exhaustive check
TINY = [(4, 0x13, 2, 15), (4, 0x13, 3, 15), (4, 0x13, 1, 15), (4, 0x13, 2, 12), (4, 0x13, 3, 13), (5, 0x25, 2, 16)]

_codes = {}


def spec_code(poly, m, t, n):
    """the spec's code object, built once and shared (its cache of located remainders with it)"""
    key = (poly, m, t, n)
    if key not in _codes:
        _codes[key] = bs.Code(m, poly, t, n)
    return _codes[key]


def chosen_error_rows(code, seed):
    """one frame per error count e = 0 .. t + 2 -> (sent [t + 3][n] codewords, received [t + 3][n], both 0 / 1).  The error positions
    include 0, k - 1, k and n - 1 as far as e allows; the rest are drawn"""
    rng = np.random.default_rng(seed)
    n, k, t = code.n, code.k, code.t
    sent = code.encode_bytes(rng.integers(0, 2, (t + 3, n), dtype=np.uint8))
    got = sent.copy()
    must = list(dict.fromkeys([0, k - 1, k, n - 1]))
    for e in range(t + 3):
        at = must[:e]
        rest = np.setdiff1d(np.arange(n), at)
        at = at + rng.permutation(rest)[:e - len(at)].tolist()
        assert len(set(at)) == e
        got[e, np.array(at, np.int64)] ^= 1
    return sent, got


# ---- the spec against what it restates
def test_parity_lengths():
    for (poly, m, t), p in bs.PARITY_LENGTHS.items():
        N0 = 2 ** m - 1
        c = bs.Code(m, poly, t, N0)
        assert c.p == p and c.k == N0 - p, (hex(poly), m, t)
        assert bs.poly_mod((1 << N0) | 1, c.g) == 0, "g does not divide x^N0 - 1"
        assert c.g & 1 and p <= m * t
        b = E.Bch(m, poly, t, N0, device=-1)
        assert (b.p, b.k, b.n) == (p, N0 - p, N0) and b.params() == (m, poly, t, N0, N0 - p)
        assert np.array_equal(b.generator(), c.generator())
        assert E.lib().ldpc_bch_generator(b._h, None) == p                   # g may be NULL
        b.close()


def test_builtin_parameters():
    for kind, (name, m, poly, t) in bs.BUILTINS.items():
        assert E.Bch.builtin_params(kind) == (m, poly, t) == E.Bch.builtin_params(name) and E.BCH_KINDS[name] == kind
        assert (poly, m, t) in bs.PARITY_LENGTHS or (m, poly) == (16, 0x1002D)
    assert len(E.BCH_KINDS) == len(bs.BUILTINS) == 4
    L = E.lib()
    assert L.ldpc_bch_builtin(2, None, None, None) == 0                      # any pointer may be NULL
    for kind in (-1, 4, 1000):
        assert L.ldpc_bch_builtin(kind, None, None, None) == EINVAL and L.ldpc_last_error_code() == EINVAL and "kind" in E.last_error()
    b = E.Bch.builtin("m16t12", 32400, device=-1)
    assert b.params() == (16, 0x1002D, 12, 32400, 32400 - 192)
    b.close()


@pytest.mark.parametrize("poly,m,t,n", SHAPES, ids=SHAPE_IDS)
def test_encoded_rows_have_zero_syndromes(poly, m, t, n):
    c = spec_code(poly, m, t, n)
    rng = np.random.default_rng(n)
    rows = rng.integers(0, 256, (4, n), dtype=np.uint8)
    rows[1, :c.k] &= 0xFE                                                    # the zero message
    out = c.encode_bytes(rows)
    assert np.array_equal(out[:, :c.k], rows[:, :c.k]) and np.isin(out[:, c.k:], (0, 1)).all()
    assert not out[1, c.k:].any()
    for r in out:
        v = c.row_int(r)
        assert c.syndromes(v) == [0] * (2 * t) and c.is_codeword(r)
        assert c.syndromes(bs.poly_mod(v ^ 1, c.g)) == c.syndromes(v ^ 1) != [0] * (2 * t)     # a row and its remainder: the same syndromes
    packed = rng.integers(0, 256, (4, bs.row_bytes(n)), dtype=np.uint8)      # junk in the parity and pad bits
    got = c.encode_packed(packed)
    assert np.array_equal(bs.unpack(got, n)[:, :c.k], bs.unpack(packed, n)[:, :c.k])
    assert (np.unpackbits(got, axis=-1, bitorder="little")[:, n:] == 0).all()
    assert all(c.is_codeword(r) for r in bs.unpack(got, n))


@pytest.mark.parametrize("poly,m,t,n", SHAPES, ids=SHAPE_IDS)
def test_the_generator_and_its_shift_are_codewords(poly, m, t, n):
    c = spec_code(poly, m, t, n)
    for v in [c.g] + ([c.g << 1] if c.p + 1 < n else []):
        row = c.int_row(v)
        assert c.is_codeword(row) and np.array_equal(c.encode_bytes(row[None])[0], row)
        out, nerr = c.decode_bytes(row[None])
        assert nerr.tolist() == [0] and np.array_equal(out[0], row)
    assert not c.is_codeword(c.int_row(c.g ^ 1))


def _popcount16(a):
    table = np.array([bin(i).count("1") for i in range(256)], np.uint8)
    return table[a & 0xFF] + table[a >> 8]


def brute_force(code):
    """every word of n <= 16 bits -> (the nearest codeword if within t, else the word; its distance, else -1), by search"""
    n, k, p, t = code.n, code.k, code.p, code.t
    cws = np.array([(msg << p) | code.parity(msg) for msg in range(2 ** k)], np.uint32)
    assert all(bs.poly_mod(int(c), code.g) == 0 for c in cws[:64])
    words = np.arange(2 ** n, dtype=np.uint32)
    out, nerr = words.copy(), np.full(2 ** n, -1, np.int32)
    for lo in range(0, 2 ** n, 2048):
        w = words[lo:lo + 2048]
        dist = _popcount16(w[:, None] ^ cws[None, :])
        best = dist.argmin(1)
        dmin = dist[np.arange(len(w)), best]
        assert ((dist == dmin[:, None]).sum(1)[dmin <= t] == 1).all()        # within t the nearest codeword is unique
        hit = dmin <= t
        out[lo:lo + 2048][hit] = cws[best[hit]]
        nerr[lo:lo + 2048][hit] = dmin[hit]
    return out, nerr


def spec_all_words(code):
    """the spec's decoder on every word of n bits, as integers -> (words after the decode, nerr)"""
    n = code.n
    out, nerr = np.arange(2 ** n, dtype=np.uint32), np.full(2 ** n, -1, np.int32)
    for v in range(2 ** n):
        at = code.locate(bs.poly_mod(v, code.g))
        if at is not None:
            nerr[v] = len(at)
            for d in at:
                out[v] ^= np.uint32(1 << d)
    return out, nerr


@pytest.mark.parametrize("m,poly,t,n", TINY, ids=[f"m{m}-t{t}-n{n}" for m, _, t, n in TINY])
def test_the_decoder_is_bounded_distance_decoding_on_every_word(m, poly, t, n):
    c = bs.Code(m, poly, t, n)
    want, want_nerr = brute_force(c)
    got, got_nerr = spec_all_words(c)
    assert np.array_equal(got_nerr, want_nerr) and np.array_equal(got, want)
    assert (got[got_nerr < 0] == np.arange(2 ** n)[got_nerr < 0]).all()
    if (m, t, n) == (4, 3, 15):
        assert [int((got_nerr == e).sum()) for e in (0, 1, 2, 3, -1)] == [32, 480, 3360, 14560, 14336]


# ---- the library's host functions against the spec
def test_abi_symbols():
    L = C.CDLL(E.SO_PATH)
    for s in NEW_SYMBOLS:
        assert s in E.ABI_SYMBOLS and hasattr(L, s), s
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ldpc_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr, s
    assert E.lib().ldpc_abi_version() == 3


@pytest.mark.parametrize("poly,m,t,n", SHAPES, ids=SHAPE_IDS)
def test_host_functions_equal_the_spec(poly, m, t, n):
    c = spec_code(poly, m, t, n)
    b = E.Bch(m, poly, t, n, device=-1)
    assert (b.k, b.p) == (c.k, c.p) and np.array_equal(b.generator(), c.generator())
    rng = np.random.default_rng(31 * n + t)
    rows = rng.integers(0, 256, (3, n), dtype=np.uint8)
    want = c.encode_bytes(rows)
    for r, w in zip(rows, want):
        assert np.array_equal(b.encode_host(r), w)
    sent, got = chosen_error_rows(c, 7 * n + t)
    junk = got | (rng.integers(0, 128, got.shape, dtype=np.uint8) << 1).astype(np.uint8)
    want, want_nerr = c.decode_bytes(junk)
    for e in range(t + 3):
        out, nerr = b.decode_host(junk[e])
        assert nerr == want_nerr[e] and np.array_equal(out, want[e]), e
        if e <= t:
            assert nerr == e and np.array_equal(out & 1, sent[e]) and np.array_equal(out >> 1, junk[e] >> 1)
        elif nerr < 0:
            assert np.array_equal(out, junk[e])
    b.close()


def test_host_decode_on_every_word_of_a_shortened_code():
    poly, m, t, n = SHAPES[1]
    c = spec_code(poly, m, t, n)
    b = E.Bch(m, poly, t, n, device=-1)
    words = ((np.arange(2 ** n)[:, None] >> np.arange(n - 1, -1, -1)) & 1).astype(np.uint8)
    want, want_nerr = c.decode_bytes(words)
    assert (want_nerr == -1).any() and (want_nerr == t).any()
    for w, o, e in zip(words, want, want_nerr):
        out, nerr = b.decode_host(w)
        assert nerr == e and np.array_equal(out, o)
    b.close()


# ---- refusals, all before a device is needed
BAD = [
    ("m 2", (2, 0x7, 1, 3), "m"), ("m 17", (17, 0x20009, 1, 100), "m"), ("t 0", (4, 0x13, 0, 15), "t"), ("t 17", (16, 0x1002D, 17, 1000), "t"),
    ("poly of degree 3", (4, 0xB, 1, 15), "prim_poly"), ("poly of degree 5", (4, 0x25, 1, 15), "prim_poly"), ("poly 0", (4, 0, 1, 15), "prim_poly"),
    ("x^4 + x^3 + x^2 + x + 1: order 5", (4, 0x1F, 1, 15), "prim_poly"), ("x^4 + 1", (4, 0x11, 1, 15), "prim_poly"), ("x^4 + x: even", (4, 0x12, 1, 15), "prim_poly"),
    ("x^8 + x^4 + x^3 + x + 1: order 51", (8, 0x11B, 2, 255), "prim_poly"),
    ("2t = 8 >= 7", (3, 0xB, 4, 7), "t"), ("n = p", (4, 0x13, 3, 10), "n"), ("n = 0", (4, 0x13, 3, 0), "n"), ("n = -1", (4, 0x13, 3, -1), "n"),
    ("n = N0 + 1", (4, 0x13, 2, 16), "n"), ("n = 65536", (16, 0x1002D, 12, 65536), "n"),
]


@pytest.mark.parametrize("what,args,names", BAD, ids=[b[0] for b in BAD])
def test_create_refuses_before_a_device_is_needed(what, args, names):
    m, poly, t, n = args
    L = E.lib()
    for device in (-1, 0):
        assert not L.ldpc_bch_create_on(device, m, poly, t, n), what
        assert L.ldpc_last_error_code() == EINVAL and (names + " = ") in E.last_error(), (what, E.last_error())
    with pytest.raises(E.LdpcError) as e:
        E.Bch(m, poly, t, n, device=-1)
    assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        bs.Code(m, poly, t, n)


def test_host_functions_refuse_null_pointers_and_a_host_only_object_refuses_device_calls():
    L = E.lib()
    b = E.Bch(4, 0x13, 2, 15, device=-1)
    row = np.zeros(15, np.uint8)
    pr = row.ctypes.data_as(C.POINTER(C.c_uint8))
    e = C.c_int(5)
    for call, name in ((lambda: L.ldpc_bch_params(None, None, None, None, None, None), "bch"), (lambda: L.ldpc_bch_generator(None, None), "bch"),
                       (lambda: L.ldpc_bch_encode_host(None, pr), "bch"), (lambda: L.ldpc_bch_encode_host(b._h, None), "row"),
                       (lambda: L.ldpc_bch_decode_host(None, pr, C.byref(e)), "bch"), (lambda: L.ldpc_bch_decode_host(b._h, None, C.byref(e)), "row"),
                       (lambda: L.ldpc_bch_decode_host(b._h, pr, None), "nerr"),
                       (lambda: L.ldpc_bch_encode_dev(None, 1, 16, 0, None), "bch"), (lambda: L.ldpc_bch_encode_dev(b._h, 1, None, 0, None), "d_rows"),
                       (lambda: L.ldpc_bch_decode_dev(b._h, 1, 16, 0, None, None), "d_nerr"), (lambda: L.ldpc_bch_decode_dev(None, 1, 16, 0, 16, None), "bch"),
                       (lambda: L.ldpc_sim_bch_decode(None, b._h, 1, 16, 0, 16, None), "sim"),
                       (lambda: L.ldpc_bch_encode_dev(b._h, 1, 16, 0, None), "host-only"), (lambda: L.ldpc_bch_decode_dev(b._h, 1, 16, 0, 16, None), "host-only")):
        assert call() == EINVAL and L.ldpc_last_error_code() == EINVAL and name in E.last_error(), (name, E.last_error())
    assert e.value == 5 and not row.any()
    with pytest.raises(E.LdpcError):
        b.encode_host(np.zeros(14, np.uint8))
    with pytest.raises(E.LdpcError):
        E.Bch(4, 2 ** 32 + 0x13, 2, 15, device=-1)                           # would wrap to a valid polynomial in a uint32
    b.close()


def test_bch_kernels_need_no_scratch():
    """the build refuses a csrc/bch.hip kernel with scratch or spills (ecc_ldpc_amd/build.py check_no_spills); here: that it looked at them"""
    from ecc_ldpc_amd import build
    objdir = os.path.join(os.path.dirname(E.SO_PATH), "build")
    res = build.bch_resources(objdir)
    assert res, f"no device assembly of csrc/bch.hip in {objdir}: build first (python ecc_ldpc_amd/build.py)"
    names = " ".join(res)
    assert "bch_encode_kernel" in names and "bch_decode_kernel" in names and len(res) == 30      # W = 1, 2, 4, 6, 8 x {bytes, four bytes a lane, packed}
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
