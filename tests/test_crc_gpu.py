"""GPU: CRC attach and check on the device (csrc/crc.hip, the entry points in csrc/api.cc) against tests/crc_spec.py.  Everything is
integer arithmetic: every comparison is equality.

  1. ldpc_crc_attach_dev against the spec, bytes and packed, batches 1 and 7 (261 on one shape: 66 workgroups, the last with one live
     wave), on the shapes of tests/test_crc_spec.py SHAPES.  Payload bytes carry junk in bits 1..7 and come back unchanged; the CRC bytes
     and the packed pad bits hold junk before the call.  The bytes format runs from an aligned base and from base + 1: every k here but
     k = 7 is a multiple of 4, so only the odd base reaches the kernel that loads a byte a lane;
  2. ldpc_crc_check_dev: attached rows pass; for k <= 68 every single bit flipped in turn, one frame per position, fails; random rows give
     the spec's flag, and both outcomes for w = 1 and w = 6;
  3. ldpc_sim_crc_check = ldpc_sim_extract_messages + ldpc_crc_check_dev on a quasi-cyclic source (jpl.1024, msg_pos = 0 .. k - 1) and on
     the 40 x 90 systematic-form source (msg_pos interleaves, N = 90 is no multiple of 8), decoded bytes and packed decoded bits; and on
     the dense moon.7.13 source (k = 7 of N = 20: the four-bytes-a-lane kernel with k no multiple of 4);
  4. ldpc_sim_tally_crc: exact counts on the four kinds of frame, twice, so the counts accumulate;
  5. the launch limit: batch 70 001 (above 65 535 and 65 536);
  6. the chain on jpl.1024 min-sum; 7. refusals that need a device.
Every output is pre-filled and every buffer carries a guard row past the batch."""
import numpy as np
import pytest

from tests import crc_spec as cs
from tests import systematic_encoder_spec as sys_spec
from tests.helpers import CODES, load
from tests.test_crc_spec import SHAPE_IDS, SHAPES, random_rows

pytestmark = pytest.mark.gpu

GUARD, OKFILL = 0x5B, 7
BIG = (57, (11, 0x621, 0x155, 0x7FF))        # the shape that also runs at batch 261


class Dev:
    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)

    def put(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def rows(self, a, shift=0):
        """a [B][n] uint8 on the device with a guard row behind it -> (tensor, pointer); shift: bytes the first row starts past the base"""
        flat = np.concatenate([np.full(shift, GUARD, np.uint8), np.ascontiguousarray(a, np.uint8).reshape(-1), np.full(a.shape[1], GUARD, np.uint8)])
        t = self.put(flat)
        assert t.data_ptr() % 16 == 0
        return t, t.data_ptr() + shift

    def back(self, t, shape, shift=0):
        self.torch.cuda.synchronize()
        a = t.cpu().numpy()
        n = shape[0] * shape[1]
        assert (a[:shift] == GUARD).all() and (a[shift + n:] == GUARD).all(), "bytes outside the batch were written"
        return a[shift:shift + n].reshape(shape)

    def flags(self, B):
        return self.torch.full((B + 1,), OKFILL, dtype=self.torch.uint8, device=self.dev)

    def got_flags(self, t, B):
        self.torch.cuda.synchronize()
        a = t.cpu().numpy()
        assert a[B] == OKFILL, "a flag past the batch was written"
        assert np.isin(a[:B], (0, 1)).all(), "a flag was not written, or is not 0 or 1"
        return a[:B]


def _batches(L, params):
    return (1, 7, 261) if (L, params) == BIG else (1, 7)


def _payloads(rng, B, L, w):
    """[B][k] bytes: payload bytes with junk in bits 1..7, junk in the CRC bytes"""
    msg = rng.integers(0, 256, (B, L + w), dtype=np.uint8)
    if B > 1:
        msg[1, :L] &= 0xFE                                           # an all-zero payload: the CRC is C0
    return msg


# ---- 1. attach
@pytest.mark.parametrize("L,params", SHAPES, ids=SHAPE_IDS)
def test_attach_against_the_spec(hip, L, params):
    w, poly, init, xorout = params
    k = L + w
    d = Dev()
    crc = hip.Crc(w, poly, init, xorout, n_bits=L)
    assert crc.params() == (w, poly, init, xorout, L) and crc.k == k
    rng = np.random.default_rng(100 * L + w)
    for B in _batches(L, params):
        msg = _payloads(rng, B, L, w)
        want = cs.attach_bytes(msg, L, w, poly, init, xorout)
        assert np.array_equal(want[:, :L], msg[:, :L]) and np.isin(want[:, L:], (0, 1)).all()
        for shift in (0, 1):
            t, p = d.rows(msg, shift)
            crc.attach(B, p, "bytes")
            assert np.array_equal(d.back(t, (B, k), shift), want), (B, shift)
        rows = rng.integers(0, 256, (B, cs.row_bytes(k)), dtype=np.uint8)    # junk in the CRC bits and in the pad bits
        want = cs.attach_packed(rows, L, w, poly, init, xorout)
        assert np.array_equal(cs.unpack(want, k)[:, :L], cs.unpack(rows, k)[:, :L])
        assert (np.unpackbits(want, axis=-1, bitorder="little")[:, k:] == 0).all()
        t, p = d.rows(rows)
        crc.attach(B, p, "packed")
        assert np.array_equal(d.back(t, rows.shape), want), (B, "packed")
    crc.close()


# ---- 2. check
def _check_both(d, crc, bits, L, params, what):
    """the flags of bits [B][k] (0 / 1) through the bytes format (junk in bits 1..7, aligned and odd base) and the packed format; all
    must be the spec's.  -> flags"""
    w, poly, init, xorout = params
    B, k = bits.shape
    want = cs.check_bytes(bits, L, w, poly, init, xorout)
    junk = bits | (np.random.default_rng(B + k).integers(0, 128, bits.shape, dtype=np.uint8) << 1).astype(np.uint8)
    for shift in (0, 1):
        t, p = d.rows(junk, shift)
        ok = d.flags(B)
        crc.check(B, p, ok.data_ptr(), "bytes")
        assert np.array_equal(d.got_flags(ok, B), want), (what, "bytes", shift)
        assert np.array_equal(d.back(t, (B, k), shift), junk)               # the messages are not written
    rows = cs.pack(bits)
    if k % 32:
        rows[:, -1] |= 0x80                                              # a pad bit set: not read
    assert np.array_equal(cs.check_packed(rows, L, w, poly, init, xorout), want)
    t, p = d.rows(rows)
    ok = d.flags(B)
    crc.check(B, p, ok.data_ptr(), "packed")
    assert np.array_equal(d.got_flags(ok, B), want), (what, "packed")
    return want


@pytest.mark.parametrize("L,params", SHAPES, ids=SHAPE_IDS)
def test_check_against_the_spec(hip, L, params):
    w, poly, init, xorout = params
    k = L + w
    d = Dev()
    crc = hip.Crc(w, poly, init, xorout, n_bits=L)
    rng = np.random.default_rng(200 * L + w)
    for B in _batches(L, params):
        good = cs.attach_bytes(rng.integers(0, 2, (B, k), dtype=np.uint8), L, w, poly, init, xorout)
        assert _check_both(d, crc, good, L, params, ("attached", B)).all()
        rand = random_rows(B, L, w)
        flags = _check_both(d, crc, rand, L, params, ("random", B))
        if w <= 6:
            assert flags.any() and not flags.all()
    if k <= 68:                                                              # every single bit position in turn, one frame per position
        one = cs.attach_bytes(rng.integers(0, 2, (1, k), dtype=np.uint8), L, w, poly, init, xorout)
        flipped = np.repeat(one, k, 0) ^ np.eye(k, dtype=np.uint8)
        assert not _check_both(d, crc, flipped, L, params, "single flips").any()
    crc.close()


# ---- 3. the check straight on decoded codewords
def _qc_source(hip, B):
    c = load("jpl.1024.4.5")
    ecc = hip.ECC(CODES, "ldpc/hip-minsum/jpl.1024.4.5/50/4/5", max_batch=B)
    return ecc.sim, c.N, ecc, (ecc,)


def _systematic_source(hip, B):
    H = sys_spec.toy_40x90()
    code = hip.Code.from_csr(*sys_spec.csr(H), 90)
    sim = hip.Sim(code, None, 90, systematic=True, max_batch=B)
    return sim, 90, None, (sim, code)


def _dense_moon_source(hip, B):
    """k = 7 of N = 20: rows 4-byte aligned and no position table, so the four-bytes-a-lane kernel runs with k no multiple of 4"""
    c = load("moon.7.13")
    code = hip.Code.from_csr(c.graph.row_ptr, c.graph.col_idx, c.N)
    sim = hip.Sim(code, 7, 20, G=c.G, max_batch=B)
    return sim, 20, None, (sim, code)


SOURCES = {"qc-jpl1024": (_qc_source, 24), "systematic-40x90": (_systematic_source, 6)}
CHECK_SOURCES = dict(SOURCES, **{"dense-moon": (_dense_moon_source, 6)})


def _decoded(rng, B, N, mp, crc_params, L):
    """decoded bits [B][N] 0 / 1: even frames carry a valid CRC'd message at the message positions, odd ones are random"""
    w, poly, init, xorout = crc_params
    bits = rng.integers(0, 2, (B, N), dtype=np.uint8)
    msg = cs.attach_bytes(rng.integers(0, 2, (B, L + w), dtype=np.uint8), L, w, poly, init, xorout)
    bits[::2, mp] = msg[::2]
    return bits


@pytest.mark.parametrize("case", list(CHECK_SOURCES))
def test_sim_crc_check_equals_extract_then_check(hip, case):
    make, w = CHECK_SOURCES[case]
    B = 33
    sim, N, _, owned = make(hip, B)
    k = sim.k
    L = k - w
    params = cs.builtin("crc24a" if w == 24 else "crc6")
    mp = sim.positions()[0]
    if case.startswith("systematic"):
        assert not np.array_equal(mp, np.arange(k)) and N % 8 != 0
    else:
        assert (k, L) in ((1024, 1000), (7, 1)) and np.array_equal(mp, np.arange(k))
    d = Dev()
    crc = hip.Crc(*params, n_bits=L)
    rng = np.random.default_rng(300 + w)
    for n in (B, 7, 1):
        bits = _decoded(rng, n, N, mp, params, L)
        want = cs.check_bytes(bits[:, mp], L, *params)
        assert want[::2].all() and (n == 1 or not want.all())
        junk = bits | (rng.integers(0, 128, bits.shape, dtype=np.uint8) << 1).astype(np.uint8)     # decoded bytes: bit 0 counts
        for fmt in ("bytes", "packed"):                                      # the two-call route, through a message buffer of either format
            t, p = d.rows(junk)
            mbuf, pm = d.rows(np.full((n, k if fmt == "bytes" else cs.row_bytes(k)), 0xEE, np.uint8))
            two = d.flags(n)
            sim.extract_messages(n, p, pm, fmt)
            crc.check(n, pm, two.data_ptr(), fmt)
            assert np.array_equal(d.got_flags(two, n), want), (case, n, fmt, "two calls")
        one = d.flags(n)
        sim.crc_check(crc, n, p, one.data_ptr(), "bytes")
        assert np.array_equal(d.got_flags(one, n), want), (case, n, "bytes")
        assert np.array_equal(d.back(t, junk.shape), junk)
        PB = (N + 7) // 8
        packed = np.packbits(np.concatenate([bits, np.ones((n, 8 * PB - N), np.uint8)], 1), axis=1, bitorder="little")   # pad bits set: not read
        assert packed.shape == (n, PB)
        t, p = d.rows(packed)
        one = d.flags(n)
        sim.crc_check(crc, n, p, one.data_ptr(), "packed")
        assert np.array_equal(d.got_flags(one, n), want), (case, n, "packed")
    crc.close()
    for o in owned:
        o.close()


# ---- 4. the tally
@pytest.mark.parametrize("case", list(SOURCES))
def test_tally_crc_counts_detected_and_undetected_errors(hip, case):
    make, w = SOURCES[case]
    B = 4
    sim, N, _, owned = make(hip, B)
    k, n_tx = sim.k, sim.n_tx
    L = k - w
    params = cs.builtin("crc24a" if w == 24 else "crc6")
    mp = sim.positions()[0]
    d = Dev()
    torch = d.torch
    crc = hip.Crc(*params, n_bits=L)
    rng = np.random.default_rng(400 + w)
    payload = rng.integers(0, 2, (B + 1, k), dtype=np.uint8)
    t, p = d.rows(payload[:B])
    crc.attach(B, p, "bytes")
    msg = d.back(t, (B, k))
    assert np.array_equal(msg, cs.attach_bytes(payload[:B], L, *params))
    other = cs.attach_bytes(payload[B:], L, *params)[0]                     # another valid message
    assert not np.array_equal(other, msg[2])
    cw, pc = d.rows(np.zeros((B, n_tx), np.uint8))
    sim.encode_messages(B, p, pc, "bytes", "bytes")                          # the messages the tally compares against are now these
    bits = np.zeros((B, N), np.uint8)
    bits[:, :n_tx] = d.back(cw, (B, n_tx))
    assert np.array_equal(bits[:, mp], msg)
    bits[1, mp[L // 2]] ^= 1                                                 # one payload bit flipped: fails, in error
    bits[2, mp] = other                                                      # another valid message: passes, in error -- undetected
    outside = np.setdiff1d(np.arange(N), mp)
    bits[3, outside[:5]] ^= 1                                                # differs outside the message positions only: passes, no error
    tb, pb = d.rows(bits)
    ok = d.flags(B)
    sim.crc_check(crc, B, pb, ok.data_ptr(), "bytes")
    assert d.got_flags(ok, B).tolist() == [1, 0, 1, 1]
    tally = torch.tensor([1000, 2000, 3000, 4000, 77], dtype=torch.int64, device=d.dev)
    for rep in (1, 2):
        sim.tally_crc(B, pb, ok.data_ptr(), tally.data_ptr())
        torch.cuda.synchronize()
        assert tally.cpu().tolist() == [1000 + 4 * rep, 2000 + 3 * rep, 3000 + 2 * rep, 4000 + 1 * rep, 77]
    sim.tally_crc(3, pb, ok.data_ptr(), tally.data_ptr())                    # a shorter batch: the first three frames
    torch.cuda.synchronize()
    assert tally.cpu().tolist() == [1011, 2008, 3006, 4003, 77]
    crc.close()
    for o in owned:
        o.close()


# ---- 5. the launch limit
def test_batch_past_the_grid_limits(hip):
    """70 001 frames = 17 501 workgroups, the last with one live wave; a frame index in blockIdx.y, or a 16-bit one, would stop short"""
    L, params = SHAPES[4]
    w, poly, init, xorout = params
    k, B = L + w, 70001
    assert (L, w) == (40, 24)
    d = Dev()
    crc = hip.Crc(w, poly, init, xorout, n_bits=L)
    rng = np.random.default_rng(5)
    msg = rng.integers(0, 256, (B, k), dtype=np.uint8)
    want = cs.attach_bytes(msg, L, w, poly, init, xorout)
    t, p = d.rows(msg)
    crc.attach(B, p, "bytes")
    got = d.back(t, (B, k))
    assert np.array_equal(got, want)
    bad = rng.permutation(B)[:B // 3]
    bad = np.union1d(bad, [0, 65535, 65536, B - 1])
    want[bad, rng.integers(0, k, len(bad))] ^= 1
    flags = cs.check_bytes(want, L, w, poly, init, xorout)
    assert not flags[bad].any() and flags.sum() == B - len(bad)
    t, p = d.rows(want)
    ok = d.flags(B)
    crc.check(B, p, ok.data_ptr(), "bytes")
    assert np.array_equal(d.got_flags(ok, B), flags)
    crc.close()


# ---- 6. the chain
def test_chain_on_jpl1024_minsum(hip):
    """CRC'd messages -> ldpc_sim_generate_from -> min-sum decode -> ldpc_sim_crc_check -> ldpc_sim_tally_crc.  At 6 dB every frame decodes:
    all flags 1, no undetected error.  At 0 dB with 5 iterations nothing is asserted about the channel: every flag is the spec's on the
    bits read back"""
    B, L, w = 64, 1000, 24
    params = cs.builtin("crc24a")
    sim, N, ecc, owned = _qc_source(hip, B)
    d = Dev()
    torch = d.torch
    crc = hip.Crc.builtin("crc24a", L)
    assert crc.params() == params + (L,)
    payload = np.random.default_rng(6).integers(0, 2, (B, L + w), dtype=np.uint8)
    t, p = d.rows(payload)
    crc.attach(B, p, "bytes")
    llr = torch.full((B + 1, N), 777.0, dtype=torch.float32, device=d.dev)
    its = torch.full((B + 1,), -1, dtype=torch.int32, device=d.dev)
    for db, iters in ((6.0, 50), (0.0, 5)):
        bits, pb = d.rows(np.full((B, N), 9, np.uint8))
        torch.cuda.synchronize()
        sim.generate_from(0xC4C, 11, B, db, p, llr.data_ptr(), "bytes", None)
        torch.cuda.synchronize()                                             # the context decodes on its own stream
        ecc.decoder.decode_batch_dev(llr.data_ptr(), pb, B, iters, its.data_ptr(), None, None)
        ecc.decoder.synchronize()
        ok = d.flags(B)
        tally = torch.zeros(4, dtype=torch.int64, device=d.dev)
        sim.crc_check(crc, B, pb, ok.data_ptr(), "bytes")
        sim.tally_crc(B, pb, ok.data_ptr(), tally.data_ptr())
        flags = d.got_flags(ok, B)
        decoded = d.back(bits, (B, N))
        msg = d.back(t, (B, L + w))
        want = cs.check_bytes(decoded[:, :L + w], L, *params)
        assert np.array_equal(flags, want), db
        wrong = (decoded[:, :L + w] != msg).any(1)
        assert tally.cpu().tolist() == [B, int(want.sum()), int(wrong.sum()), int((wrong & (want == 1)).sum())], db
        if db == 6.0:
            assert flags.all() and not wrong.any()
    crc.close()
    for o in owned:
        o.close()


# ---- 7. refusals that need a device
def test_refusals_that_need_a_device(hip):
    B = 4
    sim, N, _, owned = _qc_source(hip, B)
    d = Dev()
    crc = hip.Crc.builtin("crc24a", 1000)
    short = hip.Crc.builtin("crc24a", 999)                                   # L + w = 1023, the source's k is 1024
    bits, pb = d.rows(np.zeros((B, N), np.uint8))
    msg, pm = d.rows(np.zeros((B, 1024), np.uint8))
    ok = d.flags(B)
    tally = d.torch.zeros(4, dtype=d.torch.int64, device=d.dev)

    def refused(fn, *a):
        with pytest.raises(hip.LdpcError) as e:
            fn(*a)
        assert e.value.code == hip.EINVAL
        return str(e.value)

    assert "999 + 24" in refused(sim.crc_check, short, B, pb, ok.data_ptr())
    refused(sim.crc_check, crc, B, pb, None)                                 # a NULL d_ok
    refused(crc.check, B, pm, None)
    refused(sim.crc_check, crc, B, None, ok.data_ptr())
    refused(sim.crc_check, None, B, pb, ok.data_ptr())
    for batch in (0, -1):
        refused(sim.crc_check, crc, batch, pb, ok.data_ptr())
        refused(crc.check, batch, pm, ok.data_ptr())
        refused(crc.attach, batch, pm)
        refused(sim.tally_crc, batch, pb, ok.data_ptr(), tally.data_ptr())
    refused(sim.tally_crc, B + 1, pb, ok.data_ptr(), tally.data_ptr())       # above the source's max_batch: its stored messages end there
    refused(sim.tally_crc, B, pb, None, tally.data_ptr())
    refused(crc.check, 2 ** 22, pm, ok.data_ptr())                           # batch * k = 2^32 > 2^32 - 256
    for fmt in (2, -1):
        refused(crc.attach, B, pm, fmt)
        refused(crc.check, B, pm, ok.data_ptr(), fmt)
        refused(sim.crc_check, crc, B, pb, ok.data_ptr(), fmt)
    refused(crc.attach, B, pm + 1, "packed")                                 # packed rows are whole aligned words
    refused(crc.check, B, pm + 2, ok.data_ptr(), "packed")
    d.torch.cuda.synchronize()
    assert (ok.cpu().numpy() == OKFILL).all() and (tally.cpu().numpy() == 0).all()          # a refused call writes nothing
    assert (d.back(msg, (B, 1024)) == 0).all() and (d.back(bits, (B, N)) == 0).all()
    crc.close(); short.close()
    for o in owned:
        o.close()
