"""GPU: BCH encode and bounded-distance decode on the device (csrc/bch.hip, the entry points in csrc/api.cc) against tests/bch_spec.py.
Everything is integer arithmetic: every comparison is equality.

  1. ldpc_bch_encode_dev against the spec on tests/test_bch_spec.py SHAPES, batches 1 and 7 (261 on one shape: 66 workgroups, the last
     with one live wave).  Bytes rows carry junk in bits 1..7 and run from an aligned base and from base + 1 (n = 100, 300 and 700 are
     multiples of 4: only the odd base reaches their byte-a-lane kernel); packed rows carry junk in the parity and pad bits;
  2. ldpc_bch_decode_dev on EVERY word of (0x13, 4, 3, 15) and of its shortening to 13, one batch each, bytes and packed: all of nerr =
     0, 1, 2, 3 and -1 occur, and a failed row comes back as it was;
  3. chosen errors: on each shape one frame per error count e = 0 .. t + 2, positions 0, k - 1, k and n - 1 among them;
  4. the full length once: (0x1002D, 16, 12, 32 400), a clean row, 12 errors with both ends among them, 13 errors;
  5. ldpc_sim_bch_decode = extract, spec, scatter, on a quasi-cyclic source (jpl.1024, msg_pos = 0 .. k - 1) and on the 40 x 90
     systematic-form source (msg_pos interleaves, N = 90 is no multiple of 8), decoded bytes and packed decoded bits;
  6. the launch limit: batch 70 001; 7. the chain on jpl.1024 min-sum; 8. refusals that need a device.
Every output is pre-filled and every buffer carries a guard row past the batch."""
import numpy as np
import pytest

from tests import bch_spec as bs
from tests.test_bch_spec import SHAPE_IDS, SHAPES, chosen_error_rows, spec_code
from tests.test_crc_gpu import Dev, _qc_source, _systematic_source

pytestmark = pytest.mark.gpu

NERRFILL = -77
BIG = (0x11D, 8, 4, 100)                     # the shape that also runs at batch 261


def _nerr(d, B):
    return d.torch.full((B + 1,), NERRFILL, dtype=d.torch.int32, device=d.dev)


def _got_nerr(d, t, B):
    d.torch.cuda.synchronize()
    a = t.cpu().numpy()
    assert a[B] == NERRFILL, "a count past the batch was written"
    assert (a[:B] != NERRFILL).all(), "a count was not written"
    return a[:B]


def _junk(bits, seed):
    """bits 0 / 1 -> bytes with junk in bits 1..7"""
    return bits | (np.random.default_rng(seed).integers(0, 128, bits.shape, dtype=np.uint8) << 1).astype(np.uint8)


def _pad_junk(rows, n):
    """packed rows with every pad bit (>= n) set"""
    out = rows.copy()
    bits = np.unpackbits(out, axis=-1, bitorder="little")
    bits[:, n:] = 1
    return np.packbits(bits, axis=-1, bitorder="little")


# ---- 1. encode
@pytest.mark.parametrize("poly,m,t,n", SHAPES, ids=SHAPE_IDS)
def test_encode_against_the_spec(hip, poly, m, t, n):
    c = spec_code(poly, m, t, n)
    d = Dev()
    bch = hip.Bch(m, poly, t, n)
    assert bch.params() == (m, poly, t, n, c.k) and (bch.k, bch.p) == (c.k, c.p)
    rng = np.random.default_rng(100 * n + t)
    for B in (1, 7, 261) if (poly, m, t, n) == BIG else (1, 7):
        rows = rng.integers(0, 256, (B, n), dtype=np.uint8)
        if B > 1:
            rows[1, :c.k] &= 0xFE                                            # the zero message: zero parity
        want = c.encode_bytes(rows)
        for shift in (0, 1):
            tr, p = d.rows(rows, shift)
            bch.encode(B, p, "bytes")
            assert np.array_equal(d.back(tr, (B, n), shift), want), (B, shift)
        packed = rng.integers(0, 256, (B, bs.row_bytes(n)), dtype=np.uint8)  # junk in the parity bits and in the pad bits
        want = c.encode_packed(packed)
        tr, p = d.rows(packed)
        bch.encode(B, p, "packed")
        assert np.array_equal(d.back(tr, packed.shape), want), (B, "packed")
    bch.close()


# ---- 2, 3, 4. decode
def _decode_both(d, bch, c, bits, what):
    """bits [B][n] 0 / 1 through the bytes format (junk in bits 1..7, aligned and odd base) and the packed format (pad bits set): rows and
    counts must be the spec's.  -> (rows after the decode, 0 / 1; nerr)"""
    B, n = bits.shape
    junk = _junk(bits, B + n)
    want, want_nerr = c.decode_bytes(junk)
    assert np.array_equal(want >> 1, junk >> 1)
    for shift in (0, 1):
        tr, p = d.rows(junk, shift)
        ne = _nerr(d, B)
        bch.decode(B, p, ne.data_ptr(), "bytes")
        assert np.array_equal(_got_nerr(d, ne, B), want_nerr), (what, "bytes", shift)
        assert np.array_equal(d.back(tr, (B, n), shift), want), (what, "bytes", shift)
    rows = _pad_junk(bs.pack(bits), n)
    wantp, wantp_nerr = c.decode_packed(rows)
    assert np.array_equal(wantp_nerr, want_nerr) and np.array_equal(bs.unpack(wantp, n), want & 1)
    tr, p = d.rows(rows)
    ne = _nerr(d, B)
    bch.decode(B, p, ne.data_ptr(), "packed")
    assert np.array_equal(_got_nerr(d, ne, B), want_nerr), (what, "packed")
    assert np.array_equal(d.back(tr, rows.shape), wantp), (what, "packed")
    return want & 1, want_nerr


@pytest.mark.parametrize("n", (15, 13))
def test_decode_every_word(hip, n):
    poly, m, t = 0x13, 4, 3
    c = spec_code(poly, m, t, n)
    d = Dev()
    bch = hip.Bch(m, poly, t, n)
    words = ((np.arange(2 ** n)[:, None] >> np.arange(n - 1, -1, -1)) & 1).astype(np.uint8)
    out, nerr = _decode_both(d, bch, c, words, n)
    if n == 15:
        assert [int((nerr == e).sum()) for e in (0, 1, 2, 3, -1)] == [32, 480, 3360, 14560, 14336]
    assert all((nerr == e).any() for e in (0, 1, 2, 3, -1))
    assert np.array_equal(out[nerr < 0], words[nerr < 0])                    # a failure is left as it was
    assert ((out != words).sum(1)[nerr >= 0] == nerr[nerr >= 0]).all()
    bch.close()


@pytest.mark.parametrize("poly,m,t,n", SHAPES, ids=SHAPE_IDS)
def test_decode_chosen_errors(hip, poly, m, t, n):
    c = spec_code(poly, m, t, n)
    d = Dev()
    bch = hip.Bch(m, poly, t, n)
    sent, got = chosen_error_rows(c, 7 * n + t)
    out, nerr = _decode_both(d, bch, c, got, (m, t, n))
    assert nerr[:t + 1].tolist() == list(range(t + 1)) and np.array_equal(out[:t + 1], sent[:t + 1])
    bch.close()


def test_decode_at_full_length(hip):
    poly, m, t, n = 0x1002D, 16, 12, 32400
    c = spec_code(poly, m, t, n)
    d = Dev()
    bch = hip.Bch.builtin("m16t12", n)
    assert bch.params() == (m, poly, t, n, n - 192)
    rng = np.random.default_rng(4)
    msg = rng.integers(0, 2, (3, n), dtype=np.uint8)
    tr, p = d.rows(msg)
    bch.encode(3, p, "bytes")
    sent = d.back(tr, (3, n))
    assert np.array_equal(sent, c.encode_bytes(msg))
    got = sent.copy()
    got[1, np.concatenate([[0, n - 1], 1 + rng.permutation(n - 2)[:10]])] ^= 1
    got[2, rng.permutation(n)[:13]] ^= 1
    out, nerr = _decode_both(d, bch, c, got, "full length")
    assert nerr[:2].tolist() == [0, 12] and np.array_equal(out[:2], sent[:2])
    bch.close()


# ---- 5. the decode straight on decoded codewords
SOURCES = {"qc-jpl1024": (_qc_source, (11, 0x805, 4)), "systematic-40x90": (_systematic_source, (6, 0x43, 3))}


@pytest.mark.parametrize("case", list(SOURCES))
def test_sim_bch_decode_equals_extract_spec_scatter(hip, case):
    make, (m, poly, t) = SOURCES[case]
    B = 33
    sim, N, _, owned = make(hip, B)
    n = sim.k
    mp = sim.positions()[0]
    if case.startswith("systematic"):
        assert not np.array_equal(mp, np.arange(n)) and N % 8 != 0 and n < 64
    else:
        assert n == 1024 and np.array_equal(mp, np.arange(n))
    c = spec_code(poly, m, t, n)
    d = Dev()
    bch = hip.Bch(m, poly, t, n)
    rng = np.random.default_rng(500 + m)
    for nb in (B, 1):
        bits = rng.integers(0, 2, (nb, N), dtype=np.uint8)
        cw = c.encode_bytes(rng.integers(0, 2, (nb, n), dtype=np.uint8))
        for f in range(nb):                                                  # frame f carries f mod (t + 3) errors at message positions
            cw[f, rng.permutation(n)[:f % (t + 3)]] ^= 1
        bits[:, mp] = cw
        junk = _junk(bits, nb)
        fixed, want_nerr = c.decode_bytes(junk[:, mp])
        assert want_nerr[:t + 1].tolist() == list(range(min(nb, t + 1)))
        want = junk.copy()
        want[:, mp] = fixed
        assert ((want != junk).sum(1) == np.maximum(want_nerr, 0)).all()
        tr, p = d.rows(junk)
        ne = _nerr(d, nb)
        sim.bch_decode(bch, nb, p, ne.data_ptr(), "bytes")
        assert np.array_equal(_got_nerr(d, ne, nb), want_nerr), (case, nb, "bytes")
        assert np.array_equal(d.back(tr, junk.shape), want), (case, nb, "bytes")
        PB = (N + 7) // 8
        packed = np.packbits(np.concatenate([bits, np.ones((nb, 8 * PB - N), np.uint8)], 1), axis=1, bitorder="little")   # pad bits set: kept
        wantp = np.packbits(np.concatenate([want & 1, np.ones((nb, 8 * PB - N), np.uint8)], 1), axis=1, bitorder="little")
        tr, p = d.rows(packed)
        ne = _nerr(d, nb)
        sim.bch_decode(bch, nb, p, ne.data_ptr(), "packed")
        assert np.array_equal(_got_nerr(d, ne, nb), want_nerr), (case, nb, "packed")
        assert np.array_equal(d.back(tr, packed.shape), wantp), (case, nb, "packed")
    bch.close()
    for o in owned:
        o.close()


# ---- 6. the launch limit
def test_batch_past_the_grid_limits(hip):
    """70 001 frames = 17 501 workgroups, the last with one live wave; a frame index in blockIdx.y, or a 16-bit one, would stop short"""
    poly, m, t, n, B = 0x13, 4, 3, 15, 70001
    c = spec_code(poly, m, t, n)
    d = Dev()
    bch = hip.Bch(m, poly, t, n)
    rows = np.random.default_rng(6).integers(0, 256, (B, n), dtype=np.uint8)
    want, want_nerr = c.decode_bytes(rows)
    assert all((want_nerr == e).any() for e in (0, 1, 2, 3, -1))
    tr, p = d.rows(rows)
    ne = _nerr(d, B)
    bch.decode(B, p, ne.data_ptr(), "bytes")
    assert np.array_equal(_got_nerr(d, ne, B), want_nerr)
    assert np.array_equal(d.back(tr, (B, n)), want)
    want = c.encode_bytes(rows[:, :n])
    tr, p = d.rows(rows)
    bch.encode(B, p, "bytes")
    assert np.array_equal(d.back(tr, (B, n)), want)
    bch.close()


# ---- 7. the chain
def test_chain_on_jpl1024_minsum(hip):
    """payload -> ldpc_bch_encode_dev -> ldpc_sim_generate_from -> min-sum decode (6 dB: every frame decodes) -> f mod (t + 3) message bits
    of decoded frame f flipped -> ldpc_sim_bch_decode -> ldpc_sim_extract_messages"""
    B, m, poly, t = 64, 11, 0x805, 4
    sim, N, ecc, owned = _qc_source(hip, B)
    n = sim.k
    c = spec_code(poly, m, t, n)
    assert (n, c.p) == (1024, 44)
    d = Dev()
    torch = d.torch
    bch = hip.Bch(m, poly, t, n)
    rng = np.random.default_rng(7)
    payload = rng.integers(0, 2, (B, n), dtype=np.uint8)
    tm, pm = d.rows(payload)
    bch.encode(B, pm, "bytes")
    msg = d.back(tm, (B, n))
    assert np.array_equal(msg, c.encode_bytes(payload))
    llr = torch.full((B + 1, N), 777.0, dtype=torch.float32, device=d.dev)
    its = torch.full((B + 1,), -1, dtype=torch.int32, device=d.dev)
    bits, pb = d.rows(np.full((B, N), 9, np.uint8))
    torch.cuda.synchronize()
    sim.generate_from(0xC4C, 11, B, 6.0, pm, llr.data_ptr(), "bytes", None)
    torch.cuda.synchronize()                                                 # the context decodes on its own stream
    ecc.decoder.decode_batch_dev(llr.data_ptr(), pb, B, 50, its.data_ptr(), None, None)
    ecc.decoder.synchronize()
    decoded = d.back(bits, (B, N)).copy()
    assert np.array_equal(decoded[:, :n], msg), "a frame did not decode at 6 dB"
    for f in range(B):
        decoded[f, rng.permutation(n)[:f % (t + 3)]] ^= 1
    fixed, want_nerr = c.decode_bytes(decoded[:, :n])
    few = (np.arange(B) % (t + 3)) <= t
    assert np.array_equal(want_nerr[few], (np.arange(B) % (t + 3))[few]) and np.array_equal(fixed[few], msg[few])
    bits, pb = d.rows(decoded)
    ne = _nerr(d, B)
    out, po = d.rows(np.full((B, n), 0xEE, np.uint8))
    sim.bch_decode(bch, B, pb, ne.data_ptr(), "bytes")
    sim.extract_messages(B, pb, po, "bytes")
    nerr = _got_nerr(d, ne, B)
    got = d.back(out, (B, n))
    assert np.array_equal(nerr, want_nerr) and np.array_equal(got, fixed)
    assert np.array_equal(got[few], msg[few]) and np.array_equal(got[few, :c.k], payload[few, :c.k])
    assert np.array_equal(d.back(bits, (B, N))[:, n:], decoded[:, n:])       # the LDPC parity bits are not touched
    bch.close()
    for o in owned:
        o.close()


# ---- 8. refusals that need a device
def test_refusals_that_need_a_device(hip):
    B = 4
    sim, N, _, owned = _qc_source(hip, B)
    d = Dev()
    bch = hip.Bch(11, 0x805, 4, 1024)
    short = hip.Bch(11, 0x805, 4, 1023)                                      # the source's messages have 1024 bits
    hostonly = hip.Bch(11, 0x805, 4, 1024, device=-1)
    bits, pb = d.rows(np.zeros((B, N), np.uint8))
    rows, pr = d.rows(np.ones((B, 1024), np.uint8))
    ne = _nerr(d, B)

    def refused(fn, *a):
        with pytest.raises(hip.LdpcError) as e:
            fn(*a)
        assert e.value.code == hip.EINVAL
        return str(e.value)

    assert "n = 1023" in refused(sim.bch_decode, short, B, pb, ne.data_ptr())
    assert "device" in refused(sim.bch_decode, hostonly, B, pb, ne.data_ptr())
    assert "host-only" in refused(hostonly.decode, B, pr, ne.data_ptr())
    assert "d_nerr" in refused(sim.bch_decode, bch, B, pb, None)
    assert "d_nerr" in refused(bch.decode, B, pr, None)
    assert "d_bits" in refused(sim.bch_decode, bch, B, None, ne.data_ptr())
    assert "d_rows" in refused(bch.encode, B, None)
    refused(sim.bch_decode, None, B, pb, ne.data_ptr())
    for batch in (0, -1):
        assert "batch" in refused(sim.bch_decode, bch, batch, pb, ne.data_ptr())
        assert "batch" in refused(bch.decode, batch, pr, ne.data_ptr())
        assert "batch" in refused(bch.encode, batch, pr)
    assert "batch" in refused(bch.decode, 2 ** 22, pr, ne.data_ptr())        # batch * n = 2^32 > 2^32 - 256
    assert "batch" in refused(bch.encode, 2 ** 22, pr)
    for fmt in (2, -1):
        assert "fmt" in refused(bch.encode, B, pr, fmt)
        assert "fmt" in refused(bch.decode, B, pr, ne.data_ptr(), fmt)
        assert "fmt" in refused(sim.bch_decode, bch, B, pb, ne.data_ptr(), fmt)
    refused(bch.encode, B, pr + 1, "packed")                                 # packed rows are whole aligned words
    refused(bch.decode, B, pr + 2, ne.data_ptr(), "packed")
    d.torch.cuda.synchronize()
    assert (ne.cpu().numpy() == NERRFILL).all()                              # a refused call writes nothing
    assert (d.back(rows, (B, 1024)) == 1).all() and (d.back(bits, (B, N)) == 0).all()
    bch.close(); short.close(); hostonly.close()
    for o in owned:
        o.close()
