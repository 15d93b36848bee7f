"""GPU: rate matching and HARQ soft combining (csrc/demap_rm.hip, csrc/ratematch.cc, the entry points in csrc/api.cc) against
tests/ratematch_spec.py.

  1. ldpc_demap_dev_rm against the spec, bit for bit, with and without gains: table objects m = 1..6 and product objects b = 3 and 6, the
     three formats, batches 1 and 7, N = 96 through five tables -- random injective (E = 79), random with repeats (E = 97), circular with
     E = 2 N + 5 (fan-in 2 and 3) and E = 3 N, and ten positions named twenty times each (E = 200).  79, 97 and 197 are prime, so every
     m > 1 has pad bits in the last symbol there; 288 and 200 have them for the m that do not divide them.  One more: N = 1000,
     E = 2005, batch 3, so a frame spans several workgroups and a workgroup two frames.  On every shape the two-call route
     (ldpc_demap_dev into float32, then ldpc_ratematch_llr_dev) gives the same bits, and the injective table those of
     ldpc_demap_dev_il / ldpc_demap_dev_il_csi (NaNs are compared by mask, as everywhere in these tests);
  2. accumulate = 1 over three rounds through three different tables; what no round sends keeps its sentinel;
  3. special values: a NaN sample, a NaN gain, a zero gain, and sums that saturate fp16 and int8 where no single LLR does;
  4. ldpc_ratematch_bits_dev in the four byte / packed combinations; ldpc_sim_transmit_rm against the float64 restatement within the
     16 * 2^-24 units of tests/test_fading_gpu.py test_transmit_il_fading_against_the_restatement; a second round on the first one's
     messages;
  5. refusals that need a device;
  6. the chain of tests/test_ratematch_spec.py on the device.
Every output buffer is pre-filled and carries one guard row past the batch."""
import numpy as np
import pytest

from tests import fading_spec as fs
from tests import interleaver_spec as ils
from tests import modulation_spec as ms
from tests import product_modulation_spec as ps
from tests import ratematch_spec as rs
from tests.test_fading_gpu import _source203
from tests.test_modulation_gpu import FILL, NP_OF, TABLES, Dev, _codewords, _qc_jpl1024, _same
from tests.test_product_modulation_gpu import _uneven
from tests.test_ratematch_spec import CHAIN_DB, CHAIN_FRAMES, CHAIN_K, CHAIN_ROUNDS, CHAIN_SEED

pytestmark = pytest.mark.gpu

N = 96
SEED, FIRST = 0x5EED4A5251AB, 2 ** 32 - 2                       # the frame ids cross 2^32
FMTS = (("f32", ms.LLR_F32, 0.0), ("f16", ms.LLR_F16, 0.0), ("i8", ms.LLR_I8, 2.5))
TABLE_OF_M = {1: "bpsk", 2: "qpsk", 3: "8psk", 4: "16qam", 5: "apsk32", 6: "grid64"}
OBJECTS = [("table", m) for m in range(1, 7)] + [("product", 3), ("product", 6)]
IDS = [f"{kind}-{n}" for kind, n in OBJECTS]


class Obj:
    """one of the eight objects: the library's handle, m, the materialised points, and the spec's LLRs of the transmitted bits"""

    def __init__(self, hip, kind, n):
        if kind == "table":
            self.pts = TABLES[TABLE_OF_M[n]]()
            self.m = n
            self.mod = hip.Modulation(self.pts)
            self.bit_llrs = lambda sym, E, nv, a=None: rs.bit_llrs(self.pts, sym, E, nv, a)
        else:
            li, lq = _uneven(n, 60 + n), (_uneven(n, 70 + n) * np.float32(0.6)).astype(np.float32)
            self.pts = ps.materialise(li, lq)
            self.m = 2 * n
            self.mod = hip.Modulation.product(li, lq)
            self.bit_llrs = lambda sym, E, nv, a=None: rs.bit_llrs_product(li, lq, sym, E, nv, a)
        assert self.mod.bits == self.m and len(self.pts) == 1 << self.m


def _tables(seed=0):
    """{name: pos} over N = 96"""
    rng = np.random.default_rng(900 + seed)
    ten = rng.permutation(N)[:10]
    t = {"injective79": rng.permutation(N)[:79], "repeats97": rng.integers(0, N, 97), "circular2N+5": rs.circular_positions(N, 17, 2 * N + 5),
         "circular3N": rs.circular_positions(N, 95, 3 * N, rng.permutation(N)), "ten-by-twenty": rng.permutation(np.repeat(ten, 20))}
    t = {k: np.ascontiguousarray(v, np.int32) for k, v in t.items()}
    fan = rs.fanin(t["circular2N+5"], N)
    assert sorted(set(fan.tolist())) == [2, 3] and len(set(t["repeats97"].tolist())) < 97 and (rs.fanin(t["circular3N"], N) == 3).all()
    assert sorted(rs.fanin(t["ten-by-twenty"], N).tolist()) == [0] * 86 + [20] * 10
    return t


def _samples(pts, B, ns, seed):
    """[B][ns][2] float32: a point plus N(0, 0.3^2); a few samples of magnitude up to 1e4 (LLRs beyond fp16 and int8) and one NaN sample"""
    rng = np.random.default_rng(seed)
    n = B * ns
    y = (pts[rng.integers(0, len(pts), n)] + rng.normal(0.0, 0.3, (n, 2))).astype(np.float32)
    y[rng.permutation(n)[:3]] = rng.uniform(-1e4, 1e4, (3, 2)).astype(np.float32)
    y[n - 2] = (np.nan, 0.25)
    return y.reshape(B, ns, 2)


def _gains(B, ns, seed):
    a = np.random.default_rng(seed).uniform(0.01, 8.0, (B, ns)).astype(np.float32)
    a[0, 1], a[B - 1, 0], a[B - 1, ns - 1] = 0.0, 1.0, np.nan   # an erasure, the AWGN scale, a NaN (on the symbol with the pad bits)
    return a


def _buffer(d, init, fmt):
    """a device buffer holding init [B][n] plus a guard row of FILL"""
    guard = np.full((1, init.shape[1]), FILL[fmt], NP_OF[fmt])
    return d.put(np.concatenate([init.astype(NP_OF[fmt]), guard]))


def _run_shape(hip, d, o, name, pos, n_pos, B, counts):
    E = len(pos)
    ns = ms.symbols_per_frame(E, o.m)
    nv = 0.05
    rm = hip.Ratematch(pos, n_pos)
    assert rm.dims == (E, n_pos) and np.array_equal(rm.positions, pos) and np.array_equal(rm.fanin, rs.fanin(pos, n_pos)) and rm.fanin.sum() == E
    injective = len(set(pos.tolist())) == E
    il = hip.Interleaver(pos, n_pos) if injective else None
    sym, a = _samples(o.pts, B, ns, 31 * o.m + E + B), _gains(B, ns, 37 * o.m + E + B)
    sym_t, a_t = d.put(sym), d.put(a)
    tx_t = d.full(B, E, 555.0, "f32")
    d.sync()
    hip.demap(o.mod, B, E, E, sym_t.data_ptr(), nv, tx_t.data_ptr(), "f32", 0.0, None)
    for gain, gain_t in ((None, None), (a, a_t)):
        v, sent = rs.position_sums(o.bit_llrs(sym, E, nv, gain), pos, n_pos)
        assert np.isnan(v).any() and sent.sum() == len(set(pos.tolist()))
        for fmt, code, qs in FMTS:
            want = rs.combine(v, sent, code, qs or 4.0)
            out = d.full(B, n_pos, FILL[fmt], fmt)
            d.sync()
            hip.demap_rm(o.mod, rm, B, sym_t.data_ptr(), None if gain is None else gain_t.data_ptr(), nv, out.data_ptr(), fmt, qs, False, None)
            got = d.get(out, B, FILL[fmt])
            _same(got, want, (name, B, fmt, "gains" if gain is not None else "no gains"))
            counts["fused"] += 1
            if gain is None:                                   # the two-call route: ldpc_demap_dev, then the table alone
                two = d.full(B, n_pos, FILL[fmt], fmt)
                d.sync()
                hip.ratematch_llr(rm, B, tx_t.data_ptr(), two.data_ptr(), fmt, qs, False, None)
                _same(d.get(two, B, FILL[fmt]), got, (name, B, fmt, "two calls"))
            if injective:                                      # the interleaver's scatter kernels
                ref = d.full(B, n_pos, FILL[fmt], fmt)
                d.sync()
                if gain is None:
                    hip.demap_il(o.mod, il, B, sym_t.data_ptr(), nv, ref.data_ptr(), fmt, qs, None)
                else:
                    hip.demap_il_csi(o.mod, il, B, sym_t.data_ptr(), gain_t.data_ptr(), nv, ref.data_ptr(), fmt, qs, None)
                _same(got, d.get(ref, B, FILL[fmt]), (name, B, fmt, "the interleaver's kernel"))
                counts["injective"] += 1
    rm.close()
    if il is not None:
        il.close()


@pytest.mark.parametrize("kind,n", OBJECTS, ids=IDS)
def test_demap_rm_against_the_spec(hip, kind, n):
    d = Dev()
    o = Obj(hip, kind, n)
    counts = {"fused": 0, "injective": 0}
    for name, pos in _tables().items():
        assert o.m == 1 or name in ("circular3N", "ten-by-twenty") or len(pos) % o.m != 0
        for B in (1, 7):
            _run_shape(hip, d, o, name, pos, N, B, counts)
    big = rs.circular_positions(1000, 123, 2005, np.random.default_rng(4).permutation(1000))
    _run_shape(hip, d, o, "N1000", big, 1000, 3, counts)
    assert counts["fused"] == 66 and counts["injective"] == 12
    o.mod.close()


@pytest.mark.parametrize("kind,n", OBJECTS, ids=IDS)
def test_harq_three_rounds_through_three_tables(hip, kind, n):
    """accumulate = 1 in every round, onto a buffer of known values: positions 80 .. 95 are sent by no round"""
    d = Dev()
    o = Obj(hip, kind, n)
    B, nv = 3, 0.05
    rng = np.random.default_rng(70 + o.m)
    ten = rng.permutation(60)[:10]
    tables = [rng.integers(0, 60, 43).astype(np.int32), rs.circular_positions(N, 50, 30), rng.permutation(np.repeat(ten, 20)).astype(np.int32)]
    never = np.arange(80, N)
    assert all(p.max() < 80 for p in tables)
    start = {"f32": rng.normal(0.0, 5.0, (B, N)).astype(np.float32), "i8": rng.integers(-127, 128, (B, N)).astype(np.int8)}
    start["f16"] = start["f32"].astype(np.float16)
    for fmt in start:
        start[fmt][:, never] = FILL[fmt]                       # the sentinel
    for fmt, code, qs in FMTS:
        soft = start[fmt].copy()
        buf = _buffer(d, soft, fmt)
        for r, pos in enumerate(tables):
            E = len(pos)
            ns = ms.symbols_per_frame(E, o.m)
            rm = hip.Ratematch(pos, N)
            sym = _samples(o.pts, B, ns, 100 * r + o.m)
            a = _gains(B, ns, 200 * r + o.m) if r == 1 else None        # the second round with channel state
            sym_t = d.put(sym)
            a_t = None if a is None else d.put(a)
            soft = rs.ratematch_llr(o.bit_llrs(sym, E, nv, a), pos, N, code, qs or 4.0, old=soft)
            hip.demap_rm(o.mod, rm, B, sym_t.data_ptr(), None if a is None else a_t.data_ptr(), nv, buf.data_ptr(), fmt, qs, True, None)
            got = d.get(buf, B, FILL[fmt])
            _same(got, soft, (kind, n, fmt, "round", r))
            assert (got[:, never] == FILL[fmt]).all()
            if fmt == "i8":
                assert (np.abs(got.astype(np.int32)) == 127).any()
            rm.close()
        assert (got[:, :80] != start[fmt][:, :80]).any()
    o.mod.close()


def test_special_values(hip):
    """16QAM, N = 12.  Position 0 is named by the first bit of eight symbols that all hold the sample (1500, 0.3): each LLR lies
    between 1e4 and 65504 in magnitude, inside fp16 and, at the qscale chosen below, inside int8; their sum is outside both.  Position 1: a NaN sample.  Position 2: a NaN
    gain.  Position 3: a zero gain.  Position 4: two ordinary bits.  The rest is not sent"""
    d = Dev()
    pts = TABLES["16qam"]()
    mod = hip.Modulation(pts)
    m, ns, n_pos, B = 4, 12, 12, 2
    E = m * ns
    pos = np.full(E, 5, np.int32)                              # everything else lands on position 5 ..
    pos[0:32:4] = 0
    pos[4 * 8], pos[4 * 9 + 1], pos[4 * 10 + 2], pos[4 * 11], pos[4 * 11 + 3] = 1, 2, 3, 4, 4
    pos[pos == 5] = np.resize(np.arange(5, 9), (pos == 5).sum())   # .. to 8: positions 9 .. 11 stay unsent
    sym = np.tile(np.array([1500.0, 0.3], np.float32), (B, ns, 1))
    sym[:, 8:] = (pts[[3, 7, 9, 12]] + np.float32(0.1)).astype(np.float32)
    sym[:, 8, 0] = np.nan
    a = np.ones((B, ns), np.float32)
    a[:, 9], a[:, 10] = np.nan, 0.0
    nv = 0.05
    tx = rs.bit_llrs(pts, sym, E, nv, a)
    v, sent = rs.position_sums(tx, pos, n_pos)
    single = tx[0, 0]
    qs = float(np.float32(64.0) / abs(single))                 # one LLR quantises to +-64, eight of them clip
    sign = np.sign(single)
    assert 1e4 < abs(single) < 65504 and abs(single) * qs < 127 and abs(v[0, 0]) > 65504 and v[0, 0] == np.float32(8) * single
    assert np.isnan(v[0, 1]) and np.isnan(v[0, 2]) and v[0, 3] == 0 and np.isfinite(v[0, 4]) and v[0, 4] != 0 and not sent[9:].any()
    rm = hip.Ratematch(pos, n_pos)
    sym_t, a_t = d.put(sym), d.put(a)
    old = {"f32": np.full((B, n_pos), 3.0, np.float32), "f16": np.full((B, n_pos), 3.0, np.float16), "i8": np.full((B, n_pos), 3, np.int8)}
    for fmt, code, _ in FMTS:
        want0, want1 = rs.combine(v, sent, code, qs), rs.combine(v, sent, code, qs, old=old[fmt])
        out0, out1 = d.full(B, n_pos, FILL[fmt], fmt), _buffer(d, old[fmt], fmt)
        d.sync()
        hip.demap_rm(mod, rm, B, sym_t.data_ptr(), a_t.data_ptr(), nv, out0.data_ptr(), fmt, qs, False, None)
        hip.demap_rm(mod, rm, B, sym_t.data_ptr(), a_t.data_ptr(), nv, out1.data_ptr(), fmt, qs, True, None)
        got0, got1 = d.get(out0, B, FILL[fmt]), d.get(out1, B, FILL[fmt])
        _same(got0, want0, (fmt, "accumulate 0"))
        _same(got1, want1, (fmt, "accumulate 1"))
        sat = {"f32": np.float32(8) * single, "f16": np.float16(sign * 65504.0), "i8": int(sign) * 127}[fmt]
        assert got0[0, 0] == sat and (got0[:, 9:] == 0).all() and (got1[:, 9:] == 3).all()
        assert got1[0, 0] == (sat + np.float32(3.0) if fmt == "f32" else sat)
        if fmt == "i8":
            assert (got0[:, 1:4] == 0).all() and (got1[:, 1:4] == 3).all()                 # NaN -> 0; NaN keeps the buffer; a zero gain adds 0
        else:
            assert np.isnan(got0[:, 1:3].astype(np.float32)).all() and np.isnan(got1[:, 1:3].astype(np.float32)).all() and (got0[:, 3] == 0).all() and (got1[:, 3] == 3).all()
    rm.close(); mod.close()


# ---- the transmit side
def test_ratematch_bits_in_the_four_formats(hip):
    d = Dev()
    B = 5
    pos = _tables(1)["repeats97"]
    rm = hip.Ratematch(pos, N)
    cw = np.random.default_rng(6).integers(0, 2, (B, N)).astype(np.uint8)
    want = rs.ratematch_bits(cw, pos)
    assert want.shape == (B, 97) and 97 % 8 != 0
    ins = {"bytes": d.put(cw), "packed": d.put(ils.pack(cw))}
    for cf, src in ins.items():
        for tf, w in (("bytes", want), ("packed", ils.pack(want))):
            out = d.full(B, w.shape[1], 0xEE, "u8")
            d.sync()
            hip.ratematch_bits(rm, B, src.data_ptr(), out.data_ptr(), cf, tf, None)
            assert np.array_equal(d.get(out, B, 0xEE), w), (cf, tf)
    rm.close()


def _rm_table(src, o):
    """a circular read of the source's transmitted prefix for 2 n_tx + 5 bits, through a shuffled buffer"""
    buf = np.random.default_rng(800 + o.m).permutation(src.n_tx).astype(np.int32)
    return rs.circular_positions(src.n_tx, 11, 2 * src.n_tx + 5, buf)


@pytest.mark.parametrize("kind,n", OBJECTS, ids=IDS)
def test_transmit_rm_against_the_restatement(hip, kind, n):
    d = Dev()
    o = Obj(hip, kind, n)
    B = 3
    src = _source203(hip)
    cw, _, _ = _codewords(d, src, B, SEED, FIRST)
    ids = np.uint64(FIRST) + np.arange(B, dtype=np.uint64)
    pos = _rm_table(src, o)
    E = len(pos)
    rm = hip.Ratematch(pos, src.N)
    full = np.zeros((B, src.N), np.uint8)
    full[:, :src.n_tx] = cw
    tx = rs.ratematch_bits(full, pos)
    ns = o.mod.symbols(E)
    db = 6.0
    nv = src.sim.noise_var_rm(o.mod, rm, db)
    assert abs(nv / rs.noise_var(src.k, E, o.pts, db) - 1.0) < 1e-12 and abs(nv * src.n_tx / (src.sim.noise_var(o.mod, db) * E) - 1.0) < 1e-12
    worst_a = worst_y = 0.0
    for fad, block, K in ((None, ns, 0.0), (hip.Fading(ns, 0.0), ns, 0.0), (hip.Fading(5, 4.0), 5, 4.0)):
        sym, gain = d.full(B, 2 * ns, 777.0, "f32"), d.full(B, ns, 555.0, "f32")
        d.sync()
        src.sim.transmit_rm(o.mod, rm, fad, SEED, FIRST, B, db, sym.data_ptr(), gain.data_ptr(), None, "bytes", None, None)
        got, a = d.get(sym, B, 777.0).reshape(B, ns, 2), d.get(gain, B, 555.0)
        if fad is None:
            assert (a == 555.0).all()                          # AWGN: no gains are written
            want, unit, _ = fs.transmit(o.pts, o.m, SEED, ids, tx, nv, np.ones((B, ns)))
        else:
            want_a, unit_a = fs.gains(SEED, ids, ns, block, K)
            err_a = np.abs(a.astype(np.float64) - want_a) / (2.0 ** -24 * unit_a)
            worst_a = max(worst_a, float(err_a.max()))
            assert err_a.max() <= 16.0, (block, K, float(err_a.max()))
            want, unit, _ = fs.transmit(o.pts, o.m, SEED, ids, tx, nv, want_a, unit_a)
        err_y = np.abs(got.astype(np.float64) - want) / (2.0 ** -24 * unit)
        worst_y = max(worst_y, float(err_y.max()))
        assert err_y.max() <= 16.0, (block, K, float(err_y.max()))
    print(f"{kind}-{n}: worst gain error {worst_a:.2f}, worst sample error {worst_y:.2f} (x 2^-24 units)")
    rm.close(); o.mod.close(); src.close()


def test_second_round_carries_the_same_messages_and_other_noise(hip):
    d = Dev()
    o = Obj(hip, "table", 4)
    B = 3
    src = _source203(hip)
    pos = _rm_table(src, o)
    rm = hip.Ratematch(pos, src.N)
    ns = o.mod.symbols(len(pos))
    fad = hip.Fading(ns, 2.0)

    def send(seed, db, msg_in):
        sym, gain, msg = d.full(B, 2 * ns, 777.0, "f32"), d.full(B, ns, 555.0, "f32"), d.full(B, src.k, 9, "u8")
        d.sync()
        src.sim.transmit_rm(o.mod, rm, fad, seed, FIRST, B, db, sym.data_ptr(), gain.data_ptr(), None if msg_in is None else msg_in.data_ptr(), "bytes", msg.data_ptr(), None)
        return d.get(sym, B, 777.0).reshape(B, ns, 2), d.get(gain, B, 555.0), d.get(msg, B, 9), msg

    y1, a1, m1, m1_t = send(SEED, 6.0, None)
    y2, a2, m2, _ = send(SEED + 1, 6.0, m1_t)
    c1, _, _, _ = send(SEED, 300.0, None)
    c2, _, _, _ = send(SEED + 1, 300.0, m1_t)
    _, _, other, _ = send(SEED + 1, 6.0, None)
    assert np.array_equal(m1, m2) and not np.array_equal(m1, other)              # the caller's messages, not those of the new seed
    assert np.array_equal(c1, c2) and np.isin(c1, o.pts).all()                  # the same codewords: at 300 dB the samples are the points
    assert (y1 != y2).mean() > 0.99 and (a1 != a2).all()                        # fresh noise and fresh gains
    rm.close(); o.mod.close(); src.close()


def test_refusals(hip):
    import torch
    d = Dev()
    src = _source203(hip)
    o = Obj(hip, "table", 2)
    B = 3
    good = hip.Ratematch(_rm_table(src, o), src.N)
    ns = o.mod.symbols(good.E)
    sym, gain, llr = d.full(B, 2 * ns, 777.0, "f32"), d.full(B, ns, 777.0, "f32"), d.full(B, src.N, 777.0, "f32")
    tx = d.full(B, good.E, 777.0, "f32")
    d.sync()
    s, g, l, t = sym.data_ptr(), gain.data_ptr(), llr.data_ptr(), tx.data_ptr()
    beyond = hip.Ratematch(np.array([0, 5, src.n_tx, 5], np.int32), src.N)       # a position the source's codewords do not hold
    narrow = hip.Ratematch(np.arange(40, dtype=np.int32), src.n_tx)               # another N than the code's
    fad = hip.Fading(4, 1.0)

    def refused(fn, *a, code=-1, **kw):
        with pytest.raises(hip.LdpcError) as e:
            fn(*a, **kw)
        assert e.value.code == code, str(e.value)

    T = src.sim.transmit_rm
    for rm in (None, beyond, narrow):
        refused(T, o.mod, rm, fad, 1, 0, B, 2.0, s, g)
        refused(T, o.mod, rm, None, 1, 0, B, 2.0, s, None)
    for f in (hip.Fading(0), hip.Fading(4, -1.0), hip.Fading(4, 1.0, struct_size=0)):
        refused(T, o.mod, good, f, 1, 0, B, 2.0, s, g)
    refused(T, None, good, fad, 1, 0, B, 2.0, s, g)
    refused(T, o.mod, good, fad, 1, 0, B, 2.0, None, g)
    refused(T, o.mod, good, fad, 1, 0, B, 2.0, s + 4, g)                          # misaligned samples, gains
    refused(T, o.mod, good, fad, 1, 0, B, 2.0, s, g + 2)
    refused(T, o.mod, good, fad, 1, 0, B, float("nan"), s, g)
    for batch in (0, B + 1, -1):
        refused(T, o.mod, good, fad, 1, 0, batch, 2.0, s, g)
    refused(hip.demap_rm, o.mod, good, B, s + 4, None, 0.1, l)
    refused(hip.demap_rm, o.mod, good, B, s, g + 2, 0.1, l)
    refused(hip.demap_rm, o.mod, good, B, s, None, 0.1, l + 2)
    refused(hip.demap_rm, o.mod, good, B, s, None, 0.1, l + 1, "f16")
    refused(hip.demap_rm, o.mod, good, B, s, None, 0.1, l, "f32", 0.0, 2)
    refused(hip.ratematch_llr, good, B, t + 2, l)
    refused(hip.ratematch_llr, good, B, t, l + 2)
    if torch.cuda.device_count() > 1:                                             # a table on another device
        far = hip.Ratematch(good.positions, src.N, device=1)
        refused(T, o.mod, far, fad, 1, 0, B, 2.0, s, g)
        refused(hip.demap_rm, o.mod, far, B, s, None, 0.1, l)
        refused(hip.ratematch_llr, far, B, t, l)
        refused(hip.ratematch_bits, far, B, s, l)
        far.close()
    d.sync()
    for x in (sym, gain, llr, tx):
        assert (x.cpu().numpy() == 777.0).all()                                   # a refused call writes nothing
    T(o.mod, good, None, 1, 0, B, 2.0, s, None)                                   # and the accepted form
    d.sync()
    assert (d.get(sym, B, 777.0) != 777.0).all()
    for x in (good, beyond, narrow, o.mod):
        x.close()
    src.close()


def test_chain_two_chase_rounds_against_one(hip):
    """the scenario of tests/test_ratematch_spec.py test_chain_on_the_oracle through device encode, transmit, demap-and-combine and
    decode: the same constants, the same two inequalities.  Measured on MI355X: 46 frame errors of 64 after the first round, 0 after
    the two rounds combined (the oracle on the restatement's samples: 47 and 0)"""
    F = CHAIN_FRAMES
    src = _qc_jpl1024(hip, F)
    d = Dev()
    torch = d.torch
    mod = hip.Modulation("16qam")
    rm = hip.Ratematch.circular(src.N, 0, src.n_tx, n_buf=src.n_tx)
    ns = mod.symbols(rm.E)
    assert ns == 320 and rm.dims == (1280, 1408)
    fad = hip.Fading(ns, CHAIN_K)
    dec = hip.Decoder(src.code, "min", "f32", F)
    soft, sym, gain = d.full(F, src.N, 777.0, "f32"), d.full(F, 2 * ns, 777.0, "f32"), d.full(F, ns, 555.0, "f32")
    msgs = d.full(F, src.k, 9, "u8")
    nv = src.sim.noise_var_rm(mod, rm, CHAIN_DB)
    errs = []
    for r in range(CHAIN_ROUNDS):
        back = d.full(F, src.k, 9, "u8")
        d.sync()
        src.sim.transmit_rm(mod, rm, fad, CHAIN_SEED + r, 0, F, CHAIN_DB, sym.data_ptr(), gain.data_ptr(), None if r == 0 else msgs.data_ptr(), "bytes",
                            msgs.data_ptr() if r == 0 else back.data_ptr(), None)
        hip.demap_rm(mod, rm, F, sym.data_ptr(), gain.data_ptr(), nv, soft.data_ptr(), "f32", 0.0, r > 0, None)
        d.sync()
        assert r == 0 or np.array_equal(d.get(back, F, 9), d.get(msgs, F, 9))
        out, its = d.full(F, src.N, 9, "u8"), torch.full((F + 1,), -1, dtype=torch.int32, device=d.dev)
        got, tally = d.full(F, src.k, 9, "u8"), torch.zeros(4, dtype=torch.int64, device=d.dev)
        d.sync()
        dec.decode_batch_dev(soft.data_ptr(), out.data_ptr(), F, 50, its.data_ptr(), None, None)
        dec.synchronize()
        src.sim.extract_messages(F, out.data_ptr(), got.data_ptr())
        src.sim.tally(F, out.data_ptr(), its.data_ptr(), tally.data_ptr(), None)
        d.sync()
        frames, fe, be, it = tally.cpu().numpy().tolist()
        assert frames == F and fe == int((d.get(got, F, 9) != d.get(msgs, F, 9)).any(axis=1).sum())
        print(f"after round {r + 1}: {fe} frame errors of {F}, {be} bit errors, mean iterations {it / F:.1f} at {CHAIN_DB} dB")
        errs.append(fe)
    assert (d.get(soft, F, 777.0)[:, src.n_tx:] == 0).all()                       # the tail is never sent: round 1 cleared it, round 2 left it
    assert errs[0] / F >= 0.5
    assert errs[-1] / F <= 0.1
    dec.close(); rm.close(); mod.close()
    src.close()
