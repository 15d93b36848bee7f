"""GPU: per-symbol channel state in the demapper (csrc/demap_csi.hip) and the fading channel of the frame source's modulated path
(csrc/sim_mod_fading.hip) against tests/fading_spec.py.

  1. ldpc_demap_dev_il_csi against the spec, bit for bit: the six table sizes and the six product sizes, the three formats, batch 3,
     gains random in [0.01, 8] plus a 0, a 1 and a NaN; with gains all 1 the bytes of ldpc_demap_dev_il;
  2. ldpc_sim_transmit_il_fading, block in {1, 2, 3, 5, n_sym, n_sym + 7}, K in {0, 4}: gains bitwise equal inside a block; gains and
     samples against the float64 restatement within 16 * 2^-24 units (the unit of tests/test_modulation_gpu.py carried through the gain
     rule: fading_spec.gains, fading_spec.transmit; measured on MI355X: at most 1.56 for a gain and 2.00 for a sample, DESIGN.md
     section 3.5); stream 2 untouched; replay across a batch split at first_frame = 2^32 + 5;
  3. ldpc_sim_generate_mod_il_fading = ldpc_sim_transmit_il_fading + ldpc_demap_dev_il_csi, bit for bit, all twelve objects, the three
     formats, d_gain NULL and given;
  4. refusals;
  5. the chain at the point of tests/test_fading_spec.py: per-symbol weights decode, one scale for all symbols does not.
Shapes: batch 3; N = 203 with n_tx = 187 (the last symbol has pad bits for most m; 16 punctured positions; n_sym odd for m = 1, 3, 4,
10) through a random table; n_tx = N = 120 through the block table of 120 / m rows and m columns (m divides n_tx; n_sym odd for m = 8).
Every output buffer is pre-filled and carries one guard row past the batch."""
import numpy as np
import pytest

from tests import fading_spec as fs
from tests import interleaver_spec as ils
from tests import layered_i8_spec
from tests import modulation_spec as ms
from tests import product_modulation_spec as ps
from tests.test_fading_spec import CHAIN_DB, CHAIN_FRAMES, CHAIN_SEED
from tests.test_modulation_gpu import FILL, NP_OF, TABLES, Dev, Source, _codewords, _qc_jpl1024, _same
from tests.test_product_modulation_gpu import _uneven

pytestmark = pytest.mark.gpu

B = 3
SEED, FIRST = 0x5EEDFAD1234567, 2 ** 32 - 2                      # the three frame ids cross 2^32
FMTS = (("f32", ms.LLR_F32, 0.0), ("f16", ms.LLR_F16, 0.0), ("i8", ms.LLR_I8, 2.5))
TABLE_OF_M = {1: "bpsk", 2: "qpsk", 3: "8psk", 4: "16qam", 5: "apsk32", 6: "grid64"}
OBJECTS = [("table", m) for m in range(1, 7)] + [("product", b) for b in range(1, 7)]
IDS = [f"{kind}-{n}" for kind, n in OBJECTS]


class Obj:
    """one of the twelve objects: the library's handle, m, the materialised points, and the spec's demapper for it"""

    def __init__(self, hip, kind, n):
        if kind == "table":
            self.pts = TABLES[TABLE_OF_M[n]]()
            self.m = n
            self.mod = hip.Modulation(self.pts)
            self.demap = lambda sym, a, pos, N, nv, fmt, qs: fs.demap_il_csi(self.pts, sym, a, pos, N, nv, fmt, qs)
        else:
            li, lq = _uneven(n, 60 + n), (_uneven(n, 70 + n) * np.float32(0.6)).astype(np.float32)
            self.pts = ps.materialise(li, lq)
            self.m = 2 * n
            self.mod = hip.Modulation.product(li, lq)
            self.demap = lambda sym, a, pos, N, nv, fmt, qs: fs.demap_il_csi_product(li, lq, sym, a, pos, N, nv, fmt, qs)
        assert self.mod.bits == self.m and len(self.pts) == 1 << self.m


def _shapes(m):
    """{name: (pos, N)}: the random table of 187 of 203 positions (its 16 holes scattered), the block table where m divides n_tx"""
    inj = np.random.default_rng(500 + m).permutation(203)[:187].astype(np.int32)
    assert len(ils.holes(inj, 203)) == 16 and 120 % m == 0
    return {"random187of203": (inj, 203), "block120": (ils.block_positions(120 // m, m, (np.arange(m) * 7) % (120 // m)), 120)}


def _samples(pts, ns, seed):
    rng = np.random.default_rng(seed)
    y = (pts[rng.integers(0, len(pts), B * ns)] + rng.normal(0.0, 0.2, (B * ns, 2))).astype(np.float32).reshape(B, ns, 2)
    y[2, ns - 1] = (np.nan, 0.25)                                # one NaN sample, under an ordinary gain
    return y


def _gains(ns, seed):
    a = np.random.default_rng(seed).uniform(0.01, 8.0, (B, ns)).astype(np.float32)
    a[0, 1], a[1, 0], a[1, ns - 1] = 0.0, 1.0, np.nan           # an erasure, the AWGN scale, a NaN (on the symbol with the pad bits)
    return a


@pytest.mark.parametrize("kind,n", OBJECTS, ids=IDS)
def test_demapper_csi_against_the_spec(hip, kind, n):
    o = Obj(hip, kind, n)
    d = Dev()
    nv = 0.05
    for name, (pos, N) in _shapes(o.m).items():
        n_tx = len(pos)
        ns = ms.symbols_per_frame(n_tx, o.m)
        il = hip.Interleaver(pos, N)
        sym, a = _samples(o.pts, ns, 10 * o.m + n_tx), _gains(ns, 20 * o.m + n_tx)
        sym_t, a_t, one_t = d.put(sym), d.put(a), d.put(np.ones((B, ns), np.float32))
        f32 = o.demap(sym, a, pos, N, nv, ms.LLR_F32, 4.0)
        e0, en = pos[o.m:2 * o.m], pos[(ns - 1) * o.m:n_tx]
        assert (f32[0, e0] == 0).all() and np.isnan(f32[1, en]).all() and np.isnan(f32[2, en]).any() and (f32[:, ils.holes(pos, N)] == 0).all()
        for fmt, code, qs in FMTS:
            want = o.demap(sym, a, pos, N, nv, code, qs or 4.0)
            out, ref, uni = d.full(B, N, FILL[fmt], fmt), d.full(B, N, FILL[fmt], fmt), d.full(B, N, FILL[fmt], fmt)
            d.sync()
            hip.demap_il_csi(o.mod, il, B, sym_t.data_ptr(), a_t.data_ptr(), nv, out.data_ptr(), fmt, qs, None)
            hip.demap_il_csi(o.mod, il, B, sym_t.data_ptr(), one_t.data_ptr(), nv, uni.data_ptr(), fmt, qs, None)
            hip.demap_il(o.mod, il, B, sym_t.data_ptr(), nv, ref.data_ptr(), fmt, qs, None)
            _same(d.get(out, B, FILL[fmt]), want, (kind, n, name, fmt))
            assert d.get(uni, B, FILL[fmt]).tobytes() == d.get(ref, B, FILL[fmt]).tobytes(), (kind, n, name, fmt, "gains of 1 are not ldpc_demap_dev_il")
        il.close()
    o.mod.close()


# ---- the frame source
def _source203(hip, max_batch=B, n_tx=187, generator=True):
    """a dense source of N = 203, n_tx = 187, k = 100: a random generator (the source does not look at H; 29 checks of 7 positions).
    The generator is kept as .G; generator=False: the source without one (all-zero codewords), .G = None"""
    code = hip.Code.from_csr(np.arange(0, 204, 7, dtype=np.int32), np.arange(203, dtype=np.int32), 203)
    G = np.random.default_rng(11).integers(0, 2, (100, 103)).astype(np.uint8) if generator else None
    sim = hip.Sim(code, 100, n_tx, G=G, max_batch=max_batch)
    src = Source(sim, code, 203, n_tx, (sim, code))
    src.G = G
    return src


def _source120(hip, max_batch=B):
    code = hip.Code.from_csr(np.arange(0, 121, 6, dtype=np.int32), np.arange(120, dtype=np.int32), 120)
    G = np.random.default_rng(12).integers(0, 2, (50, 70)).astype(np.uint8)
    sim = hip.Sim(code, 50, 120, G=G, max_batch=max_batch)
    src = Source(sim, code, 120, 120, (sim, code))
    src.G = G
    return src


def _source_table(src, m):
    if src.n_tx == 120:
        return ils.block_positions(120 // m, m, (np.arange(m) * 7) % (120 // m))
    return np.random.default_rng(600 + m).permutation(src.n_tx).astype(np.int32)


def _transmit(d, src, o, il, fad, first, n, db, ns, seed=SEED):
    sym, gain = d.full(n, 2 * ns, 777.0, "f32"), d.full(n, ns, 555.0, "f32")
    d.sync()
    src.sim.transmit_il_fading(o.mod, il, fad, seed, first, n, db, sym.data_ptr(), gain.data_ptr(), None, "bytes", None, None)
    return d.get(sym, n, 777.0).reshape(n, ns, 2), d.get(gain, n, 555.0), sym, gain


@pytest.mark.parametrize("kind,n", OBJECTS, ids=IDS)
def test_transmit_il_fading_against_the_restatement(hip, kind, n):
    d = Dev()
    o = Obj(hip, kind, n)
    worst_a = worst_y = 0.0
    for src in (_source203(hip), _source120(hip)):
        cw, _, _ = _codewords(d, src, B, SEED, FIRST)
        ids = np.uint64(FIRST) + np.arange(B, dtype=np.uint64)
        pos = _source_table(src, o.m)
        il = hip.Interleaver(pos, src.N)
        tx = ils.interleave(cw, pos)
        ns = o.mod.symbols(src.n_tx)
        db = 6.0
        nv = src.sim.noise_var(o.mod, db)
        for block in (1, 2, 3, 5, ns, ns + 7):
            for K in (0.0, 4.0):
                got, a, _, _ = _transmit(d, src, o, il, hip.Fading(block, K), FIRST, B, db, ns)
                q = np.arange(ns) // block
                first_of = np.flatnonzero(np.diff(q, prepend=-1))
                assert np.array_equal(a.view(np.uint32), a[:, first_of][:, q].view(np.uint32)), (block, K, "gains differ inside a block")
                assert len(np.unique(a[:, first_of])) == a[:, first_of].size and (a >= 2.0 ** -20).all()
                want_a, unit_a = fs.gains(SEED, ids, ns, block, K)
                err_a = np.abs(a.astype(np.float64) - want_a) / (2.0 ** -24 * unit_a)
                want, unit, _ = fs.transmit(o.pts, o.m, SEED, ids, tx, nv, want_a, unit_a)
                err_y = np.abs(got.astype(np.float64) - want) / (2.0 ** -24 * unit)
                worst_a, worst_y = max(worst_a, float(err_a.max())), max(worst_y, float(err_y.max()))
                assert err_a.max() <= 16.0, (src.N, block, K, float(err_a.max()))
                assert err_y.max() <= 16.0, (src.N, block, K, float(err_y.max()))
        # d_gain may be NULL: the same samples
        sym2 = d.full(B, 2 * ns, 777.0, "f32")
        d.sync()
        src.sim.transmit_il_fading(o.mod, il, hip.Fading(ns + 7, 4.0), SEED, FIRST, B, db, sym2.data_ptr(), None, None, "bytes", None, None)
        assert np.array_equal(d.get(sym2, B, 777.0).reshape(B, ns, 2).view(np.uint32), got.view(np.uint32))
        il.close()
        src.close()
    print(f"{kind}-{n}: worst gain error {worst_a:.2f}, worst sample error {worst_y:.2f} (x 2^-24 units)")
    o.mod.close()


def test_transmit_il_fading_leaves_stream_2_alone_and_replays(hip):
    """(y - c) sqrt(a) is ldpc_sim_transmit_il's y - c.  The faded sample is fl(c + fl(sg_s z)) with sg_s = fl(sg / fl(sqrt a)): half an ulp
    of each sample for the two sums, and at most 4 roundings (sqrt, divide, the two products) on the noise term"""
    d = Dev()
    o = Obj(hip, "table", 4)
    src = _source203(hip)
    ns = o.mod.symbols(src.n_tx)
    il = hip.Interleaver(_source_table(src, 4), src.N)
    first = 2 ** 32 + 5
    fad = hip.Fading(3, 0.0)
    y, a, _, _ = _transmit(d, src, o, il, fad, first, B, 6.0, ns)
    c, _, _, _ = _transmit(d, src, o, il, fad, first, B, 300.0, ns)
    awgn = d.full(B, 2 * ns, 777.0, "f32")
    d.sync()
    src.sim.transmit_il(o.mod, il, SEED, first, B, 6.0, awgn.data_ptr(), None, "bytes", None, None)
    ya = d.get(awgn, B, 777.0).reshape(B, ns, 2)
    assert np.isin(c, o.pts).all() and np.abs(a - 1.0).max() > 0.5
    y64, c64, ya64 = y.astype(np.float64), c.astype(np.float64), ya.astype(np.float64)
    ra = np.sqrt(a.astype(np.float64))[..., None]
    bound = 0.5 * ra * np.spacing(np.abs(y)) + 0.5 * np.spacing(np.abs(ya)) + 4.0 * 2.0 ** -24 * np.abs(ya64 - c64)
    err = np.abs((y64 - c64) * ra - (ya64 - c64))
    print(f"stream 2: worst |(y - c) sqrt(a) - (y_awgn - c)| / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    # replay: the batch in two calls
    y1, a1, _, _ = _transmit(d, src, o, il, fad, first, 2, 6.0, ns)
    y2, a2, _, _ = _transmit(d, src, o, il, fad, first + 2, 1, 6.0, ns)
    assert np.array_equal(np.concatenate([y1, y2]).view(np.uint32), y.view(np.uint32)) and np.array_equal(np.concatenate([a1, a2]).view(np.uint32), a.view(np.uint32))
    y3, a3, _, _ = _transmit(d, src, o, il, fad, first, B, 6.0, ns, seed=SEED + 1)
    assert not np.array_equal(a3, a)
    il.close(); o.mod.close(); src.close()


@pytest.mark.parametrize("kind,n", OBJECTS, ids=IDS)
def test_fused_fading_equals_two_step(hip, kind, n):
    d = Dev()
    o = Obj(hip, kind, n)
    db = 9.0
    for si, src in enumerate((_source203(hip), _source120(hip))):
        pos = _source_table(src, o.m)
        il = hip.Interleaver(pos, src.N)
        ns = o.mod.symbols(src.n_tx)
        nv = src.sim.noise_var(o.mod, db)
        hole = ils.holes(pos, src.N)
        for block, K in ((3, 4.0), ((1, 2, 5, ns, ns + 7, 1)[(n + si) % 6], 0.0)):
            fad = hip.Fading(block, K)
            _, a, sym_t, gain_t = _transmit(d, src, o, il, fad, FIRST, B, db, ns)
            for fmt, code, qs in FMTS:
                two, one, bare, g = d.full(B, src.N, FILL[fmt], fmt), d.full(B, src.N, FILL[fmt], fmt), d.full(B, src.N, FILL[fmt], fmt), d.full(B, ns, 555.0, "f32")
                d.sync()
                hip.demap_il_csi(o.mod, il, B, sym_t.data_ptr(), gain_t.data_ptr(), nv, two.data_ptr(), fmt, qs, None)
                src.sim.generate_mod_il_fading(o.mod, il, fad, SEED, FIRST, B, db, one.data_ptr(), fmt, qs, g.data_ptr(), None, "bytes", None, None)
                src.sim.generate_mod_il_fading(o.mod, il, fad, SEED, FIRST, B, db, bare.data_ptr(), fmt, qs, None, None, "bytes", None, None)
                t, f, nb = d.get(two, B, FILL[fmt]), d.get(one, B, FILL[fmt]), d.get(bare, B, FILL[fmt])
                _same(f, t, (kind, n, src.N, block, K, fmt))
                _same(nb, t, (kind, n, src.N, block, K, fmt, "d_gain NULL"))
                assert np.array_equal(d.get(g, B, 555.0).view(np.uint32), a.view(np.uint32)), (kind, n, src.N, block, K, fmt, "gains")
                assert (f[:, hole] == 0).all() and (fmt == "i8" or (f[:, pos] != 0).mean() > 0.9)
        il.close()
        src.close()
    o.mod.close()


def test_refusals(hip):
    import torch
    d = Dev()
    src = _source203(hip)
    o = Obj(hip, "table", 2)
    ns = o.mod.symbols(src.n_tx)
    sym, gain, llr = d.full(B, 2 * ns, 777.0, "f32"), d.full(B, ns, 777.0, "f32"), d.full(B, src.N, 777.0, "f32")
    d.sync()
    s, g, l = sym.data_ptr(), gain.data_ptr(), llr.data_ptr()
    good = hip.Interleaver(_source_table(src, 2), src.N)
    short = hip.Interleaver(np.arange(src.n_tx - 2), src.N)          # a table of other dimensions
    narrow = hip.Interleaver(np.arange(src.n_tx), src.n_tx)
    fad = hip.Fading(4, 1.0)

    def refused(fn, *a, code=-1, **kw):
        with pytest.raises(hip.LdpcError) as e:
            fn(*a, **kw)
        assert e.value.code == code, str(e.value)

    T, G = src.sim.transmit_il_fading, src.sim.generate_mod_il_fading
    bad = [hip.Fading(0), hip.Fading(-3), hip.Fading(4, -1.0), hip.Fading(4, float("nan")), hip.Fading(4, float("inf")), hip.Fading(4, 1.0, struct_size=0),
           hip.Fading(4, 1.0, struct_size=12), None]
    for f in bad:
        refused(T, o.mod, good, f, 1, 0, B, 2.0, s, g)
        refused(G, o.mod, good, f, 1, 0, B, 2.0, l)
    for il in (None, short, narrow):
        refused(T, o.mod, il, fad, 1, 0, B, 2.0, s, g)
        refused(G, o.mod, il, fad, 1, 0, B, 2.0, l)
    if torch.cuda.device_count() > 1:                                  # a table on another device
        far = hip.Interleaver(_source_table(src, 2), src.N, device=1)
        refused(T, o.mod, far, fad, 1, 0, B, 2.0, s, g)
        refused(G, o.mod, far, fad, 1, 0, B, 2.0, l)
        far.close()
    refused(T, None, good, fad, 1, 0, B, 2.0, s, g)
    refused(T, o.mod, good, fad, 1, 0, B, 2.0, None, g)
    refused(T, o.mod, good, fad, 1, 0, B, 2.0, s + 4, g)
    refused(T, o.mod, good, fad, 1, 0, B, 2.0, s, g + 2)
    refused(T, o.mod, good, fad, 1, 0, B, float("nan"), s, g)
    refused(G, o.mod, good, fad, 1, 0, B, 2.0, None)
    refused(G, o.mod, good, fad, 1, 0, B, 2.0, l + 2)
    refused(G, o.mod, good, fad, 1, 0, B, 2.0, l, "f32", 0.0, g + 1)
    refused(G, o.mod, good, fad, 1, 0, B, 400.0, l)
    refused(G, o.mod, good, fad, 1, 0, B, 2.0, l, 3)
    for batch in (0, B + 1, -1):
        refused(T, o.mod, good, fad, 1, 0, batch, 2.0, s, g)
        refused(G, o.mod, good, fad, 1, 0, batch, 2.0, l)
    # LDPC_ENCODER_NONE with the caller's messages: msg ++ zeros is no codeword
    bare = hip.Sim(src.code, 100, 187, max_batch=B)
    assert bare.encoder == "none"
    msg = d.put(np.zeros((B, 100), np.uint8))
    refused(bare.transmit_il_fading, o.mod, good, fad, 1, 0, B, 2.0, s, g, msg.data_ptr(), code=-5)
    refused(bare.generate_mod_il_fading, o.mod, good, fad, 1, 0, B, 2.0, l, "f32", 0.0, g, msg.data_ptr(), code=-5)
    # the demapper
    refused(hip.demap_il_csi, o.mod, good, B, s, None, 0.1, l)
    refused(hip.demap_il_csi, o.mod, good, B, s, g + 2, 0.1, l)
    refused(hip.demap_il_csi, o.mod, None, B, s, g, 0.1, l)
    refused(hip.demap_il_csi, o.mod, good, B, s + 4, g, 0.1, l)
    refused(hip.demap_il_csi, o.mod, good, B, s, g, 0.0, l)
    refused(hip.demap_il_csi, o.mod, good, 0, s, g, 0.1, l)
    d.sync()
    assert (sym.cpu().numpy() == 777.0).all() and (gain.cpu().numpy() == 777.0).all() and (llr.cpu().numpy() == 777.0).all()      # a refused call writes nothing
    # and the accepted forms: a struct_size of a later version, all-zero codewords with drawn messages
    T(o.mod, good, hip.Fading(4, 1.0, struct_size=64), 1, 0, B, 2.0, s, g)
    bare.generate_mod_il_fading(o.mod, good, fad, 1, 0, B, 2.0, l)
    d.sync()
    assert (d.get(gain, B, 777.0) != 777.0).all() and (d.get(llr, B, 777.0)[:, :src.n_tx] != 777.0).all()
    for x in (good, short, narrow, o.mod, bare):
        x.close()
    src.close()


def test_chain_per_symbol_weights_decode_and_one_scale_does_not(hip):
    """the point of tests/test_fading_spec.py test_chain_on_the_oracle: jpl.1024.4.5, 16QAM, the block table of 320 x 4, block = 1,
    K = 0, 64 frames, min-sum, 50 iterations.  Measured there on the oracle with these Philox draws: 0 frame errors weighted per symbol,
    40 with one scale"""
    F = CHAIN_FRAMES
    src = _qc_jpl1024(hip, F)
    d = Dev()
    torch = d.torch
    mod = hip.Modulation("16qam")
    il = hip.Interleaver.block(320, 4, N=src.N)
    fad = hip.Fading(1, 0.0)
    ns = mod.symbols(src.n_tx)
    assert ns == 320 and il.dims == (src.n_tx, src.N)
    dec = hip.Decoder(src.code, "min", "f32", F)
    llr, q8, flat = d.full(F, src.N, 777.0, "f32"), d.full(F, src.N, 99, "i8"), d.full(F, src.N, 777.0, "f32")
    sym, gain = d.full(F, 2 * ns, 777.0, "f32"), d.full(F, ns, 555.0, "f32")
    d.sync()
    errs = {}

    def decode(name, t):
        out, its = d.full(F, src.N, 9, "u8"), torch.full((F + 1,), -1, dtype=torch.int32, device=d.dev)
        back, tally = d.full(F, src.k, 9, "u8"), torch.zeros(4, dtype=torch.int64, device=d.dev)
        d.sync()
        dec.decode_batch_dev(t.data_ptr(), out.data_ptr(), F, 50, its.data_ptr(), None, None)
        dec.synchronize()
        src.sim.extract_messages(F, out.data_ptr(), back.data_ptr())
        src.sim.tally(F, out.data_ptr(), its.data_ptr(), tally.data_ptr(), None)
        d.sync()
        frames, fe, be, it = tally.cpu().numpy().tolist()
        assert frames == F and fe == int((d.get(back, F, 9) != d.get(msgs, F, 9)).any(axis=1).sum())
        print(f"{name}: {fe} frame errors of {F}, {be} bit errors, mean iterations {it / F:.1f} at {CHAIN_DB} dB")
        errs[name] = fe

    msgs = d.full(F, src.k, 9, "u8")
    src.sim.generate_mod_il_fading(mod, il, fad, CHAIN_SEED, 0, F, CHAIN_DB, q8.data_ptr(), "i8", 4.0, None, None, "bytes", None, None)
    src.sim.generate_mod_il_fading(mod, il, fad, CHAIN_SEED, 0, F, CHAIN_DB, llr.data_ptr(), "f32", 0.0, None, None, "bytes", msgs.data_ptr(), None)
    d.sync()
    l = d.get(llr, F, 777.0)
    assert np.array_equal(d.get(q8, F, 99).astype(np.int32), layered_i8_spec.quantize(l, 4.0))
    decode("per-symbol weights", llr)
    # all today's interface without channel state can say: one scale for every symbol, on the same samples
    src.sim.transmit_il_fading(mod, il, fad, CHAIN_SEED, 0, F, CHAIN_DB, sym.data_ptr(), gain.data_ptr(), None, "bytes", None, None)
    hip.demap_il(mod, il, F, sym.data_ptr(), src.sim.noise_var(mod, CHAIN_DB), flat.data_ptr(), "f32", 0.0, None)
    d.sync()
    decode("one scale", flat)
    assert errs["per-symbol weights"] <= 3
    assert errs["one scale"] >= 16
    dec.close(); il.close(); mod.close()
    src.close()
