"""GPU: product constellations up to 4096-QAM -- the per-axis device demapper (csrc/demap_product.hip) and the frame source's modulated
path (csrc/sim_mod_product.hip) against tests/product_modulation_spec.py.

  1. ldpc_demap_dev on a product object against the spec, bit for bit (float32 as uint32, NaNs by mask): b = 1..6, two different
     non-uniform level sets, batch 3 and 70, (n_tx, N) of moon.7.13 (13: at m = 12 the second symbol carries one bit and eleven pads),
     jpl.1024.4.5 (a punctured tail, N > n_tx, N % m != 0 for m = 6, 10, 12) and 1920.1280.3.303 (1920: N % m == 0 for every m, the
     vector stores), the three formats, rows at an aligned pointer and one element past it; samples with a NaN in I only, in Q only,
     +-inf, a coordinate on a level and midway between two;
  2. ldpc_sim_transmit with a b <= 3 product object = ldpc_sim_transmit with the same constellation as a table, bit for bit;
  3. ldpc_sim_transmit for b = 4, 5, 6 (the built-ins 256QAM, 1024QAM, 4096QAM) against the float64 restatement, within
     16 * 2^-24 * (|c| + sg * radius) per coordinate (the unit and bar of tests/test_modulation_gpu.py; measured on MI355X: at most 2.45);
  4. ldpc_sim_generate_mod = ldpc_demap_dev(ldpc_sim_transmit), bit for bit, one source per encoder, b = 4 and 6, float32 and int8;
  5. the chain at 50 dB, 256QAM and 4096QAM on 1920.1280.3.303: the signs are the codeword, the f32 and the LDPC_I8 decoder converge in 0
     iterations, ldpc_sim_extract_messages returns the caller's messages;
  6. refusals through the entry points, as for table objects.
Every output buffer carries one guard row past the batch, which must stay untouched."""
import numpy as np
import pytest

from tests import dvbs2_short
from tests import modulation_spec as ms
from tests import product_modulation_spec as ps
from tests.helpers import load
from tests.test_modulation_gpu import FILL, FIRST, NP_OF, SEED, Dev, _codewords, _dense_moon, _qc_jpl1024, _same, _sparse, _systematic

pytestmark = pytest.mark.gpu

BUILTIN = {3: "64qam", 4: "256qam", 5: "1024qam", 6: "4096qam"}


def _uneven(b, seed):
    """a non-uniform level set [2^b], labels shuffled, no two levels equal"""
    rng = np.random.default_rng(seed)
    lev = np.sort(rng.uniform(-1.5, 1.5, 1 << b)) + np.arange(1 << b) * 0.05
    return rng.permutation(lev).astype(np.float32)


def _samples(li, lq, B, ns, seed):
    """[B][ns][2] float32: a point plus N(0, 0.1^2); then, from the front and as far as they fit: NaN in I only, NaN in Q only, +-inf, a
    block of magnitudes up to 1e3, every level of either axis with the other coordinate off its levels, the midpoints of neighbouring
    levels"""
    rng = np.random.default_rng(seed)
    n = B * ns
    y = np.stack([li[rng.integers(0, len(li), n)], lq[rng.integers(0, len(lq), n)]], axis=1) + rng.normal(0.0, 0.1, (n, 2))
    y = y.astype(np.float32)
    sp = [np.array([[np.nan, 0.25], [0.25, np.nan], [np.inf, 0.1], [0.1, -np.inf], [-np.inf, np.inf], [0.0, -0.0]], np.float32),
          rng.uniform(-1e3, 1e3, (8, 2)).astype(np.float32)]
    for ax, lev in ((0, li), (1, lq)):
        s = np.sort(lev)
        for vals in (lev, ((s[1:] + s[:-1]) * np.float32(0.5)).astype(np.float32)):
            blk = np.full((len(vals), 2), np.float32(0.123), np.float32)
            blk[:, ax] = vals
            sp.append(blk)
    sp = np.concatenate(sp)[:n]
    y[:len(sp)] = sp
    return y.reshape(B, ns, 2)


def _shapes():
    j = load("jpl.1024.4.5")
    assert j.n_tx < j.N
    return ((13, 13), (j.n_tx, j.N), (1920, 1920))


@pytest.mark.parametrize("b", [1, 2, 3, 4, 5, 6])
def test_demapper_against_the_spec(hip, b):
    m = 2 * b
    li, lq = _uneven(b, 60 + b), (_uneven(b, 70 + b) * np.float32(0.6)).astype(np.float32)
    mod = hip.Modulation.product(li, lq)
    assert mod.bits == m
    d = Dev()
    torch = d.torch
    launches, aligned_rows, ragged_rows = 0, False, False
    for B in (3, 70):
        for n_tx, N in _shapes():
            ns = ms.symbols_per_frame(n_tx, m)
            assert mod.symbols(n_tx) == ns
            sym = _samples(li, lq, B, ns, 1000 * m + n_tx + B)
            sym_t = d.put(sym)
            aligned_rows |= N % m == 0
            ragged_rows |= N % m != 0
            for nv in (0.02, 1e-3):                      # 1e-3 with the 1e3 block: fp16 saturates, int8 clips
                f32 = ps.demap(li, lq, sym, n_tx, N, nv)
                wants = {("f32", 0.0): f32, ("f16", 0.0): ms.round_f16(f32), ("i8", 4.0): ps.demap(li, lq, sym, n_tx, N, nv, ps.LLR_I8, 4.0),
                         ("i8", 2.5): ps.demap(li, lq, sym, n_tx, N, nv, ps.LLR_I8, 2.5)}
                if B * ns >= 4:
                    per = ps.symbol_llrs(li, lq, sym, nv).reshape(B * ns, m)
                    nan = np.isnan(per)                  # a NaN coordinate stays on its axis
                    assert nan[0, :b].all() and not nan[0, b:].any() and nan[1, b:].all() and not nan[1, :b].any() and nan[2, :b].all() and nan[3, b:].all()
                for (fmt, qs), want in wants.items():
                    item = np.dtype(NP_OF[fmt]).itemsize
                    # rows at an aligned pointer
                    out = d.full(B, N, FILL[fmt], fmt)
                    d.sync()
                    hip.demap(mod, B, n_tx, N, sym_t.data_ptr(), nv, out.data_ptr(), fmt, qs, None)
                    _same(d.get(out, B, FILL[fmt]), want, (b, B, n_tx, N, nv, fmt, qs, "aligned"))
                    # and one element past it: no vector store may be used
                    flat = torch.full(((B + 1) * N + 1,), FILL[fmt], dtype=d.dt[fmt], device=d.dev)
                    assert flat.data_ptr() % 16 == 0
                    d.sync()
                    hip.demap(mod, B, n_tx, N, sym_t.data_ptr(), nv, flat.data_ptr() + item, fmt, qs, None)
                    d.sync()
                    fl = flat.cpu().numpy()
                    assert fl[0] == FILL[fmt] and (fl[1 + B * N:] == FILL[fmt]).all(), "written outside the rows"
                    _same(fl[1:1 + B * N].reshape(B, N), want, (b, B, n_tx, N, nv, fmt, qs, "shifted"))
                    launches += 2
    assert aligned_rows and (ragged_rows or b == 1)
    print(f"b={b}: m={m}, {launches} launches")
    mod.close()


SOURCES = {
    "dense-moon-ntx13": lambda hip, B: _dense_moon(hip, B, 13),
    "qc-jpl1024": _qc_jpl1024,
    "sparse-dvbs2-short": lambda hip, B: _sparse(hip, B, *dvbs2_short.csr(), dvbs2_short.N),
    "systematic-1920": lambda hip, B: _systematic(hip, B, "1920.1280.3.303"),
}
BMAX = 70


@pytest.mark.parametrize("case", ["dense-moon-ntx13", "qc-jpl1024", "systematic-1920"])
def test_transmit_equals_the_table_object(hip, case):
    src = SOURCES[case](hip, BMAX)
    d = Dev()
    for b in (1, 2, 3):
        li, lq = _uneven(b, 80 + b), _uneven(b, 90 + b)
        prod, tab = hip.Modulation.product(li, lq), hip.Modulation(ps.materialise(li, lq))
        assert prod.bits == tab.bits == 2 * b and prod.energy == tab.energy
        ns = prod.symbols(src.n_tx)
        for B in (3, BMAX):
            _, msg, msg_t = _codewords(d, src, B)
            for db, msg_in in ((3.0, None), (7.5, msg_t.data_ptr())):
                got = []
                for mod in (prod, tab):
                    sym = d.full(B, 2 * ns, 777.0, "f32")
                    d.sync()
                    src.sim.transmit(mod, SEED, FIRST, B, db, sym.data_ptr(), msg_in, "bytes", None, None)
                    got.append(d.get(sym, B, 777.0))
                assert src.sim.noise_var(prod, db) == src.sim.noise_var(tab, db)
                assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)), (case, b, B, db)
        prod.close(); tab.close()
    src.close()


@pytest.mark.parametrize("case", ["dense-moon-ntx13", "qc-jpl1024", "systematic-1920"])
def test_transmit_against_the_restatement(hip, case):
    src = SOURCES[case](hip, BMAX)
    d = Dev()
    worst = 0.0
    for B, seed, first in ((3, SEED, FIRST), (BMAX, 2 ** 63 + 12345, 2 ** 40 + 2 ** 32 - 5)):    # seeds and frame ids past 2^32
        cw, msg, _ = _codewords(d, src, B, seed, first)
        ids = np.uint64(first) + np.arange(B, dtype=np.uint64)
        for b in (4, 5, 6):
            mod = hip.Modulation(BUILTIN[b])
            lev = ps.builtin_levels(2 * b)
            ns = mod.symbols(src.n_tx)
            for db in (12.0, 300.0):
                sym, mg = d.full(B, 2 * ns, 777.0, "f32"), d.full(B, src.k, 9, "u8")
                d.sync()
                src.sim.transmit(mod, seed, first, B, db, sym.data_ptr(), None, "bytes", mg.data_ptr(), None)
                got = d.get(sym, B, 777.0).reshape(B, ns, 2)
                assert np.array_equal(d.get(mg, B, 9), msg)
                want, unit, sg, nv = ps.transmit(lev, lev, seed, ids, cw, src.k, db)
                assert nv == src.sim.noise_var(mod, db) == ps.noise_var(src.k, src.n_tx, lev, lev, db)
                if db == 300.0:                          # sg ~ 1e-15, no level is 0: the symbols are the constellation points
                    c = ps.materialise(lev, lev)[ms.labels(cw, 2 * b)]
                    assert (np.abs(c) > 1e-3).all() and sg < 2e-15
                    assert np.array_equal(got.view(np.uint32), c.view(np.uint32)), (case, b, "300 dB")
                    continue
                err = np.abs(got.astype(np.float64) - want) / (2.0 ** -24 * unit)
                worst = max(worst, float(err.max()))
                assert err.max() <= 16.0, (case, b, float(err.max()))
            mod.close()
    print(f"{case}: worst symbol error = {worst:.2f} x 2^-24 (|c| + sg radius)")
    src.close()


@pytest.mark.parametrize("case", list(SOURCES))
def test_fused_equals_two_step(hip, case):
    B = 33
    src = SOURCES[case](hip, B)
    d = Dev()
    cw, msg, msg_t = _codewords(d, src, B)
    for b in (4, 6):
        mod = hip.Modulation(BUILTIN[b])
        ns = mod.symbols(src.n_tx)
        for fmt, qs in (("f32", 0.0), ("i8", 4.0)):
            for db, msg_in in ((12.0, None), (50.0, msg_t.data_ptr())):
                sym, two, one = d.full(B, 2 * ns, 777.0, "f32"), d.full(B, src.N, FILL[fmt], fmt), d.full(B, src.N, FILL[fmt], fmt)
                mg = d.full(B, src.k, 9, "u8")
                d.sync()
                src.sim.transmit(mod, SEED, FIRST, B, db, sym.data_ptr(), msg_in, "bytes", None, None)
                hip.demap(mod, B, src.n_tx, src.N, sym.data_ptr(), src.sim.noise_var(mod, db), two.data_ptr(), fmt, qs, None)
                src.sim.generate_mod(mod, SEED, FIRST, B, db, one.data_ptr(), fmt, qs, msg_in, "bytes", None if msg_in else mg.data_ptr(), None)
                a, f = d.get(two, B, FILL[fmt]), d.get(one, B, FILL[fmt])
                d.get(sym, B, 777.0)
                _same(f, a, (case, b, fmt, db))
                assert (f[:, src.n_tx:] == 0).all() and (msg_in or np.array_equal(d.get(mg, B, 9), msg))
                assert fmt == "i8" or (f[:, :src.n_tx] != 0).mean() > 0.9         # (at 12 dB the low bits of 4096-QAM quantise to 0)
                if db == 50.0:                           # far below half the minimum distance: the signs are the codeword
                    assert np.array_equal((f[:, :src.n_tx] > 0).astype(np.uint8), cw), (case, b, fmt, "50 dB")
        mod.close()
    # the instances of the fused kernel the loop above leaves out (b = 1, 2, 3, 5 in every format, fp16 of b = 4, 6): the two steps, bit for bit
    for b in range(1, 7):
        mod = hip.Modulation.product(_uneven(b, 80 + b), _uneven(b, 90 + b))
        ns = mod.symbols(src.n_tx)
        for fmt, qs in (("f16", 0.0),) if b in (4, 6) else (("f32", 0.0), ("f16", 0.0), ("i8", 4.0)):
            sym, two, one = d.full(B, 2 * ns, 777.0, "f32"), d.full(B, src.N, FILL[fmt], fmt), d.full(B, src.N, FILL[fmt], fmt)
            d.sync()
            src.sim.transmit(mod, SEED, FIRST, B, 12.0, sym.data_ptr(), None, "bytes", None, None)
            hip.demap(mod, B, src.n_tx, src.N, sym.data_ptr(), src.sim.noise_var(mod, 12.0), two.data_ptr(), fmt, qs, None)
            src.sim.generate_mod(mod, SEED, FIRST, B, 12.0, one.data_ptr(), fmt, qs, None, "bytes", None, None)
            a, f = d.get(two, B, FILL[fmt]), d.get(one, B, FILL[fmt])
            d.get(sym, B, 777.0)
            _same(f, a, (case, b, fmt, "every instance"))
            assert (f[:, src.n_tx:] == 0).all()
        mod.close()
    src.close()


@pytest.mark.parametrize("name", ["256qam", "4096qam"])
def test_chain_noiseless_frames_need_no_iteration(hip, name):
    B = 33
    src = _systematic(hip, B, "1920.1280.3.303")
    d = Dev()
    torch = d.torch
    mod = hip.Modulation(name)
    msg = np.random.default_rng(7).integers(0, 2, (B + 1, src.k)).astype(np.uint8)       # the caller's messages
    msg_t = d.put(msg)
    cw_t = d.full(B, src.n_tx, 7, "u8")
    d.sync()
    src.sim.encode_messages(B, msg_t.data_ptr(), cw_t.data_ptr())
    cw = d.get(cw_t, B, 7)
    for kind, fmt, qs in (("f32", "f32", 0.0), ("i8", "i8", 4.0)):
        dec = hip.Decoder(src.code, "min", kind, B, schedule="layered", **({"qscale": qs} if kind == "i8" else {}))
        llr = d.full(B, src.N, FILL[fmt], fmt)
        out, its, conv = d.full(B, src.N, 9, "u8"), torch.full((B + 1,), -1, dtype=torch.int32, device=d.dev), torch.full((B + 1,), 9, dtype=torch.uint8, device=d.dev)
        back = d.full(B, src.k, 9, "u8")
        d.sync()
        src.sim.generate_mod(mod, SEED, FIRST, B, 50.0, llr.data_ptr(), fmt, qs, msg_t.data_ptr(), "bytes", None, None)
        d.sync()                                         # the context decodes on its own stream
        l = d.get(llr, B, FILL[fmt])
        assert np.array_equal((l[:, :src.n_tx] > 0).astype(np.uint8), cw) and (l[:, :src.n_tx] != 0).all(), (name, fmt, "the signs are not the codeword")
        dec.decode_batch_dev(llr.data_ptr(), out.data_ptr(), B, 20, its.data_ptr(), conv.data_ptr(), None, llr_i8=(fmt == "i8"))
        dec.synchronize()
        assert (d.get(conv, B, 9) == 1).all() and (d.get(its, B, -1) == 0).all(), (name, fmt, "a noiseless frame needed an iteration")
        assert np.array_equal(d.get(out, B, 9)[:, :src.n_tx], cw)
        src.sim.extract_messages(B, out.data_ptr(), back.data_ptr())
        assert np.array_equal(d.get(back, B, 9), msg[:B]), (name, fmt)
        dec.close()
    mod.close()
    src.close()


def test_refusals(hip):
    import torch
    c = load("moon.7.13")
    code = hip.Code.from_csr(c.graph.row_ptr, c.graph.col_idx, c.N)
    dev = torch.device("cuda", 0)
    B, N, n_tx = 4, c.N, 13
    mod = hip.Modulation("4096qam")
    ns = mod.symbols(n_tx)
    assert ns == 2
    sym = torch.full((B + 1, 2 * ns + 2), 777.0, dtype=torch.float32, device=dev)
    llr = torch.full((B + 1, N), 777.0, dtype=torch.float32, device=dev)
    msg = torch.ones((B + 1, 7), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    s, l, mm = sym.data_ptr(), llr.data_ptr(), msg.data_ptr()

    def refused(code_, fn, *a, **kw):
        with pytest.raises(hip.LdpcError) as e:
            fn(*a, **kw)
        assert e.value.code == code_, str(e.value)

    refused(-1, hip.demap, mod, B, n_tx, N, None, 0.1, l)
    refused(-1, hip.demap, mod, B, n_tx, N, s, 0.1, None)
    refused(-1, hip.demap, mod, B, n_tx, N, s + 4, 0.1, l)             # samples off their 8-byte alignment
    refused(-1, hip.demap, mod, B, n_tx, N, s, 0.1, l + 2)             # float32 LLRs off their element
    refused(-1, hip.demap, mod, B, n_tx, N, s, 0.1, l + 1, "f16")
    for fmt in (3, -1):
        refused(-1, hip.demap, mod, B, n_tx, N, s, 0.1, l, fmt)
    for batch in (0, -1):
        refused(-1, hip.demap, mod, batch, n_tx, N, s, 0.1, l)
    refused(-1, hip.demap, mod, B, N + 1, N, s, 0.1, l)
    for nv in (0.0, float("nan"), 1e-40):
        refused(-1, hip.demap, mod, B, n_tx, N, s, nv, l)
    refused(-1, hip.demap, mod, B, n_tx, N, s, 0.1, l, "i8", -1.0)
    sim = hip.Sim(code, 7, n_tx, G=c.G, max_batch=B)
    for batch in (0, B + 1, -1):
        refused(-1, sim.transmit, mod, 1, 0, batch, 2.0, s)
        refused(-1, sim.generate_mod, mod, 1, 0, batch, 2.0, l)
    refused(-1, sim.transmit, mod, 1, 0, B, 2.0, None)
    refused(-1, sim.transmit, mod, 1, 0, B, 2.0, s + 4)
    refused(-1, sim.generate_mod, mod, 1, 0, B, 2.0, None)
    refused(-1, sim.generate_mod, mod, 1, 0, B, 2.0, l + 2)
    for fmt in (3, -1):
        refused(-1, sim.generate_mod, mod, 1, 0, B, 2.0, l, fmt)
        refused(-1, sim.generate_mod, mod, 1, 0, B, 2.0, l, "f32", 0.0, mm, fmt)      # the message format
        refused(-1, sim.transmit, mod, 1, 0, B, 2.0, s, mm, fmt)
    refused(-1, sim.generate_mod, mod, 1, 0, B, 400.0, l)
    refused(-1, sim.transmit, mod, 1, 0, B, float("nan"), s)
    plain = hip.Sim(code, 7, n_tx, max_batch=B)
    refused(-5, plain.transmit, mod, 1, 0, B, 2.0, s, mm)
    refused(-5, plain.generate_mod, mod, 1, 0, B, 2.0, l, "f32", 0.0, mm)
    torch.cuda.synchronize()
    assert (sym.cpu().numpy() == 777.0).all() and (llr.cpu().numpy() == 777.0).all()          # a refused call writes nothing
    # a source without an encoder sends its all-zero codewords: label 0 everywhere
    tight = torch.full((B + 1, 2 * ns), 777.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    plain.transmit(mod, 1, 0, B, 400.0, tight.data_ptr())
    plain.generate_mod(mod, 1, 0, B, 50.0, l)
    torch.cuda.synchronize()
    got, gl = tight.cpu().numpy(), llr.cpu().numpy()
    assert (got[B] == 777.0).all() and (got[:B].reshape(B, ns, 2) == mod.points[0]).all()
    assert (gl[B] == 777.0).all() and (gl[:B, :n_tx] < 0).all() and (gl[:B, n_tx:] == 0).all()
    plain.close(); sim.close(); mod.close(); code.close()
