"""GPU: the bit interleaver fused into the demapper (csrc/demap_il.hip) and into the frame source's modulated path (csrc/sim_mod_il.hip)
against tests/interleaver_spec.py, which only moves the values of tests/modulation_spec.py and tests/product_modulation_spec.py.

  1. ldpc_demap_dev_il against the spec, bit for bit (float32 as uint32, NaNs by mask): table objects m = 1..6 and product objects
     b = 1, 2, 4, 6, batch 3 and 70, the three formats (int8 at qscale 4.0 and 2.5), the samples of the existing demapper tests (NaN,
     +-inf, on a level), four tables -- (13, 13) a random permutation, (13, 20) a random injection whose 7 holes are scattered and hold
     position 0, (1280, 1408) a random permutation of the prefix with the tail punctured, (1920, 1920) the block table of 1920 / m rows
     and m columns with twists -- rows at an aligned pointer and one element past it; the identity table = ldpc_demap_dev;
  2. ldpc_sim_transmit_il: with sigma = 0 the symbols are bit for bit the points of the labels of interleave(codewords, pos); at 2 dB
     against the float64 restatement within 16 * 2^-24 * (|c| + sg * radius) per coordinate (the unit and bar of
     tests/test_modulation_gpu.py);
  3. ldpc_sim_generate_mod_il = ldpc_demap_dev_il(ldpc_sim_transmit_il), bit for bit, one source per encoder; the identity table =
     ldpc_sim_generate_mod;
  4. ldpc_interleave_bits_dev and ldpc_deinterleave_llr_dev against the spec;
  5. the chain at 50 dB on 1920.1280.3.303 through the block table;
  6. refusals through the device entry points.
Every output buffer is pre-filled with a non-zero value and carries one guard row past the batch: an unwritten hole or a write outside
the rows fails."""
import numpy as np
import pytest

from tests import dvbs2_short
from tests import interleaver_spec as ils
from tests import modulation_spec as ms
from tests import product_modulation_spec as ps
from tests.helpers import load
from tests.test_modulation_gpu import FILL, FIRST, NP_OF, SEED, TABLES, Dev, _dense_moon, _qc_jpl1024, _same, _sparse, _systematic
from tests.test_modulation_gpu import _samples as _table_samples
from tests.test_product_modulation_gpu import BUILTIN, _uneven
from tests.test_product_modulation_gpu import _samples as _product_samples

pytestmark = pytest.mark.gpu

TABLE_OF_M = {1: "bpsk", 2: "qpsk", 3: "8psk", 4: "16qam", 5: "apsk32", 6: "grid64"}


def _twist(rows, m):
    return (np.arange(m) * 7) % rows


def _block1920(m):
    return ils.block_positions(1920 // m, m, _twist(1920 // m, m))


def _tables(m):
    """{name: (pos, N)}"""
    rng = np.random.default_rng(4242)
    j = load("jpl.1024.4.5")
    assert (j.n_tx, j.N) == (1280, 1408) and 1920 % m == 0
    inj = (1 + rng.permutation(19))[:13]                     # position 0 is a hole
    h = ils.holes(inj, 20)
    assert len(h) == 7 and h[0] == 0 and (np.diff(h) > 1).sum() >= 3 and set(h.tolist()) != set(range(13, 20))      # scattered, not the tail
    return {"perm13": (rng.permutation(13), 13), "inject13of20": (inj, 20), "jpl1024-prefix": (rng.permutation(1280), 1408), "block1920": (_block1920(m), 1920)}


def _run_demap_il(hip, d, mod, il, B, sym_t, nv, fmt, qs, N, want, what):
    torch = d.torch
    item = np.dtype(NP_OF[fmt]).itemsize
    out = d.full(B, N, FILL[fmt], fmt)                       # rows at an aligned pointer
    d.sync()
    hip.demap_il(mod, il, B, sym_t.data_ptr(), nv, out.data_ptr(), fmt, qs, None)
    _same(d.get(out, B, FILL[fmt]), want, what + ("aligned",))
    flat = torch.full(((B + 1) * N + 1,), FILL[fmt], dtype=d.dt[fmt], device=d.dev)      # and one element past it
    assert flat.data_ptr() % 16 == 0
    d.sync()
    hip.demap_il(mod, il, B, sym_t.data_ptr(), nv, flat.data_ptr() + item, fmt, qs, None)
    d.sync()
    fl = flat.cpu().numpy()
    assert fl[0] == FILL[fmt] and (fl[1 + B * N:] == FILL[fmt]).all(), "written outside the rows"
    _same(fl[1:1 + B * N].reshape(B, N), want, what + ("shifted",))


def _demapper_case(hip, m, mod, samples, spec_demap, nvs):
    """spec_demap(sym, n_tx, nv, fmt, qs) -> the LLRs [B][n_tx] in transmitted order"""
    d = Dev()
    launches = 0
    for name, (pos, N) in _tables(m).items():
        n_tx = len(pos)
        il = hip.Interleaver(pos, N)
        assert il.dims == (n_tx, N) and np.array_equal(il.positions, pos)
        ident = hip.Interleaver(np.arange(n_tx), N)
        ns = ms.symbols_per_frame(n_tx, m)
        for B in (3, 70):
            sym = samples(B, ns, 1000 * m + n_tx + B)
            sym_t = d.put(sym)
            for nv in nvs:
                flat32 = spec_demap(sym, n_tx, nv, ms.LLR_F32, 4.0)
                assert np.isnan(flat32).any() or B * ns < 4
                for fmt, code, qs in (("f32", ms.LLR_F32, 0.0), ("f16", ms.LLR_F16, 0.0), ("i8", ms.LLR_I8, 4.0), ("i8", ms.LLR_I8, 2.5)):
                    tx = spec_demap(sym, n_tx, nv, code, qs or 4.0)
                    want = ils.deinterleave(tx, pos, N)
                    assert want.dtype == NP_OF[fmt] and (want[:, ils.holes(pos, N)] == 0).all()
                    _run_demap_il(hip, d, mod, il, B, sym_t, nv, fmt, qs or 4.0, N, want, (m, name, B, nv, fmt, qs))
                    launches += 2
                    if fmt != "f16" and nv == nvs[0]:        # the identity table is ldpc_demap_dev, bit for bit
                        a, b = d.full(B, N, FILL[fmt], fmt), d.full(B, N, FILL[fmt], fmt)
                        d.sync()
                        hip.demap_il(mod, ident, B, sym_t.data_ptr(), nv, a.data_ptr(), fmt, qs, None)
                        hip.demap(mod, B, n_tx, N, sym_t.data_ptr(), nv, b.data_ptr(), fmt, qs, None)
                        _same(d.get(a, B, FILL[fmt]), d.get(b, B, FILL[fmt]), (m, name, B, fmt, "identity"))
                        launches += 2
        il.close(); ident.close()
    print(f"m={m}: {launches} launches")


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6])
def test_demapper_il_table_objects_against_the_spec(hip, m):
    pts = TABLES[TABLE_OF_M[m]]()
    assert ms.bits_per_symbol(pts) == m
    mod = hip.Modulation(pts)
    _demapper_case(hip, m, mod, lambda B, ns, seed: _table_samples(pts, B, ns, seed),
                   lambda sym, n_tx, nv, fmt, qs: ms.demap(pts, sym, n_tx, n_tx, nv, fmt, qs), (0.09, 1e-3))
    mod.close()


@pytest.mark.parametrize("b", [1, 2, 4, 6])
def test_demapper_il_product_objects_against_the_spec(hip, b):
    li, lq = _uneven(b, 60 + b), (_uneven(b, 70 + b) * np.float32(0.6)).astype(np.float32)
    mod = hip.Modulation.product(li, lq)
    assert mod.bits == 2 * b
    _demapper_case(hip, 2 * b, mod, lambda B, ns, seed: _product_samples(li, lq, B, ns, seed),
                   lambda sym, n_tx, nv, fmt, qs: ps.demap(li, lq, sym, n_tx, n_tx, nv, fmt, qs), (0.02, 1e-3))
    mod.close()


# ---- the frame source
MODS = {"qpsk": lambda: ms.builtin(ms.QPSK), "8psk": lambda: ms.builtin(ms.PSK8), "grid64": ms.grid64, "256qam": None, "4096qam": None}


def _mod(hip, name):
    """-> (object, m, points [2^m][2] float32, transmit restatement(seed, ids, tx_bits, k, db))"""
    if MODS[name] is None:
        b = {"256qam": 4, "4096qam": 6}[name]
        assert BUILTIN[b] == name
        lev = ps.builtin_levels(2 * b)
        return hip.Modulation(name), 2 * b, ps.materialise(lev, lev), lambda *a: ps.transmit(lev, lev, *a)
    pts = MODS[name]()
    return hip.Modulation(pts), ms.bits_per_symbol(pts), pts, lambda *a: ms.transmit(pts, *a)


def _source_table(src, m, seed=99):
    """a table for a frame source: the twisted block table where m divides n_tx = N = 1920, a random permutation of the transmitted prefix
    otherwise"""
    if src.n_tx == src.N == 1920:
        return _block1920(m)
    return np.random.default_rng(seed + m).permutation(src.n_tx).astype(np.int32)


def _caller_codewords(d, src, B, seed):
    msg = np.random.default_rng(seed).integers(0, 2, (B + 1, src.k)).astype(np.uint8)
    msg_t = d.put(msg)
    cw_t = d.full(B, src.n_tx, 7, "u8")
    d.sync()
    src.sim.encode_messages(B, msg_t.data_ptr(), cw_t.data_ptr())
    return d.get(cw_t, B, 7), msg, msg_t


@pytest.mark.parametrize("case", ["qc-jpl1024", "systematic-1920"])
def test_transmit_il(hip, case):
    B = 33
    src = _qc_jpl1024(hip, B) if case == "qc-jpl1024" else _systematic(hip, B, "1920.1280.3.303")
    d = Dev()
    cw, msg, msg_t = _caller_codewords(d, src, B, 21)
    ids = np.uint64(FIRST) + np.arange(B, dtype=np.uint64)
    worst = 0.0
    for name in MODS:
        mod, m, pts, restate = _mod(hip, name)
        pos = _source_table(src, m)
        il = hip.Interleaver(pos, src.N)
        tx = ils.interleave(cw, pos)
        assert tx.shape == (B, src.n_tx) and not np.array_equal(tx, cw)
        ns = mod.symbols(src.n_tx)
        for db in (1000.0, 2.0):
            sym = d.full(B, 2 * ns, 777.0, "f32")
            d.sync()
            src.sim.transmit_il(mod, il, SEED, FIRST, B, db, sym.data_ptr(), msg_t.data_ptr(), "bytes", None, None)
            got = d.get(sym, B, 777.0).reshape(B, ns, 2)
            if db == 1000.0:                                 # sigma^2 ~ 1e-101: float32(sigma) = 0, y = fl(c + fl(0 z)) = c
                assert np.float32(np.sqrt(src.sim.noise_var(mod, db))) == 0.0
                want = pts[ms.labels(tx, m)]
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (case, name, "sigma = 0")
                continue
            want, unit, sg, nv = restate(SEED, ids, tx, src.k, db)
            assert nv == src.sim.noise_var(mod, db)
            err = np.abs(got.astype(np.float64) - want) / (2.0 ** -24 * unit)
            print(f"{case} {name}: worst symbol error at 2 dB = {float(err.max()):.2f} x 2^-24 (|c| + sg radius)")
            worst = max(worst, float(err.max()))
            assert err.max() <= 16.0, (case, name, float(err.max()))
        il.close(); mod.close()
    print(f"{case}: worst symbol error = {worst:.2f} x 2^-24 (|c| + sg radius)")
    src.close()


SOURCES = {
    "dense-moon-ntx13": lambda hip, B: _dense_moon(hip, B, 13),
    "qc-jpl1024": _qc_jpl1024,
    "sparse-dvbs2-short": lambda hip, B: _sparse(hip, B, *dvbs2_short.csr(), dvbs2_short.N),
    "systematic-1920": lambda hip, B: _systematic(hip, B, "1920.1280.3.303"),
}


@pytest.mark.parametrize("case", list(SOURCES))
def test_fused_il_equals_two_step(hip, case):
    B = 33
    src = SOURCES[case](hip, B)
    d = Dev()
    for name in ("8psk", "256qam"):
        mod, m, _, _ = _mod(hip, name)
        ns = mod.symbols(src.n_tx)
        pos = _source_table(src, m)
        il, ident = hip.Interleaver(pos, src.N), hip.Interleaver(np.arange(src.n_tx), src.N)
        hole = ils.holes(pos, src.N)
        for fmt, qs in (("f32", 0.0), ("i8", 4.0)):
            db = 9.0
            sym, two, one = d.full(B, 2 * ns, 777.0, "f32"), d.full(B, src.N, FILL[fmt], fmt), d.full(B, src.N, FILL[fmt], fmt)
            plain, same = d.full(B, src.N, FILL[fmt], fmt), d.full(B, src.N, FILL[fmt], fmt)
            mg = d.full(B, src.k, 9, "u8")
            d.sync()
            src.sim.transmit_il(mod, il, SEED, FIRST, B, db, sym.data_ptr(), None, "bytes", None, None)
            hip.demap_il(mod, il, B, sym.data_ptr(), src.sim.noise_var(mod, db), two.data_ptr(), fmt, qs, None)
            src.sim.generate_mod_il(mod, il, SEED, FIRST, B, db, one.data_ptr(), fmt, qs, None, "bytes", mg.data_ptr(), None)
            a, f = d.get(two, B, FILL[fmt]), d.get(one, B, FILL[fmt])
            d.get(sym, B, 777.0)
            _same(f, a, (case, name, fmt))
            assert (f[:, hole] == 0).all() and (fmt == "i8" or (f[:, pos] != 0).mean() > 0.9)
            # the identity table is ldpc_sim_generate_mod, bit for bit, and returns the same drawn messages
            mg2 = d.full(B, src.k, 9, "u8")
            d.sync()
            src.sim.generate_mod_il(mod, ident, SEED, FIRST, B, db, same.data_ptr(), fmt, qs, None, "bytes", None, None)
            src.sim.generate_mod(mod, SEED, FIRST, B, db, plain.data_ptr(), fmt, qs, None, "bytes", mg2.data_ptr(), None)
            _same(d.get(same, B, FILL[fmt]), d.get(plain, B, FILL[fmt]), (case, name, fmt, "identity"))
            assert np.array_equal(d.get(mg, B, 9), d.get(mg2, B, 9))
        il.close(); ident.close(); mod.close()
    # the instances of the fused kernels the two objects above leave out (every m and b = 1..6, in every format): the two steps, bit for bit
    pts_of = {m: TABLES[TABLE_OF_M[m]]() for m in range(1, 7)}
    objects = [(f"m={m}", m, lambda m=m: hip.Modulation(pts_of[m])) for m in range(1, 7)]
    objects += [(f"b={b}", 2 * b, lambda b=b: hip.Modulation.product(_uneven(b, 60 + b), _uneven(b, 70 + b))) for b in range(1, 7)]
    for name, m, make in objects:
        mod = make()
        assert mod.bits == m
        ns = mod.symbols(src.n_tx)
        pos = _source_table(src, m)
        il = hip.Interleaver(pos, src.N)
        for fmt, qs in (("f16", 0.0),) if name in ("m=3", "b=4") else (("f32", 0.0), ("f16", 0.0), ("i8", 4.0)):
            sym, two, one = d.full(B, 2 * ns, 777.0, "f32"), d.full(B, src.N, FILL[fmt], fmt), d.full(B, src.N, FILL[fmt], fmt)
            d.sync()
            src.sim.transmit_il(mod, il, SEED, FIRST, B, 9.0, sym.data_ptr(), None, "bytes", None, None)
            hip.demap_il(mod, il, B, sym.data_ptr(), src.sim.noise_var(mod, 9.0), two.data_ptr(), fmt, qs, None)
            src.sim.generate_mod_il(mod, il, SEED, FIRST, B, 9.0, one.data_ptr(), fmt, qs, None, "bytes", None, None)
            a, f = d.get(two, B, FILL[fmt]), d.get(one, B, FILL[fmt])
            d.get(sym, B, 777.0)
            _same(f, a, (case, name, fmt, "every instance"))
            assert (f[:, ils.holes(pos, src.N)] == 0).all()
        il.close(); mod.close()
    src.close()


# ---- the table alone
@pytest.mark.parametrize("shape", ["inject13of20", "jpl1024-prefix"])
def test_interleave_bits_and_deinterleave_llr(hip, shape):
    pos, N = _tables(1)[shape]
    n_tx = len(pos)
    il = hip.Interleaver(pos, N)
    d = Dev()
    rng = np.random.default_rng(n_tx)
    for B in (3, 70):
        cw = rng.integers(0, 2, (B, N)).astype(np.uint8)
        noisy = (cw | (rng.integers(0, 128, (B, N)).astype(np.uint8) << 1)).astype(np.uint8)      # bytes in: only bit 0 is read
        ins = {"bytes": d.put(noisy), "packed": d.put(ils.pack(cw))}
        tx = ils.interleave(cw, pos)
        wants = {"bytes": tx, "packed": ils.pack(tx)}
        assert wants["packed"].shape == (B, (n_tx + 7) // 8)
        for fi, src_t in ins.items():
            for fo, want in wants.items():
                out = d.full(B, want.shape[1], 0x5A, "u8")
                d.sync()
                hip.interleave_bits(il, B, src_t.data_ptr(), out.data_ptr(), fi, fo, None)
                assert np.array_equal(d.get(out, B, 0x5A), want), (shape, B, fi, fo)
        for fmt in ("f32", "f16", "i8"):
            x = np.clip(rng.normal(0, 20, (B, n_tx)), -127, 127).astype(NP_OF[fmt])
            x[0, 0] = 0                                       # a zero that is data, next to the zeros that are holes
            if fmt != "i8":
                x[0, 1], x[1, 0] = np.nan, -np.inf
            out = d.full(B, N, FILL[fmt], fmt)
            x_t = d.put(x)
            d.sync()
            hip.deinterleave_llr(il, B, x_t.data_ptr(), out.data_ptr(), fmt, None)
            _same(d.get(out, B, FILL[fmt]), ils.deinterleave(x, pos, N), (shape, B, fmt))
    il.close()


# ---- the chain
@pytest.mark.parametrize("name", ["256qam", "4096qam"])
def test_chain_il_noiseless_frames_need_no_iteration(hip, name):
    B = 33
    src = _systematic(hip, B, "1920.1280.3.303")
    d = Dev()
    torch = d.torch
    mod = hip.Modulation(name)
    il = hip.Interleaver.block(1920 // mod.bits, mod.bits, _twist(1920 // mod.bits, mod.bits))
    assert il.dims == (1920, 1920) and np.array_equal(il.positions, _block1920(mod.bits))
    cw, msg, msg_t = _caller_codewords(d, src, B, 7)
    for kind, fmt, qs in (("f32", "f32", 0.0), ("i8", "i8", 4.0)):
        dec = hip.Decoder(src.code, "min", kind, B, schedule="layered", **({"qscale": qs} if kind == "i8" else {}))
        llr = d.full(B, src.N, FILL[fmt], fmt)
        out, its, conv = d.full(B, src.N, 9, "u8"), torch.full((B + 1,), -1, dtype=torch.int32, device=d.dev), torch.full((B + 1,), 9, dtype=torch.uint8, device=d.dev)
        back = d.full(B, src.k, 9, "u8")
        tally = torch.zeros(4, dtype=torch.int64, device=d.dev)
        d.sync()
        src.sim.generate_mod_il(mod, il, SEED, FIRST, B, 50.0, llr.data_ptr(), fmt, qs, msg_t.data_ptr(), "bytes", None, None)
        d.sync()                                             # the context decodes on its own stream
        l = d.get(llr, B, FILL[fmt])
        assert np.array_equal((l > 0).astype(np.uint8), cw) and (l != 0).all(), (name, fmt, "the signs are not the codeword")
        dec.decode_batch_dev(llr.data_ptr(), out.data_ptr(), B, 20, its.data_ptr(), conv.data_ptr(), None, llr_i8=(fmt == "i8"))
        dec.synchronize()
        assert (d.get(conv, B, 9) == 1).all() and (d.get(its, B, -1) == 0).all(), (name, fmt, "a noiseless frame needed an iteration")
        assert np.array_equal(d.get(out, B, 9), cw)
        src.sim.extract_messages(B, out.data_ptr(), back.data_ptr())
        src.sim.tally(B, out.data_ptr(), its.data_ptr(), tally.data_ptr(), None)
        assert np.array_equal(d.get(back, B, 9), msg[:B]), (name, fmt)
        assert tally.cpu().numpy().tolist() == [B, 0, 0, 0], (name, fmt)
        dec.close()
    il.close(); mod.close()
    src.close()


def test_refusals(hip):
    import torch
    B = 4
    src = _qc_jpl1024(hip, B)
    n_tx, N = src.n_tx, src.N
    dev = torch.device("cuda", 0)
    mod = hip.Modulation("qpsk")
    ns = mod.symbols(n_tx)
    sym = torch.full((B + 1, 2 * ns), 777.0, dtype=torch.float32, device=dev)
    llr = torch.full((B + 1, N), 777.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    s, l = sym.data_ptr(), llr.data_ptr()
    rng = np.random.default_rng(3)
    good = hip.Interleaver(rng.permutation(n_tx), N)
    short = hip.Interleaver(rng.permutation(n_tx - 2), N)                     # n_tx is not the source's
    narrow = hip.Interleaver(rng.permutation(n_tx), n_tx)                     # N is not the code's
    past = rng.permutation(n_tx)
    past[5] = N - 1                                                           # reaches into the punctured tail, past the source's n_tx
    reach = hip.Interleaver(past, N)

    def refused(fn, *a, **kw):
        with pytest.raises(hip.LdpcError) as e:
            fn(*a, **kw)
        assert e.value.code == -1, str(e.value)

    for il in (None, short, narrow, reach):
        refused(src.sim.transmit_il, mod, il, 1, 0, B, 2.0, s)
        refused(src.sim.generate_mod_il, mod, il, 1, 0, B, 2.0, l)
    refused(src.sim.transmit_il, None, good, 1, 0, B, 2.0, s)
    refused(src.sim.transmit_il, mod, good, 1, 0, B, 2.0, None)
    refused(src.sim.transmit_il, mod, good, 1, 0, B, 2.0, s + 4)
    refused(src.sim.transmit_il, mod, good, 1, 0, B, float("nan"), s)
    refused(src.sim.generate_mod_il, mod, good, 1, 0, B, 2.0, None)
    refused(src.sim.generate_mod_il, mod, good, 1, 0, B, 2.0, l + 2)
    refused(src.sim.generate_mod_il, mod, good, 1, 0, B, 400.0, l)
    refused(src.sim.generate_mod_il, mod, good, 1, 0, B, 2.0, l, 3)
    for batch in (0, B + 1, -1):
        refused(src.sim.transmit_il, mod, good, 1, 0, batch, 2.0, s)
        refused(src.sim.generate_mod_il, mod, good, 1, 0, batch, 2.0, l)
    # the demapper: those of ldpc_demap_dev, and a null table
    refused(hip.demap_il, mod, None, B, s, 0.1, l)
    refused(hip.demap_il, None, good, B, s, 0.1, l)
    refused(hip.demap_il, mod, good, B, None, 0.1, l)
    refused(hip.demap_il, mod, good, B, s, 0.1, None)
    refused(hip.demap_il, mod, good, B, s + 4, 0.1, l)
    refused(hip.demap_il, mod, good, B, s, 0.1, l + 2)
    refused(hip.demap_il, mod, good, B, s, 0.1, l + 1, "f16")
    for batch in (0, -1):
        refused(hip.demap_il, mod, good, batch, s, 0.1, l)
    for fmt in (3, -1):
        refused(hip.demap_il, mod, good, B, s, 0.1, l, fmt)
    for nv in (0.0, -0.5, float("nan"), float("inf"), 1e-40):
        refused(hip.demap_il, mod, good, B, s, nv, l)
    for qs in (-1.0, float("nan"), float("inf")):
        refused(hip.demap_il, mod, good, B, s, 0.1, l, "i8", qs)
    # the table alone
    refused(hip.interleave_bits, None, B, l, s)
    refused(hip.interleave_bits, good, B, None, s)
    refused(hip.interleave_bits, good, B, l, None)
    refused(hip.interleave_bits, good, 0, l, s)
    refused(hip.interleave_bits, good, B, l, s, 2, "bytes")
    refused(hip.interleave_bits, good, B, l, s, "bytes", -1)
    refused(hip.deinterleave_llr, None, B, s, l)
    refused(hip.deinterleave_llr, good, B, None, l)
    refused(hip.deinterleave_llr, good, B, s, None)
    refused(hip.deinterleave_llr, good, 0, s, l)
    refused(hip.deinterleave_llr, good, B, s, l, 3)
    refused(hip.deinterleave_llr, good, B, s + 2, l)
    torch.cuda.synchronize()
    assert (sym.cpu().numpy() == 777.0).all() and (llr.cpu().numpy() == 777.0).all()          # a refused call writes nothing
    # a table that reaches past the source's n_tx is a table like any other to the demapper
    src.sim.transmit(mod, 1, 0, B, 6.0, s)
    hip.demap_il(mod, reach, B, s, 0.1, l)
    want = torch.full((B + 1, N), 777.0, dtype=torch.float32, device=dev)
    hip.demap(mod, B, n_tx, n_tx, s, 0.1, want.data_ptr())                    # [B][n_tx] rows in the front of the buffer
    torch.cuda.synchronize()
    got = llr.cpu().numpy()
    flat = want.cpu().numpy().reshape(-1)[:B * n_tx].reshape(B, n_tx)
    assert (got[B] == 777.0).all() and np.array_equal(got[:B], ils.deinterleave(flat, past, N))
    for o in (good, short, narrow, reach, mod):
        o.close()
    src.close()
