"""GPU: higher-order modulation -- the device soft demapper (csrc/demap.hip) and the frame source's modulated path (csrc/sim_mod.hip)
against tests/modulation_spec.py.

  1. ldpc_demap_dev against the spec, bit for bit (float32 compared as uint32, NaNs by mask): m = 1..6, batch 3 and 70,
     n_tx in {5m, 5m + 1, 1920, 1917}, N = n_tx and n_tx + 9, the three formats, qscale 4 and 2.5, rows at an aligned pointer and one
     element past it (the element stores);
  2. ldpc_sim_transmit against the float64 restatement of the channel, within 16 * 2^-24 * (|c| + sg * radius) per coordinate (the bar and
     unit of tests/test_frame_source_gpu.py; measured on MI355X: at most 3.31); at 300 dB the symbols are the
     constellation points;
  3. ldpc_sim_generate_mod = ldpc_demap_dev(ldpc_sim_transmit), bit for bit, one source per encoder;
  4. replay: the drawn messages fed back give the same LLRs;
  5. the chain into the decoders, f32 and int8;
  6. refusals.
Every output buffer carries one guard row past the batch, which must stay untouched."""
import numpy as np
import pytest

from tests import dvbs2_short
from tests import layered_i8_spec
from tests import modulation_spec as ms
from tests import systematic_encoder_spec as sys_spec
from tests.helpers import CODES, load

pytestmark = pytest.mark.gpu

SEED, FIRST = 0x5EEDC0DE12345, 2 ** 32 + 11
TABLES = {
    "bpsk": lambda: ms.builtin(ms.BPSK), "qpsk": lambda: ms.builtin(ms.QPSK), "8psk": lambda: ms.builtin(ms.PSK8), "16qam": lambda: ms.builtin(ms.QAM16),
    "apsk16": lambda: ms.rings((1.0, 3.15), (4, 12), (np.pi / 4, np.pi / 12)),            # 4 + 12 points, gamma = 3.15
    "apsk32": lambda: ms.rings((1.0, 2.84, 5.27), (4, 12, 16), (np.pi / 4, np.pi / 12, 0.0)),
    "grid64": ms.grid64,
}
NP_OF = {"f32": np.float32, "f16": np.float16, "i8": np.int8}
FILL = {"f32": 777.0, "f16": 777.0, "i8": 99}


class Dev:
    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.dt = {"f32": torch.float32, "f16": torch.float16, "i8": torch.int8, "u8": torch.uint8}

    def full(self, rows, cols, fill, kind):
        return self.torch.full((rows + 1, cols), fill, dtype=self.dt[kind], device=self.dev)

    def put(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def sync(self):
        self.torch.cuda.synchronize()

    def get(self, t, rows, fill):
        self.sync()
        a = t.cpu().numpy()
        assert (a[rows:] == fill).all(), "a row past the batch was written"
        return a[:rows]


def _same(got, want, what):
    """bit for bit; NaNs by mask"""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.dtype == np.int8:
        assert np.array_equal(got, want), what
        return
    gn, wn = np.isnan(got), np.isnan(want)
    u = np.uint32 if got.dtype == np.float32 else np.uint16
    assert np.array_equal(gn, wn), (what, "NaN mask")
    assert np.array_equal(np.where(gn, 0, got.view(u)), np.where(wn, 0, want.view(u))), what


def _samples(pts, B, ns, seed):
    """[B][ns][2] float32: a point plus N(0, 0.3^2); then, from the front and as far as they fit: the points themselves, the midpoint
    of every point and its nearest neighbour, a block of magnitudes up to 1e3, one NaN sample"""
    rng = np.random.default_rng(seed)
    n = B * ns
    y = (pts[rng.integers(0, len(pts), n)] + rng.normal(0.0, 0.3, (n, 2))).astype(np.float32)
    p64 = pts.astype(np.float64)
    d = ((p64[:, None] - p64[None]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    mid = ((pts + pts[d.argmin(1)]) * np.float32(0.5)).astype(np.float32)
    big = (rng.uniform(-1e3, 1e3, (16, 2))).astype(np.float32)
    special = np.concatenate([pts, mid, big])[:max(n - 2, 0)]
    y[:len(special)] = special
    y[n - 2] = (np.nan, 0.25)
    return y.reshape(B, ns, 2)


@pytest.mark.parametrize("name", list(TABLES))
def test_demapper_against_the_spec(hip, name):
    pts = TABLES[name]()
    m = ms.bits_per_symbol(pts)
    mod = hip.Modulation(pts)
    d = Dev()
    torch = d.torch
    launches = 0
    for B in (3, 70):
        for n_tx in (5 * m, 5 * m + 1, 1920, 1917):
            ns = ms.symbols_per_frame(n_tx, m)
            assert mod.symbols(n_tx) == ns
            sym = _samples(pts, B, ns, 1000 * m + n_tx + B)
            sym_t = d.put(sym)
            for nv in (0.09, 1e-3):                      # 1e-3 with the 1e3 block: fp16 saturates, int8 clips
                per = ms.symbol_llrs(pts, sym, nv).reshape(B, ns * m)[:, :n_tx]
                for N in (n_tx, n_tx + 9):
                    f32 = np.zeros((B, N), np.float32)
                    f32[:, :n_tx] = per
                    wants = {("f32", 0.0): f32, ("f16", 0.0): ms.round_f16(f32), ("i8", 4.0): ms.demap(pts, sym, n_tx, N, nv, ms.LLR_I8, 4.0),
                             ("i8", 2.5): ms.demap(pts, sym, n_tx, N, nv, ms.LLR_I8, 2.5)}
                    if nv == 1e-3 and B * ns > 2 * len(pts) + 18:
                        assert np.abs(wants[("f16", 0.0)][np.isfinite(f32)].astype(np.float32)).max() == 65504.0 and np.abs(wants[("i8", 4.0)]).max() == 127
                    assert np.isnan(f32).any()
                    for (fmt, qs), want in wants.items():
                        item = np.dtype(NP_OF[fmt]).itemsize
                        # rows at an aligned pointer
                        out = d.full(B, N, FILL[fmt], fmt)
                        d.sync()
                        hip.demap(mod, B, n_tx, N, sym_t.data_ptr(), nv, out.data_ptr(), fmt, qs, None)
                        _same(d.get(out, B, FILL[fmt]), want, (name, B, n_tx, N, nv, fmt, qs, "aligned"))
                        # and one element past it: no vector store may be used
                        flat = torch.full(((B + 1) * N + 1,), FILL[fmt], dtype=d.dt[fmt], device=d.dev)
                        assert flat.data_ptr() % 16 == 0
                        d.sync()
                        hip.demap(mod, B, n_tx, N, sym_t.data_ptr(), nv, flat.data_ptr() + item, fmt, qs, None)
                        d.sync()
                        fl = flat.cpu().numpy()
                        assert fl[0] == FILL[fmt] and (fl[1 + B * N:] == FILL[fmt]).all(), "written outside the rows"
                        _same(fl[1:1 + B * N].reshape(B, N), want, (name, B, n_tx, N, nv, fmt, qs, "shifted"))
                        launches += 2
    # qscale 0 is 4.0
    out = d.full(B, N, 99, "i8")
    d.sync()
    hip.demap(mod, B, n_tx, N, sym_t.data_ptr(), nv, out.data_ptr(), "i8", 0.0, None)
    _same(d.get(out, B, 99), wants[("i8", 4.0)], "qscale 0")
    print(f"{name}: m={m}, {launches} launches")
    mod.close()


# ---- frame sources, one per encoder
class Source:
    def __init__(self, sim, code, N, n_tx, owners):
        self.sim, self.code, self.N, self.n_tx, self.k, self.owners = sim, code, N, n_tx, sim.k, owners

    def close(self):
        for o in self.owners:
            o.close()


def _dense_moon(hip, B, n_tx):
    c = load("moon.7.13")
    code = hip.Code.from_csr(c.graph.row_ptr, c.graph.col_idx, c.N)
    sim = hip.Sim(code, 7, n_tx, G=c.G, max_batch=B)
    return Source(sim, code, c.N, n_tx, (sim, code))


def _qc_jpl1024(hip, B):
    c = load("jpl.1024.4.5")
    ecc = hip.ECC(CODES, "ldpc/hip-minsum/jpl.1024.4.5/50/4/5", max_batch=B)
    assert c.n_tx < c.N and ecc.sim.encoder == "qc"                    # a punctured tail
    code = c.hip_code(hip)
    return Source(ecc.sim, code, c.N, c.n_tx, (ecc, code))


def _sparse(hip, B, rp, ci, N):
    code = hip.Code.from_csr(rp, ci, N)
    sim = hip.Sim(code, N - (len(rp) - 1), N, from_H=True, max_batch=B)
    return Source(sim, code, N, N, (sim, code))


def _sparse_moon(hip, B):
    c = load("moon.7.13")
    return _sparse(hip, B, c.graph.row_ptr, c.graph.col_idx, c.N)


def _systematic(hip, B, name):
    H = sys_spec.toy_40x90() if name == "40x90" else load(name).H
    N = H.shape[1]
    code = hip.Code.from_csr(*sys_spec.csr(H), N)
    sim = hip.Sim(code, None, N, systematic=True, max_batch=B)
    return Source(sim, code, N, N, (sim, code))


SOURCES = {
    "dense-moon-ntx13": (33, lambda hip, B: _dense_moon(hip, B, 13)),
    "dense-moon-ntx11": (33, lambda hip, B: _dense_moon(hip, B, 11)),
    "qc-jpl1024": (33, _qc_jpl1024),
    "sparse-dvbs2-short": (33, lambda hip, B: _sparse(hip, B, *dvbs2_short.csr(), dvbs2_short.N)),
    "systematic-40x90": (33, lambda hip, B: _systematic(hip, B, "40x90")),
    "sparse-moon-chunk": (16385, _sparse_moon),                         # crosses the 16 384-frame chunk of the encoder's scratch
}
MODS = {2: "qpsk", 3: "8psk", 5: "apsk32"}


def _codewords(d, src, B, seed=SEED, first=FIRST):
    cw, msg = d.full(B, src.n_tx, 7, "u8"), d.full(B, src.k, 9, "u8")
    d.sync()
    src.sim.encode_batch(seed, first, B, cw.data_ptr(), msg.data_ptr(), None)
    return d.get(cw, B, 7), d.get(msg, B, 9), msg


@pytest.mark.parametrize("case", ["dense-moon-ntx13", "dense-moon-ntx11", "qc-jpl1024", "systematic-40x90"])
def test_transmit_against_the_restatement(hip, case):
    B, make = SOURCES[case]
    src = make(hip, B)
    d = Dev()
    worst, odd_seen = 0.0, False
    for seed, first in ((SEED, FIRST), (2 ** 63 + 12345, 2 ** 40 + 2 ** 32 - 5)):        # seeds and frame ids past 2^32 (the ids cross a multiple of 2^32)
        cw, msg, _ = _codewords(d, src, B, seed, first)
        ids = np.uint64(first) + np.arange(B, dtype=np.uint64)
        for name in ("bpsk", "qpsk", "8psk", "16qam", "apsk32", "grid64"):
            pts = TABLES[name]()
            m = ms.bits_per_symbol(pts)
            mod = hip.Modulation(pts)
            ns = mod.symbols(src.n_tx)
            for db in (3.0, 300.0):
                sym, mg = d.full(B, 2 * ns, 777.0, "f32"), d.full(B, src.k, 9, "u8")
                d.sync()
                src.sim.transmit(mod, seed, first, B, db, sym.data_ptr(), None, "bytes", mg.data_ptr(), None)
                got = d.get(sym, B, 777.0).reshape(B, ns, 2)
                assert np.array_equal(d.get(mg, B, 9), msg)
                want, unit, sg, nv = ms.transmit(pts, seed, ids, cw, src.k, db)
                assert nv == src.sim.noise_var(mod, db) == ms.noise_var(src.k, src.n_tx, pts, db)
                if db == 300.0:
                    # sg ~ 1e-15, |z| < 7: fl(c + fl(sg z)) = c wherever sg |z| is below half an ulp of c, i.e. for every non-zero
                    # coordinate of these tables (all above 0.1); a zero coordinate (BPSK's Q, the axes of 8PSK and of the ring
                    # tables) keeps the product itself, below 1e-13
                    c = pts[ms.labels(cw, m)]
                    assert ((c == 0) | (np.abs(c) > 0.1)).all() and sg < 2e-15
                    assert np.array_equal(got[c != 0].view(np.uint32), c[c != 0].view(np.uint32)), (case, name, "300 dB")
                    assert (np.abs(got[c == 0]) < 1e-13).all()
                    continue
                err = np.abs(got.astype(np.float64) - want) / (2.0 ** -24 * unit)
                worst = max(worst, float(err.max()))
                assert err.max() <= 16.0, (case, name, float(err.max()))
            odd_seen |= bool(ns % 2)
            mod.close()
    assert odd_seen, "no table left this source an odd symbol count: the half-used last Philox call is not covered"
    print(f"{case}: worst symbol error = {worst:.2f} x 2^-24 (|c| + sg radius)")
    src.close()


def _two_step_and_fused(hip, d, src, mod, B, db, fmt, qs, msg_in=None, msg_fmt="bytes", want_msg=False):
    ns = mod.symbols(src.n_tx)
    sym, two, one = d.full(B, 2 * ns, 777.0, "f32"), d.full(B, src.N, FILL[fmt], fmt), d.full(B, src.N, FILL[fmt], fmt)
    mg = d.full(B, src.k, 9, "u8")
    d.sync()
    src.sim.transmit(mod, SEED, FIRST, B, db, sym.data_ptr(), msg_in, msg_fmt, None, None)
    hip.demap(mod, B, src.n_tx, src.N, sym.data_ptr(), src.sim.noise_var(mod, db), two.data_ptr(), fmt, qs, None)
    src.sim.generate_mod(mod, SEED, FIRST, B, db, one.data_ptr(), fmt, qs, msg_in, msg_fmt, mg.data_ptr() if want_msg else None, None)
    a, b = d.get(two, B, FILL[fmt]), d.get(one, B, FILL[fmt])
    d.get(sym, B, 777.0)
    return a, b, (d.get(mg, B, 9) if want_msg else None)


@pytest.mark.parametrize("case", list(SOURCES))
def test_fused_equals_two_step(hip, case):
    B, make = SOURCES[case]
    src = make(hip, B)
    d = Dev()
    cw, msg, msg_t = _codewords(d, src, B)
    for m, name in MODS.items():
        mod = hip.Modulation(TABLES[name]())
        assert mod.bits == m
        for fmt, qs in (("f32", 0.0), ("f16", 0.0), ("i8", 4.0)) if B < 1000 else (("f32", 0.0),):
            two, one, got_msg = _two_step_and_fused(hip, d, src, mod, B, 3.0, fmt, qs, want_msg=True)
            _same(one, two, (case, name, fmt))
            assert (one[:, src.n_tx:] == 0).all() and np.array_equal(got_msg, msg)          # 4. d_msg is ldpc_sim_encode_batch's
            assert (one[:, :src.n_tx] != 0).mean() > 0.9
            # 4. replay: the drawn messages, fed back, give the same LLRs
            _, again, _ = _two_step_and_fused(hip, d, src, mod, B, 3.0, fmt, qs, msg_in=msg_t.data_ptr())
            _same(again, one, (case, name, fmt, "replay"))
        # 5. at 40 dB the signs are the codeword
        _, l40, _ = _two_step_and_fused(hip, d, src, mod, B, 40.0, "f32", 0.0)
        assert np.array_equal((l40[:, :src.n_tx] > 0).astype(np.uint8), cw), (case, name, "40 dB")
        mod.close()
    # the instances of the fused kernel the tables above leave out (m = 1, 4, 6), in every format: the two steps, bit for bit
    for name in ("bpsk", "16qam", "grid64") if B < 1000 else ():
        mod = hip.Modulation(TABLES[name]())
        for fmt, qs in (("f32", 0.0), ("f16", 0.0), ("i8", 4.0)):
            two, one, _ = _two_step_and_fused(hip, d, src, mod, B, 3.0, fmt, qs)
            _same(one, two, (case, name, fmt))
            assert (one[:, src.n_tx:] == 0).all()
        mod.close()
    src.close()


def test_chain_noiseless_frames_need_no_iteration(hip):
    B = 33
    src = _sparse(hip, B, *dvbs2_short.csr(), dvbs2_short.N)
    d = Dev()
    torch = d.torch
    cw, msg, _ = _codewords(d, src, B)
    dec = hip.Decoder(src.code, "min", "f32", B, schedule="layered")
    for name in ("qpsk", "8psk", "apsk32"):
        mod = hip.Modulation(TABLES[name]())
        llr = d.full(B, src.N, 777.0, "f32")
        out, its, conv = d.full(B, src.N, 9, "u8"), torch.full((B + 1,), -1, dtype=torch.int32, device=d.dev), torch.full((B + 1,), 9, dtype=torch.uint8, device=d.dev)
        d.sync()
        src.sim.generate_mod(mod, SEED, FIRST, B, 40.0, llr.data_ptr(), "f32", 0.0, None, "bytes", None, None)
        d.sync()                                         # the context decodes on its own stream
        dec.decode_batch_dev(llr.data_ptr(), out.data_ptr(), B, 20, its.data_ptr(), conv.data_ptr(), None)
        dec.synchronize()
        assert (d.get(conv, B, 9) == 1).all() and (d.get(its, B, -1) == 0).all(), "a noiseless frame needed an iteration"
        assert np.array_equal(d.get(out, B, 9), cw)
        mod.close()
    dec.close()
    src.close()


def test_chain_int8_llrs_decode_as_the_quantised_floats(hip):
    """8PSK at 4 dB on 1920.1280.3.303: an LDPC_I8 context given generate_mod's float32 LLRs quantises them in its prologue; given
    generate_mod's int8 LLRs (same seed, same qscale) it reads them as they are.  The quantiser is one rule: bits, iterations and flags
    are identical.  ldpc_sim_tally counts against the messages of that generate_mod."""
    B = 64
    src = _systematic(hip, B, "1920.1280.3.303")
    d = Dev()
    torch = d.torch
    mod = hip.Modulation("8psk")
    mp, _ = src.sim.positions()
    for qs in (4.0, 2.5):
        dec = hip.Decoder(src.code, "min", "i8", B, schedule="layered", qscale=qs)
        res = []
        msgs = d.full(B, src.k, 9, "u8")
        for fmt in ("f32", "i8"):
            llr = d.full(B, src.N, FILL[fmt], fmt)
            out, its, conv = d.full(B, src.N, 9, "u8"), torch.full((B + 1,), -1, dtype=torch.int32, device=d.dev), torch.full((B + 1,), 9, dtype=torch.uint8, device=d.dev)
            d.sync()
            src.sim.generate_mod(mod, SEED, FIRST, B, 4.0, llr.data_ptr(), fmt, qs, None, "bytes", msgs.data_ptr(), None)
            d.sync()                                     # the context decodes on its own stream
            dec.decode_batch_dev(llr.data_ptr(), out.data_ptr(), B, 30, its.data_ptr(), conv.data_ptr(), None, llr_i8=(fmt == "i8"))
            dec.synchronize()
            t = torch.zeros(4, dtype=torch.int64, device=d.dev)
            d.sync()
            src.sim.tally(B, out.data_ptr(), its.data_ptr(), t.data_ptr(), None)
            d.sync()
            res.append((d.get(out, B, 9), d.get(its, B, -1), d.get(conv, B, 9), t.cpu().numpy().tolist(), d.get(llr, B, FILL[fmt])))
        (b0, i0, c0, t0, l0), (b1, i1, c1, t1, l1) = res
        assert np.array_equal(l1.astype(np.int32), layered_i8_spec.quantize(l0, qs))
        assert np.array_equal(b0, b1) and np.array_equal(i0, i1) and np.array_equal(c0, c1) and t0 == t1
        m = d.get(msgs, B, 9)
        wrong = (b1[:, mp] != m)
        assert t1 == [B, int(wrong.any(1).sum()), int(wrong.sum()), int(i1.sum())]
        print(f"qscale {qs}: {int(c1.sum())}/{B} converged, mean iterations {i1.mean():.2f}, message-bit errors {int(wrong.sum())}")
        assert c1.mean() > 0.5 and i1.max() > 0, "4 dB 8PSK should be decodable and need iterations"
        dec.close()
    mod.close()
    src.close()


def test_refusals(hip):
    import torch
    c = load("moon.7.13")
    code = hip.Code.from_csr(c.graph.row_ptr, c.graph.col_idx, c.N)
    dev = torch.device("cuda", 0)
    B, N, n_tx = 4, c.N, 13
    mod = hip.Modulation("qpsk")
    ns = mod.symbols(n_tx)
    sym = torch.full((B + 1, 2 * ns), 777.0, dtype=torch.float32, device=dev)
    llr = torch.full((B + 1, N), 777.0, dtype=torch.float32, device=dev)
    msg = torch.ones((B + 1, 7), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    s, l, mm = sym.data_ptr(), llr.data_ptr(), msg.data_ptr()

    def refused(code_, fn, *a, **kw):
        with pytest.raises(hip.LdpcError) as e:
            fn(*a, **kw)
        assert e.value.code == code_, str(e.value)

    # the demapper
    refused(-1, hip.demap, None, B, n_tx, N, s, 0.1, l)
    refused(-1, hip.demap, mod, B, n_tx, N, None, 0.1, l)
    refused(-1, hip.demap, mod, B, n_tx, N, s, 0.1, None)
    for batch in (0, -1):
        refused(-1, hip.demap, mod, batch, n_tx, N, s, 0.1, l)
    for fmt in (3, -1):
        refused(-1, hip.demap, mod, B, n_tx, N, s, 0.1, l, fmt)
    for nv in (0.0, -0.5, float("nan"), float("inf")):
        refused(-1, hip.demap, mod, B, n_tx, N, s, nv, l)
    for qs in (-1.0, float("nan"), float("inf")):
        refused(-1, hip.demap, mod, B, n_tx, N, s, 0.1, l, "i8", qs)
    refused(-1, hip.demap, mod, B, N + 1, N, s, 0.1, l)                 # n_tx > N
    refused(-1, hip.demap, mod, B, n_tx, N, s, 1e-40, l)                # 1 / (2 noise_var) is no float32
    # the frame source
    sim = hip.Sim(code, 7, n_tx, G=c.G, max_batch=B)
    for batch in (0, B + 1, -1):
        refused(-1, sim.transmit, mod, 1, 0, batch, 2.0, s)
        refused(-1, sim.generate_mod, mod, 1, 0, batch, 2.0, l)
    refused(-1, sim.transmit, None, 1, 0, B, 2.0, s)
    refused(-1, sim.transmit, mod, 1, 0, B, 2.0, None)
    refused(-1, sim.generate_mod, None, 1, 0, B, 2.0, l)
    refused(-1, sim.generate_mod, mod, 1, 0, B, 2.0, None)
    for fmt in (3, -1):
        refused(-1, sim.generate_mod, mod, 1, 0, B, 2.0, l, fmt)
        refused(-1, sim.generate_mod, mod, 1, 0, B, 2.0, l, "f32", 0.0, mm, fmt)      # the message format
        refused(-1, sim.transmit, mod, 1, 0, B, 2.0, s, mm, fmt)
    refused(-1, sim.generate_mod, mod, 1, 0, B, 2.0, l, "i8", -2.0)
    refused(-1, sim.generate_mod, mod, 1, 0, B, 400.0, l)              # 1 / (2 sigma^2) is no float32; transmit takes it (below)
    refused(-1, sim.generate_mod, mod, 1, 0, B, float("nan"), l)
    refused(-1, sim.transmit, mod, 1, 0, B, float("nan"), s)
    plain = hip.Sim(code, 7, n_tx, max_batch=B)
    assert plain.encoder == "none"
    refused(-5, plain.transmit, mod, 1, 0, B, 2.0, s, mm)
    refused(-5, plain.generate_mod, mod, 1, 0, B, 2.0, l, "f32", 0.0, mm)
    torch.cuda.synchronize()
    assert (sym.cpu().numpy() == 777.0).all() and (llr.cpu().numpy() == 777.0).all()          # a refused call writes nothing
    # a source without an encoder still sends its all-zero codewords: label 0 everywhere
    plain.transmit(mod, 1, 0, B, 400.0, s)
    plain.generate_mod(mod, 1, 0, B, 40.0, l)
    torch.cuda.synchronize()
    got, gl = sym.cpu().numpy(), llr.cpu().numpy()
    assert (got[B] == 777.0).all() and (got[:B].reshape(B, ns, 2) == mod.points[0]).all()
    assert (gl[B] == 777.0).all() and (gl[:B, :n_tx] < 0).all() and (gl[:B, n_tx:] == 0).all()
    plain.close(); sim.close(); mod.close(); code.close()


def test_which_error_wins(hip):
    """A call with TWO mistakes is refused with the error of the check that comes first.  The entry points of the demappers and of the
    modulated path share their argument checks (api.cc demap_args, sim_mod_check, sim_mod_run); this table pins the order those run
    in, entry point by entry point: each row is a call, and a piece of the text ldpc_last_error() must hold"""
    import torch
    c = load("moon.7.13")
    code = hip.Code.from_csr(c.graph.row_ptr, c.graph.col_idx, c.N)
    dev = torch.device("cuda", 0)
    B, N, n_tx = 4, c.N, 13
    mod = hip.Modulation("qpsk")
    logmap = mod.with_rule("logmap")
    ns = mod.symbols(n_tx)
    sym = torch.full((B + 1, 2 * ns + 2), 777.0, dtype=torch.float32, device=dev)
    gain = torch.full((B + 1, ns + 2), 1.0, dtype=torch.float32, device=dev)
    llr = torch.full((B + 1, N + 2), 777.0, dtype=torch.float32, device=dev)
    la = torch.zeros((B + 1, N + 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    s, g, l, a = sym.data_ptr(), gain.data_ptr(), llr.data_ptr(), la.data_ptr()
    il = hip.Interleaver(np.arange(n_tx, dtype=np.int32), N)
    rm = hip.Ratematch(np.arange(n_tx, dtype=np.int32), N)
    sim = hip.Sim(code, 7, n_tx, G=c.G, max_batch=B)
    tiny = 1e-40                                            # a noise variance whose 1 / (2 noise_var) is no float32
    rows = [
        ("bad dimensions", hip.demap, (mod, 0, n_tx, N, s, 0.0, l)),
        ("noise_var must be finite", hip.demap, (mod, B, n_tx, N, s, 0.0, l, 3)),
        ("unknown LLR format", hip.demap, (mod, B, n_tx, N, s + 4, 0.1, l, 3)),
        ("qscale must be finite", hip.demap, (mod, B, n_tx, N, s + 4, 0.1, l, "i8", -1.0)),
        ("8-byte aligned", hip.demap, (mod, B, n_tx, N, s + 4, tiny, l)),
        ("does not fit a float32", hip.demap, (mod, B, n_tx, N, s, tiny, l)),
        ("bad dimensions", hip.demap_il, (mod, il, 0, s, 0.0, l)),
        ("noise_var must be finite", hip.demap_il, (mod, il, B, s, 0.0, l, 3)),
        ("unknown LLR format", hip.demap_il, (mod, il, B, s + 4, 0.1, l, 3)),
        ("8-byte aligned", hip.demap_il, (mod, il, B, s + 4, tiny, l)),
        ("bad dimensions", hip.demap_il_csi, (mod, il, 0, s, g, 0.0, l)),
        ("unknown LLR format", hip.demap_il_csi, (mod, il, B, s, g + 2, 0.1, l, 3)),
        ("gains 4-byte aligned", hip.demap_il_csi, (mod, il, B, s, g + 2, tiny, l)),
        ("bad dimensions", hip.demap_il_apriori, (mod, il, 0, s, None, 0.0, l, l)),
        ("noise_var must be finite", hip.demap_il_apriori, (mod, il, B, s, None, 0.0, l, l)),
        ("unknown LLR format", hip.demap_il_apriori, (mod, il, B, s + 4, None, 0.1, l, l, 3)),
        ("a-priori values 4-byte aligned", hip.demap_il_apriori, (mod, il, B, s + 4, None, tiny, l, l)),
        ("overlaps d_llr", hip.demap_il_apriori, (mod, il, B, s, None, tiny, l, l)),
        ("does not fit a float32", hip.demap_il_apriori, (mod, il, B, s, None, tiny, a, l)),
        ("bad dimensions", hip.demap_rm, (mod, rm, 0, s, None, 0.1, l, "f32", 0.0, 2)),
        ("accumulate must be 0 or 1", hip.demap_rm, (mod, rm, B, s, None, 0.0, l, "f32", 0.0, 2)),
        ("noise_var must be finite", hip.demap_rm, (mod, rm, B, s, None, 0.0, l, 3)),
        ("gains 4-byte aligned", hip.demap_rm, (mod, rm, B, s, g + 2, tiny, l)),
        ("outside 1..", sim.transmit, (mod, 1, 0, 0, float("nan"), s + 4)),
        ("8-byte aligned", sim.transmit, (mod, 1, 0, B, float("nan"), s + 4)),
        ("no finite noise variance", sim.transmit, (mod, 1, 0, B, float("nan"), s)),
        ("outside 1..", sim.generate_mod, (logmap, 1, 0, 0, 2.0, l, 3)),
        ("no fused kernel for the log-MAP rule", sim.generate_mod, (logmap, 1, 0, B, 2.0, l, 3)),
        ("unknown LLR format", sim.generate_mod, (mod, 1, 0, B, 2.0, l + 2, 3)),
        ("aligned to their element", sim.generate_mod, (mod, 1, 0, B, float("nan"), l + 2)),
        ("no finite noise variance > 0", sim.generate_mod, (mod, 1, 0, B, float("nan"), l)),
        ("does not fit a float32", sim.generate_mod, (mod, 1, 0, B, 400.0, l)),
        ("no fused kernel for the log-MAP rule", sim.generate_mod_il, (logmap, None, 1, 0, B, 2.0, l)),
        ("null interleaver", sim.generate_mod_il, (mod, None, 1, 0, B, 2.0, l, 3)),
        ("unknown LLR format", sim.generate_mod_il, (mod, il, 1, 0, B, 2.0, l + 2, 3)),
        ("aligned to their element", sim.generate_mod_il, (mod, il, 1, 0, B, float("nan"), l + 2)),
        ("null interleaver", sim.transmit_il, (mod, None, 1, 0, B, float("nan"), s + 4)),
        ("8-byte aligned", sim.transmit_il, (mod, il, 1, 0, B, float("nan"), s + 4)),
    ]
    for text, fn, args in rows:
        with pytest.raises(hip.LdpcError) as e:
            fn(*args)
        assert e.value.code == (-5 if "log-MAP" in text else -1) and text in str(e.value), (fn.__name__, text, str(e.value))
    torch.cuda.synchronize()
    assert (sym.cpu().numpy() == 777.0).all() and (llr.cpu().numpy() == 777.0).all()          # a refused call writes nothing
    sim.close(); rm.close(); il.close(); logmap.close(); mod.close(); code.close()
