"""CPU: the fading specification (tests/fading_spec.py) against the statistics its gains must have, against the AWGN specifications it
must reduce to with unit gains, against its own float64 formula, and on the double-precision oracle; and the refusals of
ldpc_demap_dev_il_csi that need no device.

The float32-against-float64 bound is the one tests/test_modulation_spec.py derives, 8 u (m0 + m1) inv + one ulp of the result, at
inv = 1 / (2 sigma^2 / a), unchanged.  The one more rounding here, inv_s = fl(inv a), adds u |LLR| <= u (m0 + m1) inv, and the
derivation's first term has that to spare: it needs 5 u (m0 + m1) inv of its 8."""
import ctypes as C
import functools

import numpy as np
import pytest

import ecc_ldpc_amd as E
from oracle import oracle
from tests import fading_spec as fs
from tests import interleaver_spec as ils
from tests import modulation_spec as ms
from tests import product_modulation_spec as ps
from tests.helpers import load

U = 2.0 ** -24
SEED = 0xFAD1E5EED0123


def _moments(K):
    n = 2 ** 16
    ids = np.arange(64, dtype=np.uint64) + np.uint64(2 ** 32 - 32)          # the ids cross 2^32
    a, _ = fs.gains(SEED + int(K), ids, n // 64, 1, K)
    x = a.reshape(-1)
    assert x.size == n
    var = (2.0 * K + 1.0) / (K + 1.0) ** 2
    # the standard error of the sample variance is sqrt((mu4 - var^2) / n).  a / sd^2 is a non-central chi-square of 2 degrees of
    # freedom and non-centrality 2 K: var = 4 (1 + 2 K), mu4 = 96 (1 + 4 K) + 48 (1 + 2 K)^2, so mu4 / var^2 - 1 =
    # 6 (1 + 4 K) / (1 + 2 K)^2 + 2, which is 8 at K = 0 (the exponential) and falls with K
    print(f"K={K}: mean {x.mean():.5f}, variance {x.var():.5f} (model {var:.5f})")
    assert abs(x.mean() - 1.0) <= 5.0 * np.sqrt(var / n)
    assert abs(x.var() - var) <= 5.0 * np.sqrt((6.0 * (1.0 + 4.0 * K) / (1.0 + 2.0 * K) ** 2 + 2.0) * var * var / n)
    return x


def test_gain_draws_rayleigh():
    x = _moments(0.0)
    assert x.min() >= fs.FLOOR
    # exponential with mean 1: the median is ln 2
    assert abs(np.median(x) - np.log(2.0)) <= 5.0 / np.sqrt(x.size)


def test_gain_draws_rician():
    _moments(4.0)


def test_block_structure():
    ids = np.array([7, 8, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 3], np.uint64)
    n_sym = 47
    for K in (0.0, 4.0):
        for block in (1, 2, 3, 5, 47, 54):
            a, unit = fs.gains(SEED, ids, n_sym, block, K)
            assert a.shape == unit.shape == (len(ids), n_sym)
            q = np.arange(n_sym) // block
            for b in range(q.max() + 1):
                assert (a[:, q == b] == a[:, q == b][:, :1]).all()           # constant inside a block
            first = a[:, np.flatnonzero(np.diff(q, prepend=-1))]
            assert first.shape[1] == fs.blocks_per_frame(n_sym, block)
            assert len(np.unique(first)) == first.size                       # differs across blocks and across frames
            if block >= n_sym:
                assert (a == a[:, :1]).all()                                  # one gain per frame
            # (seed, frame) alone: one frame at a time, and the batch in two parts
            for f in range(len(ids)):
                assert np.array_equal(fs.gains(SEED, ids[f:f + 1], n_sym, block, K)[0][0], a[f])
            assert np.array_equal(np.concatenate([fs.gains(SEED, ids[:2], n_sym, block, K)[0], fs.gains(SEED, ids[2:], n_sym, block, K)[0]]), a)
            assert not np.array_equal(fs.gains(SEED + 1, ids, n_sym, block, K)[0], a)
    # the pairing: blocks 2Q and 2Q + 1 are the two halves of one call, and the call is on stream 3, not on the noise's stream 2
    z, rad = fs.block_normals(SEED, ids, 5)
    zn, _ = ms.normals(SEED, ids, 5)
    assert z.shape == zn.shape == (len(ids), 5, 2) and not np.allclose(z, zn)
    assert np.allclose((z ** 2).sum(-1), rad ** 2)


def test_gain_rule_in_float32_and_the_floor():
    rng = np.random.default_rng(1)
    z = rng.normal(0, 1, (2, 4096)).astype(np.float32)
    for K in (0.0, 4.0, 1e6):
        a = fs.gain_rule(z[0], z[1], K)
        assert a.dtype == np.float32
        mu, sd = fs.ricean(K)
        hI, hQ = np.float32(mu + np.float32(sd * z[0, 5])), np.float32(sd * z[1, 5])
        assert a[5] == max(np.float32(np.float32(hI * hI) + np.float32(hQ * hQ)), np.float32(fs.FLOOR))
        assert np.allclose(a, fs.gain_rule(z[0].astype(np.float64), z[1].astype(np.float64), K), rtol=1e-5, atol=1e-7)
    assert fs.ricean(0.0) == (np.float32(0.0), np.float32(np.sqrt(0.5)))
    zero = np.zeros(1, np.float32)                                            # a Box-Muller radius of 0: the floor keeps the sample finite
    assert fs.gain_rule(zero, zero, 0.0)[0] == np.float32(2.0 ** -20)
    assert np.isfinite(fs.sigma_rule(np.float32(0.3), fs.gain_rule(zero, zero, 0.0))).all()
    assert fs.sigma_rule(np.float32(0.3), np.ones(3, np.float32)).tolist() == [np.float32(0.3)] * 3


def _tx_case(m, F=3, n_tx=187, seed=5):
    rng = np.random.default_rng(seed)
    tx = rng.integers(0, 2, (F, n_tx)).astype(np.uint8)
    ids = np.uint64(2 ** 32 - 1) + np.arange(F, dtype=np.uint64)
    return tx, ids, ms.symbols_per_frame(n_tx, m)


def test_transmit_with_unit_gains_is_the_awgn_specification():
    k, db = 100, 3.0
    for pts in (ms.builtin(ms.QPSK), ms.builtin(ms.PSK8), ms.builtin(ms.QAM16), ms.grid64()):
        m = ms.bits_per_symbol(pts)
        tx, ids, ns = _tx_case(m)
        want, unit, sg, nv = ms.transmit(pts, SEED, ids, tx, k, db)
        got, gunit, gsg = fs.transmit(pts, m, SEED, ids, tx, nv, np.ones((len(ids), ns), np.float32))
        assert gsg == sg and np.array_equal(got, want) and np.array_equal(gunit, unit)
    lev = ps.builtin_levels(ps.QAM256)
    tx, ids, ns = _tx_case(8)
    want, unit, sg, nv = ps.transmit(lev, lev, SEED, ids, tx, k, db)
    got, gunit, gsg = fs.transmit(ps.materialise(lev, lev), 8, SEED, ids, tx, nv, np.ones((len(ids), ns), np.float32))
    assert gsg == sg and np.array_equal(got, want) and np.array_equal(gunit, unit)
    # and a gain moves the noise, not the point: (y - c) sqrt(a) is the AWGN noise term
    a, au = fs.gains(SEED, ids, ns, 3, 0.0)
    faded, funit, _ = fs.transmit(ps.materialise(lev, lev), 8, SEED, ids, tx, nv, a, au)
    c = ps.materialise(lev, lev).astype(np.float64)[ms.labels(tx, 8)]
    assert np.allclose((faded - c) * np.sqrt(a)[..., None], want - c, rtol=1e-6, atol=0) and (funit >= unit * np.minimum(1.0, 1.0 / np.sqrt(a))[..., None] * 0.999).all()


def _samples(pts, B, ns, seed):
    rng = np.random.default_rng(seed)
    return (pts[rng.integers(0, len(pts), B * ns)] + rng.normal(0.0, 0.3, (B * ns, 2))).astype(np.float32).reshape(B, ns, 2)


TABLES = {1: lambda: ms.builtin(ms.BPSK), 2: lambda: ms.builtin(ms.QPSK), 3: lambda: ms.builtin(ms.PSK8), 4: lambda: ms.builtin(ms.QAM16),
          5: lambda: ms.rings((1.0, 2.84, 5.27), (4, 12, 16), (np.pi / 4, np.pi / 12, 0.0)), 6: ms.grid64}


def _levels(b, seed):
    rng = np.random.default_rng(seed)
    return np.sort(rng.normal(0, 1, 1 << b)).astype(np.float32)[rng.permutation(1 << b)]


def _table(n_tx, N, seed):
    return np.random.default_rng(seed).permutation(N)[:n_tx].astype(np.int32)


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6])
def test_demapper_with_unit_gains_is_the_interleaved_demapper(m):
    pts = TABLES[m]()
    n_tx, N, B = 187, 203, 3
    ns = ms.symbols_per_frame(n_tx, m)
    pos = _table(n_tx, N, m)
    sym = _samples(pts, B, ns, 10 + m)
    sym[1, 3] = np.nan
    one = np.ones((B, ns), np.float32)
    for fmt in (ms.LLR_F32, ms.LLR_F16, ms.LLR_I8):
        got, want = fs.demap_il_csi(pts, sym, one, pos, N, 0.07, fmt, 2.5), ils.demap_il(pts, sym, pos, N, 0.07, fmt, 2.5)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (m, fmt)


@pytest.mark.parametrize("b", [1, 2, 3, 4, 5, 6])
def test_product_demapper_with_unit_gains_is_the_interleaved_demapper(b):
    li, lq = _levels(b, 20 + b), _levels(b, 30 + b)
    n_tx, N, B = 187, 203, 3
    ns = ms.symbols_per_frame(n_tx, 2 * b)
    pos = _table(n_tx, N, b)
    sym = _samples(ps.materialise(li, lq), B, ns, 40 + b)
    sym[2, 1, 1] = np.nan
    one = np.ones((B, ns), np.float32)
    for fmt in (ms.LLR_F32, ms.LLR_F16, ms.LLR_I8):
        got, want = fs.demap_il_csi_product(li, lq, sym, one, pos, N, 0.07, fmt, 2.5), ils.demap_il_product(li, lq, sym, pos, N, 0.07, fmt, 2.5)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (b, fmt)


def test_demapper_against_float64_at_the_symbol_noise_variance():
    rng = np.random.default_rng(9)
    worst = 0.0
    for nv in (0.09, 1e-3):
        for m in (2, 4, 6):
            pts = TABLES[m]()
            sym = _samples(pts, 1, 1024, m)[0]
            a = rng.uniform(0.01, 8.0, 1024).astype(np.float32)
            got = fs.symbol_llrs(pts, sym, a, nv).astype(np.float64)
            want = np.empty_like(got)
            mag = np.empty_like(got)
            for i in range(1024):                                             # ms.symbol_llrs_f64 takes one noise variance: sample by sample
                want[i], mag[i] = ms.symbol_llrs_f64(pts, sym[i], nv / float(a[i]))
            inv = a.astype(np.float64) / (2.0 * nv)
            bound = 8.0 * U * mag * inv[:, None] + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            worst = max(worst, float((np.abs(got - want) / bound).max()))
            assert (np.abs(got - want) <= bound).all(), (nv, m)
        for b in (2, 5):
            li, lq = _levels(b, 50 + b), _levels(b, 60 + b)
            sym = _samples(ps.materialise(li, lq), 1, 1024, b)[0]
            a = rng.uniform(0.01, 8.0, 1024).astype(np.float32)
            got = fs.symbol_llrs_product(li, lq, sym, a, nv).astype(np.float64)
            for i in range(1024):
                w, g = ps.symbol_llrs_f64(li, lq, sym[i], nv / float(a[i]))
                bound = 8.0 * U * g * float(a[i]) / (2.0 * nv) + np.spacing(np.abs(w).astype(np.float32)).astype(np.float64)
                worst = max(worst, float((np.abs(got[i] - w) / bound).max()))
                assert (np.abs(got[i] - w) <= bound).all(), (nv, b, i)
    print(f"worst |f32 - f64| / bound = {worst:.3f}")


def test_special_gains():
    n_tx, N, B = 23, 29, 2
    pos = _table(n_tx, N, 3)
    hole = ils.holes(pos, N)
    for pts, lev in ((TABLES[3](), None), (None, (_levels(2, 1), _levels(2, 2)))):
        m = 3 if lev is None else 4
        ns = ms.symbols_per_frame(n_tx, m)
        sym = _samples(pts if lev is None else ps.materialise(*lev), B, ns, 77)
        a = np.full((B, ns), 1.5, np.float32)
        a[0, 2], a[1, 4] = 0.0, np.nan
        demap = (lambda fmt: fs.demap_il_csi(pts, sym, a, pos, N, 0.05, fmt)) if lev is None else (lambda fmt: fs.demap_il_csi_product(*lev, sym, a, pos, N, 0.05, fmt))
        f32, f16, i8 = demap(ms.LLR_F32), demap(ms.LLR_F16), demap(ms.LLR_I8)
        e0, en = pos[m * 2:m * 3], pos[m * 4:m * 5]
        assert (f32[0, e0] == 0).all() and (f16[0, e0] == 0).all() and (i8[0, e0] == 0).all()                 # an erasure
        assert np.isnan(f32[1, en]).all() and np.isnan(f16[1, en]).all() and (i8[1, en] == 0).all()
        rest = np.ones((B, N), bool)
        rest[0, e0] = rest[1, en] = False
        rest[:, hole] = False
        assert np.isfinite(f32[rest]).all() and (f32[rest] != 0).all() and (f32[:, hole] == 0).all()


# ---- the chain on the oracle
CHAIN_DB, CHAIN_FRAMES, CHAIN_SEED = 14.0, 64, 0xFAD1E5EED0123


@functools.lru_cache(maxsize=None)
def chain_llrs(db=CHAIN_DB, F=CHAIN_FRAMES, seed=CHAIN_SEED, first=0):
    """jpl.1024.4.5, the 16QAM built-in, the block table of 320 x 4, block = 1, K = 0: -> (messages [F][k], LLRs weighted per symbol
    [F][N], LLRs with one scale [F][N]), the spec's own Philox draws.  Shared with tests/test_fading_gpu.py (the point)"""
    c = load("jpl.1024.4.5")
    pts = ms.builtin(ms.QAM16)
    pos = ils.block_positions(320, 4)
    assert len(pos) == c.n_tx == 1280
    ids = np.uint64(first) + np.arange(F, dtype=np.uint64)
    from oracle import frame_source
    msg = frame_source.message_bits(seed, ids, c.k)
    cw = np.stack([c.encode(w) for w in msg])
    tx = ils.interleave(cw, pos)[:, :c.n_tx]
    nv = ms.noise_var(c.k, c.n_tx, pts, db)
    a, _ = fs.gains(seed, ids, 320, 1, 0.0)
    y, _, _ = fs.transmit(pts, 4, seed, ids, tx, nv, a)
    sym, a32 = y.astype(np.float32), a.astype(np.float32)
    return msg, fs.demap_il_csi(pts, sym, a32, pos, c.N, nv), ils.demap_il(pts, sym, pos, c.N, nv)


@pytest.mark.parametrize("rule", ["min", "tanh"])
def test_chain_on_the_oracle(rule):
    """measured with numpy's generator (the issue): 0 frame errors of 64 weighted per symbol, 33 .. 59 with one scale, over twelve seeds"""
    c = load("jpl.1024.4.5")
    msg, csi, flat = chain_llrs()
    errs = {}
    for name, llr in (("per-symbol weights", csi), ("one scale", flat)):
        bits, its, _ = oracle.decode_batch(c.graph, rule, 50, llr.astype(np.float64), nthreads=4)
        fe = int((bits[:, :c.k] != msg).any(axis=1).sum())
        print(f"{rule}, {name}: {fe} frame errors of {len(msg)} at {CHAIN_DB} dB, mean iterations {its.mean():.1f}")
        errs[name] = fe
    assert errs["per-symbol weights"] <= 3
    assert errs["one scale"] >= 16


# ---- the library, no device
def test_demap_il_csi_refusals_need_no_device():
    """null and misaligned arguments are LDPC_EINVAL before the device is looked at (no ldpc_init here; an interleaver object cannot
    exist without a device, so its pointer is a stand-in that the refusals never follow)"""
    L = E.lib()
    assert "ldpc_demap_dev_il_csi" in E.ABI_SYMBOLS and "ldpc_sim_transmit_il_fading" in E.ABI_SYMBOLS and "ldpc_sim_generate_mod_il_fading" in E.ABI_SYMBOLS
    mod = E.Modulation("16qam")
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    il = C.c_void_p(p)
    call = lambda mo, i, B, sym, gain, nv, llr, fmt, qs: L.ldpc_demap_dev_il_csi(mo, i, B, sym, gain, nv, llr, fmt, qs, None)
    cases = {
        "null mod": (None, il, 2, p, p, 0.1, p, 0, 0.0), "null table": (mod._h, None, 2, p, p, 0.1, p, 0, 0.0),
        "null samples": (mod._h, il, 2, None, p, 0.1, p, 0, 0.0), "null gains": (mod._h, il, 2, p, None, 0.1, p, 0, 0.0),
        "null LLRs": (mod._h, il, 2, p, p, 0.1, None, 0, 0.0), "samples at 4": (mod._h, il, 2, p + 4, p, 0.1, p, 0, 0.0),
        "gains at 2": (mod._h, il, 2, p, p + 2, 0.1, p, 0, 0.0), "gains at 1": (mod._h, il, 2, p, p + 1, 0.1, p, 1, 0.0),
        "LLRs at 2": (mod._h, il, 2, p, p, 0.1, p + 2, 0, 0.0), "fp16 LLRs at 1": (mod._h, il, 2, p, p, 0.1, p + 1, 1, 0.0),
        "batch 0": (mod._h, il, 0, p, p, 0.1, p, 0, 0.0), "format 3": (mod._h, il, 2, p, p, 0.1, p, 3, 0.0),
        "noise_var 0": (mod._h, il, 2, p, p, 0.0, p, 0, 0.0), "noise_var NaN": (mod._h, il, 2, p, p, float("nan"), p, 0, 0.0),
        "noise_var 1e-40": (mod._h, il, 2, p, p, 1e-40, p, 0, 0.0), "qscale -1": (mod._h, il, 2, p, p, 0.1, p, 2, -1.0),
    }
    for what, args in cases.items():
        assert call(*args) == E.EINVAL, what
        assert L.ldpc_last_error_code() == E.EINVAL, what
    assert (buf == 0).all()
    mod.close()
    # the descriptor: ldpc_fading's three fields
    fad = E.Fading(32, 4.0)
    assert (fad.block, fad.k_factor) == (32, 4.0) and fad.struct.struct_size == C.sizeof(fad.struct) == C.sizeof(C.c_size_t) + 8
