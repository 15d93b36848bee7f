"""CPU: the modulation specification (tests/modulation_spec.py) against its own float64 formula and against the properties a
demapper must have, and the host-only modulation object of the built library (ldpc_modulation_*; no GPU needed).

The float32-against-float64 bound: each d_p carries at most 3 roundings (two products, one sum), the difference and the product with
inv one each; with u = 2^-24 the absolute error of LLR_j is at most about (3 u (m0 + m1) + u |m0 - m1|) inv + u |LLR| <= 8 u (m0 + m1) inv,
plus one ulp of the result for the rounding of inv itself (float32(1 / (2 sigma^2)) against the double)."""
import ctypes as C

import numpy as np
import pytest

import ecc_ldpc_amd as E
from oracle import frame_source
from tests import layered_i8_spec
from tests import modulation_spec as ms

U = 2.0 ** -24
TABLES = {
    "bpsk": lambda: ms.builtin(ms.BPSK), "qpsk": lambda: ms.builtin(ms.QPSK), "8psk": lambda: ms.builtin(ms.PSK8), "16qam": lambda: ms.builtin(ms.QAM16),
    "apsk16": lambda: ms.rings((1.0, 3.15), (4, 12), (np.pi / 4, np.pi / 12)),
    "apsk32": lambda: ms.rings((1.0, 2.84, 5.27), (4, 12, 16), (np.pi / 4, np.pi / 12, 0.0)),
    "grid64": ms.grid64,
}


def _samples(pts, n, seed, spread=0.3):
    rng = np.random.default_rng(seed)
    return (pts[rng.integers(0, len(pts), n)] + rng.normal(0.0, spread, (n, 2))).astype(np.float32)


@pytest.mark.parametrize("kind", [ms.BPSK, ms.QPSK, ms.PSK8, ms.QAM16])
def test_builtin_unit_energy_and_gray(kind):
    pts = ms.builtin(kind)
    m = ms.bits_per_symbol(pts)
    assert m == kind
    es = ms.energy(pts)
    print(f"kind {kind}: Es - 1 = {es - 1.0:.3e}")
    assert abs(es - 1.0) <= 1e-7
    # Gray: every nearest neighbour of a point differs from it in exactly one label bit
    p64 = pts.astype(np.float64)
    d = ((p64[:, None, :] - p64[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    for a in range(len(pts)):
        near = np.flatnonzero(d[a] <= d[a].min() * (1.0 + 1e-6))
        assert len(near) >= 1
        for b in near:
            assert bin(a ^ int(b)).count("1") == 1, (kind, a, int(b))


@pytest.mark.parametrize("name", list(TABLES))
def test_spec_against_float64(name):
    pts = TABLES[name]()
    m = ms.bits_per_symbol(pts)
    worst = 0.0
    for nv, spread, scale in ((0.09, 0.3, 1.0), (1e-3, 0.3, 1.0), (0.5, 1.0, 1.0), (1e-3, 0.3, 1e3)):
        y = _samples(pts, 4096, 17 + m, spread) * np.float32(scale)
        got = ms.symbol_llrs(pts, y, nv).astype(np.float64)
        want, mag = ms.symbol_llrs_f64(pts, y, nv)
        inv = 1.0 / (2.0 * nv)
        bound = 8.0 * U * mag * inv + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        worst = max(worst, float((np.abs(got - want) / bound).max()))
        assert (np.abs(got - want) <= bound).all()
    print(f"{name}: worst |f32 - f64| / bound = {worst:.3f}")


def test_bpsk_is_2y_over_sigma2():
    pts = ms.builtin(ms.BPSK)
    rng = np.random.default_rng(3)
    y = np.zeros((4096, 2), np.float32)
    y[:, 0] = rng.normal(0.0, 1.5, 4096)
    y[:, 1] = rng.normal(0.0, 1.5, 4096)               # Q carries nothing: it enters both distances alike
    for nv in (0.7, 0.05):
        got = ms.symbol_llrs(pts, y, nv)[:, 0].astype(np.float64)
        y64 = y.astype(np.float64)
        want = 2.0 * y64[:, 0] / nv
        mag = (y64[:, 0] + 1.0) ** 2 + (y64[:, 0] - 1.0) ** 2 + 2.0 * y64[:, 1] ** 2
        bound = 8.0 * U * mag / (2.0 * nv) + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (np.abs(got - want) <= bound).all()
        assert ((got > 0) == (y[:, 0] > 0)).all() or (np.abs(want[(got > 0) != (y[:, 0] > 0)]) <= bound[(got > 0) != (y[:, 0] > 0)]).all()


def test_qpsk_bit0_does_not_depend_on_q():
    """exactly so in the float64 formula; in float32 the common term min(dy^2) rounds into both sums, so the two LLRs agree within the
    sum of their two bounds"""
    pts = ms.builtin(ms.QPSK)
    rng = np.random.default_rng(5)
    yi = rng.normal(0.0, 1.0, 2048).astype(np.float32)
    a = np.stack([yi, rng.normal(0.0, 1.0, 2048).astype(np.float32)], axis=1)
    b = np.stack([yi, rng.normal(0.0, 1.0, 2048).astype(np.float32)], axis=1)
    nv = 0.2
    wa, ma = ms.symbol_llrs_f64(pts, a, nv)
    wb, mb = ms.symbol_llrs_f64(pts, b, nv)
    assert np.allclose(wa[:, 0], wb[:, 0], rtol=0, atol=1e-12 * (ma[:, 0] + mb[:, 0]) / (2 * nv))
    assert not np.allclose(wa[:, 1], wb[:, 1])
    ga, gb = ms.symbol_llrs(pts, a, nv).astype(np.float64), ms.symbol_llrs(pts, b, nv).astype(np.float64)
    inv = 1.0 / (2.0 * nv)
    bound = 8.0 * U * (ma[:, 0] + mb[:, 0]) * inv + 2.0 * np.spacing(np.abs(wa[:, 0]).astype(np.float32)).astype(np.float64)
    assert (np.abs(ga[:, 0] - gb[:, 0]) <= bound).all()
    # with Q held, the float32 LLR of bit 0 is a function of I alone, bit for bit
    c = np.stack([yi, np.full(2048, a[0, 1], np.float32)], axis=1)
    d = np.stack([yi[::-1].copy(), np.full(2048, a[0, 1], np.float32)], axis=1)
    assert np.array_equal(ms.symbol_llrs(pts, c, nv)[:, 0].view(np.uint32), ms.symbol_llrs(pts, d, nv)[::-1, 0].view(np.uint32))


@pytest.mark.parametrize("name", list(TABLES))
def test_sample_on_a_point_and_equidistant(name):
    pts = TABLES[name]()
    m = ms.bits_per_symbol(pts)
    nv = 0.05
    llr = ms.symbol_llrs(pts, pts, nv)                 # sample p exactly on point p: d_p = 0, the other class is strictly farther
    for p in range(len(pts)):
        twins = [q for q in range(len(pts)) if q != p and np.array_equal(pts[q], pts[p])]
        assert not twins
        for j in range(m):
            bit = (p >> (m - 1 - j)) & 1
            assert (llr[p, j] > 0) == bool(bit) and llr[p, j] != 0
            other = [q for q in range(len(pts)) if ((q >> (m - 1 - j)) & 1) != bit]
            d = ((pts[other].astype(np.float32) - pts[p]) ** 2).astype(np.float32)
            want = (np.float32(d[:, 0] + d[:, 1]).min()) * np.float32(1.0 / (2.0 * nv))
            assert np.float32(abs(llr[p, j])) == np.float32(want)


def test_equidistant_sample_gives_exact_zero():
    # BPSK on the Q axis; QPSK on an axis: bit 0 is undecided on the Q axis (I = 0), bit 1 on the I axis
    for y in ((0.0, 0.7), (0.0, -3.0), (0.0, 0.0)):
        assert ms.symbol_llrs(ms.builtin(ms.BPSK), np.array([y], np.float32), 0.3)[0, 0] == 0.0
    q = ms.builtin(ms.QPSK)
    l = ms.symbol_llrs(q, np.array([[0.0, 0.4], [0.9, 0.0]], np.float32), 0.3)
    assert l[0, 0] == 0.0 and l[0, 1] > 0 and l[1, 1] == 0.0 and l[1, 0] > 0
    # 16QAM: I = 0 leaves the sign bit of the I axis undecided
    g = ms.builtin(ms.QAM16)
    l = ms.symbol_llrs(g, np.array([[0.0, 0.2]], np.float32), 0.1)
    assert l[0, 0] == 0.0 and l[0, 1] != 0.0
    # a table with two equal points of different labels: bit 0 can never be told
    twin = np.array([[0.5, 0.5], [0.5, 0.5]], np.float32)
    assert (ms.symbol_llrs(twin, _samples(twin, 64, 1), 0.2) == 0.0).all()


def test_outputs_and_tail():
    pts = ms.builtin(ms.PSK8)
    n_tx, N, B = 16, 25, 3                              # 6 symbols, the last one with two pad bits; a tail of 9 zeros
    sym = _samples(pts, B * 6, 9).reshape(B, 6, 2)
    sym[1, 2] = np.nan
    sym[2] *= np.float32(1e3)
    nv = 1e-3
    f = ms.demap(pts, sym, n_tx, N, nv)
    assert f.dtype == np.float32 and (f[:, n_tx:].view(np.uint32) == 0).all()
    per = ms.symbol_llrs(pts, sym, nv).reshape(B, 18)
    assert np.array_equal(f[:, :n_tx].view(np.uint32), per[:, :n_tx].view(np.uint32))
    assert np.isnan(f[1, 6:9]).all() and np.isfinite(f[1, :6]).all() and np.isfinite(f[1, 9:]).all()
    for qs in (4.0, 2.5):
        q = ms.demap(pts, sym, n_tx, N, nv, ms.LLR_I8, qs)
        assert q.dtype == np.int8 and np.array_equal(q.astype(np.int32), layered_i8_spec.quantize(f, qs))
        assert (q[1, 6:9] == 0).all() and np.abs(q[2, :n_tx]).max() == 127 and q.min() >= -127
    h = ms.demap(pts, sym, n_tx, N, nv, ms.LLR_F16)
    assert h.dtype == np.float16 and np.isnan(h[1, 6:9]).all() and np.abs(h[2, :n_tx].astype(np.float32)).max() == 65504.0
    assert np.isfinite(h[2]).all()


def test_labels():
    cw = np.array([[1, 0, 1, 1, 0, 0, 1]], np.uint8)
    assert ms.labels(cw, 3).tolist() == [[0b101, 0b100, 0b100]]        # the first bit is the MSB; the last symbol pads with zeros
    assert ms.labels(cw, 1).tolist() == [cw[0].tolist()]
    assert ms.symbols_per_frame(7, 3) == 3 and ms.symbols_per_frame(6, 3) == 2


def test_noise_stream_2_statistics():
    """stream 2 of the Philox counter: 2^18 normals, mean and variance within 5 standard errors; and it is not stream 1"""
    F, ns = 64, 2048                                    # 64 frames x 2048 symbols x 2 = 2^18 samples
    ids = np.arange(F, dtype=np.uint64) + np.uint64(2 ** 32 + 5)
    z, rad = ms.normals(0xC0FFEE1234567, ids, ns)
    assert z.shape == (F, ns, 2) and rad.shape == (F, ns)
    x = z.reshape(-1)
    n = x.size
    assert n == 2 ** 18
    assert abs(x.mean()) <= 5.0 / np.sqrt(n)
    assert abs(x.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert abs((z[..., 0] * z[..., 1]).mean()) <= 5.0 / np.sqrt(n / 2)
    r = frame_source.philox4x32_10((5, 1, 0, ms.NOISE_STREAM), (0xC0FFEE1234567 & 0xFFFFFFFF, 0xC0FFEE1234567 >> 32))        # frame 2^32 + 5 = (lo 5, hi 1)
    z0, _ = ms.normals(0xC0FFEE1234567, ids[:1], 2)
    rf = r.astype(np.float32)
    ua, ub = float((rf[0] + np.float32(1)) * np.float32(2.0 ** -32)), float(rf[1] * np.float32(2.0 ** -32))
    assert np.isclose(z0[0, 0, 0], np.sqrt(-2 * np.log(ua)) * np.cos(2 * np.pi * ub)) and np.isclose(z0[0, 0, 1], np.sqrt(-2 * np.log(ua)) * np.sin(2 * np.pi * ub))
    z1, _ = frame_source.normals(0xC0FFEE1234567, ids[:1], 4)
    assert not np.allclose(z0.reshape(-1), z1.reshape(-1))


def test_noise_var_is_the_bpsk_formula():
    for k, n_tx, db in ((7, 13, 2.0), (1280, 1920, 4.0), (7200, 16200, -1.5)):
        assert ms.noise_var(k, n_tx, ms.builtin(ms.BPSK), db) == 1.0 / (2.0 * (k / n_tx) * 10.0 ** (db / 10.0))
    q = ms.builtin(ms.QPSK)
    assert np.isclose(ms.noise_var(1, 2, q, 0.0), ms.energy(q) / 2.0)


def test_modulation_object_of_the_library():
    """host only: needs the built library, not a GPU.  Fails on a library without ldpc_modulation_*"""
    for name, kind in (("bpsk", ms.BPSK), ("qpsk", ms.QPSK), ("8psk", ms.PSK8), ("16qam", ms.QAM16)):
        mod = E.Modulation(name)
        want = ms.builtin(kind)
        assert mod.bits == kind and np.array_equal(mod.points.view(np.uint32), want.view(np.uint32)), name
        assert mod.energy == ms.energy(want)
        mod.close()
    for name in ("apsk16", "apsk32", "grid64"):
        pts = TABLES[name]()
        mod = E.Modulation(pts)
        m = ms.bits_per_symbol(pts)
        assert mod.bits == m and np.array_equal(mod.points.view(np.uint32), pts.view(np.uint32))
        assert mod.energy == ms.energy(pts) and abs(mod.energy - 1.0) < 1e-6
        for n_tx in (0, 1, m, m + 1, 1917, 1920):
            assert mod.symbols(n_tx) == ms.symbols_per_frame(n_tx, m)
        mod.close()
    twin = E.Modulation(np.array([[0.5, 0.5], [0.5, 0.5]], np.float32))      # two equal points are allowed
    assert twin.bits == 1 and twin.energy == 0.5
    twin.close()
    L = E.lib()
    ok = np.zeros((128, 2), np.float32)
    fp = ok.ctypes.data_as(C.POINTER(C.c_float))
    for m in (0, 7, -1):
        assert not L.ldpc_modulation_create(m, fp) and L.ldpc_last_error_code() == -1
    assert not L.ldpc_modulation_create(2, None) and L.ldpc_last_error_code() == -1
    for bad in (np.nan, np.inf, -np.inf):
        pts = ms.builtin(ms.QPSK).copy()
        pts[3, 1] = bad
        with pytest.raises(E.LdpcError) as e:
            E.Modulation(pts)
        assert e.value.code == -1
        pts = np.zeros((4, 2), np.float32)
        pts[0, 0] = bad                                   # only the first 2^m points are read: a bad value past them is not seen
        big = np.concatenate([ms.builtin(ms.BPSK), pts])
        h = L.ldpc_modulation_create(1, big.ctypes.data_as(C.POINTER(C.c_float)))
        assert h
        L.ldpc_modulation_destroy(h)
    for kind in (0, 5, -3):
        assert not L.ldpc_modulation_create_builtin(kind) and L.ldpc_last_error_code() == -1
    assert L.ldpc_modulation_bits(None) == -1 and L.ldpc_modulation_points(None, fp) == -1 and L.ldpc_modulation_symbols(None, 4) == -1
    mod = E.Modulation("qpsk")
    assert L.ldpc_modulation_symbols(mod._h, -1) == -1 and L.ldpc_modulation_points(mod._h, None) == 4
    mod.close()
