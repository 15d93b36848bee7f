"""Specification of the modulation object, the max-log soft demapper and the modulated path of the frame source
(include/ldpc_hip.h ldpc_modulation_*, ldpc_demap_dev, ldpc_sim_transmit, ldpc_sim_generate_mod; csrc/demap.h): numpy, float32
operation by operation.  The library is built without contraction, so the device kernels reproduce demap() bit for bit
(tests/test_modulation_gpu.py).

Labelling      symbol s of a frame carries codeword bits m s .. m s + m - 1; label = sum_j bit(m s + j) << (m - 1 - j) (the first bit is
               the MSB); bits at positions >= n_tx pad as 0; the label is the index into the table points[2^m][2] (I, Q).
Built-ins      BPSK  b -> (2b - 1, 0);  QPSK  (b0, b1) -> ((2 b0 - 1) h, (2 b1 - 1) h), h = float32(sqrt 1/2);
               8PSK  the point at angle k pi / 4 carries the label k ^ (k >> 1) (Gray around the circle), coordinates from {0, +-h, +-1};
               16QAM (b0 b1 | b2 b3) -> (L[b0 b1], L[b2 b3]) a, L = (-3, -1, +3, +1) (Gray per axis), a = 1 / sqrt 10, each level
               rounded to float32 once.  No claim that these are any standard's labellings.
Energy         Es = (sum_p I_p^2 + Q_p^2) / 2^m, in double, in index order.
Noise variance sigma^2 = Es / (2 R m 10^(dB/10)) per real dimension, R = k / n_tx, in double.
Demapper       inv = float32(1 / (2 sigma^2)) rounded once from the double; for a sample (yI, yQ) and every point p
                 dx = yI - I_p, dy = yQ - Q_p, d_p = fl(fl(dx dx) + fl(dy dy))
                 m0_j / m1_j = min of d_p over the labels whose bit j (MSB first) is 0 / 1   (a min of floats is exact: any order)
                 LLR_j = fl(fl(m0_j - m1_j) inv)                                               (LLR > 0 <=> bit 1)
               A NaN sample makes every d_p NaN and so every LLR.
Outputs        [batch][N]: position n < n_tx = LLR (n % m) of symbol n / m; positions n_tx .. N - 1 are 0; LLRs of pad bits are dropped.
               f32 as it is; fp16 = round_f16 (clamp to +-65504, round to nearest even; NaN stays NaN);
               int8 = tests/layered_i8_spec.quantize (clip(rint(LLR qscale), -127, 127), NaN -> 0).
Channel        symbol pair g = symbols 2g, 2g + 1: one Philox4x32-10 call, counter (frame lo, frame hi, g, stream 2); the uniforms and
               Box-Muller of the BPSK source (oracle/frame_source.py): (r0, r1) -> I, Q of symbol 2g, (r2, r3) -> I, Q of symbol 2g + 1;
               y = fl(c + fl(sg z)), sg = float32(sqrt sigma^2).  Here z is float64 (the device's logf / sqrtf / sincospif are what the
               GPU test's tolerance is about).
"""
import numpy as np

from oracle import frame_source
from tests import layered_i8_spec

BPSK, QPSK, PSK8, QAM16 = 1, 2, 3, 4
LLR_F32, LLR_F16, LLR_I8 = 0, 1, 2
NOISE_STREAM = 2


def builtin(kind):
    """-> points [2^m][2] float32"""
    h = np.float32(np.sqrt(0.5))
    if kind == BPSK:
        return np.array([[-1, 0], [1, 0]], np.float32)
    if kind == QPSK:
        return np.array([[(2 * (p >> 1) - 1) * h, (2 * (p & 1) - 1) * h] for p in range(4)], np.float32)
    if kind == PSK8:
        ring = [(1, 0), (h, h), (0, 1), (-h, h), (-1, 0), (-h, -h), (0, -1), (h, -h)]
        pts = np.zeros((8, 2), np.float32)
        for k, c in enumerate(ring):
            pts[k ^ (k >> 1)] = c
        return pts
    if kind == QAM16:
        lev = [np.float32(v / np.sqrt(10.0)) for v in (-3.0, -1.0, 3.0, 1.0)]
        return np.array([[lev[p >> 2], lev[p & 3]] for p in range(16)], np.float32)
    raise ValueError(kind)


def rings(radii, counts, phases):
    """an APSK-style table: ring r holds counts[r] points of radius radii[r] from angle phases[r] on, labels in ring order, scaled to
    unit energy in double and rounded to float32 once -> [sum counts][2] float32 (sum counts must be a power of two)"""
    pts = []
    for R, n, ph in zip(radii, counts, phases):
        for i in range(n):
            a = ph + 2.0 * np.pi * i / n
            pts.append((R * np.cos(a), R * np.sin(a)))
    pts = np.array(pts, np.float64)
    pts[np.abs(pts) < 1e-12] = 0.0                       # cos(pi / 2) and its kin: on the axis, not 6e-17 off it
    assert pts.shape[0] & (pts.shape[0] - 1) == 0
    return (pts / np.sqrt((pts ** 2).sum() / pts.shape[0])).astype(np.float32)


def grid64():
    """an 8 x 8 grid, natural labels (row = the high three bits), unit energy"""
    lev = (np.arange(8) * 2.0 - 7.0) / np.sqrt(42.0)
    return np.array([[lev[p >> 3], lev[p & 7]] for p in range(64)], np.float64).astype(np.float32)


def bits_per_symbol(points):
    n = np.asarray(points).shape[0]
    m = n.bit_length() - 1
    assert 1 <= m <= 6 and n == 1 << m and np.asarray(points).shape[1] == 2
    return m


def energy(points):
    acc = 0.0
    for i, q in np.asarray(points, np.float32).astype(np.float64):
        acc += i * i + q * q
    return acc / len(points)


def symbols_per_frame(n_tx, m):
    return (n_tx + m - 1) // m


def noise_var(k, n_tx, points, ebn0_db):
    m = bits_per_symbol(points)
    return energy(points) / (2.0 * (k / n_tx) * float(m) * 10.0 ** (ebn0_db / 10.0))


def labels(codewords, m):
    """codewords [F][n_tx] 0/1 -> labels [F][n_sym]"""
    cw = np.asarray(codewords).astype(np.int64)
    F, n_tx = cw.shape
    ns = symbols_per_frame(n_tx, m)
    pad = np.zeros((F, ns * m), np.int64)
    pad[:, :n_tx] = cw
    return (pad.reshape(F, ns, m) << (m - 1 - np.arange(m))).sum(axis=2)


def symbol_llrs(points, sym, nv):
    """sym [..., 2] float32 -> LLRs [..., m] float32: the demapper's rule, one float32 operation at a time"""
    pts = np.asarray(points, np.float32)
    m = bits_per_symbol(pts)
    sym = np.asarray(sym, np.float32)
    inv = np.float32(1.0 / (2.0 * float(nv)))
    with np.errstate(invalid="ignore", over="ignore"):
        dx = sym[..., None, 0] - pts[:, 0]
        dy = sym[..., None, 1] - pts[:, 1]
        d = dx * dx + dy * dy                                  # float32: both products round, then the sum
        assert d.dtype == np.float32
        out = np.empty(sym.shape[:-1] + (m,), np.float32)
        lab = np.arange(1 << m)
        for j in range(m):
            one = ((lab >> (m - 1 - j)) & 1).astype(bool)
            m0, m1 = np.minimum.reduce(d[..., ~one], axis=-1), np.minimum.reduce(d[..., one], axis=-1)
            out[..., j] = (m0 - m1) * inv
    return out


def symbol_llrs_f64(points, sym, nv):
    """the same formula in float64 on the same float32 inputs -> (LLRs [..., m], m0 + m1 [..., m])"""
    pts = np.asarray(points, np.float32).astype(np.float64)
    m = bits_per_symbol(pts)
    sym = np.asarray(sym, np.float32).astype(np.float64)
    inv = 1.0 / (2.0 * float(nv))
    d = (sym[..., None, 0] - pts[:, 0]) ** 2 + (sym[..., None, 1] - pts[:, 1]) ** 2
    out, mag = np.empty(sym.shape[:-1] + (m,)), np.empty(sym.shape[:-1] + (m,))
    lab = np.arange(1 << m)
    for j in range(m):
        one = ((lab >> (m - 1 - j)) & 1).astype(bool)
        m0, m1 = d[..., ~one].min(axis=-1), d[..., one].min(axis=-1)
        out[..., j], mag[..., j] = (m0 - m1) * inv, m0 + m1
    return out, mag


def round_f16(x):
    with np.errstate(invalid="ignore"):
        return np.clip(np.asarray(x, np.float32), np.float32(-65504.0), np.float32(65504.0)).astype(np.float16)


def demap(points, sym, n_tx, N, nv, fmt=LLR_F32, qscale=4.0):
    """sym [B][n_sym][2] float32 -> [B][N] float32 / float16 / int8"""
    m = bits_per_symbol(points)
    sym = np.asarray(sym, np.float32)
    B, ns = sym.shape[:2]
    assert ns == symbols_per_frame(n_tx, m) and n_tx <= N
    llr = np.zeros((B, N), np.float32)
    llr[:, :n_tx] = symbol_llrs(points, sym, nv).reshape(B, ns * m)[:, :n_tx]
    if fmt == LLR_F32:
        return llr
    if fmt == LLR_F16:
        return round_f16(llr)
    return layered_i8_spec.quantize(llr, qscale).astype(np.int8)


def normals(seed, frame_ids, n_sym):
    """-> (z [F][n_sym][2] float64: the I and Q normals of every symbol, radius [F][n_sym]: the Box-Muller radius of its pair half)"""
    flo, fhi, klo, khi = frame_source._split(seed, frame_ids)
    pairs = (n_sym + 1) // 2
    g = np.arange(pairs, dtype=np.uint64)
    r = frame_source.philox4x32_10((flo[:, None], fhi[:, None], g[None, :], NOISE_STREAM), (klo, khi))
    rf = r.astype(np.float32)
    one, s = np.float32(1.0), np.float32(2.0 ** -32)
    ua, ub = ((rf[0] + one) * s).astype(np.float64), (rf[1] * s).astype(np.float64)
    uc, ud = ((rf[2] + one) * s).astype(np.float64), (rf[3] * s).astype(np.float64)
    ra, rc = np.sqrt(-2.0 * np.log(ua)), np.sqrt(-2.0 * np.log(uc))
    ta, tc = 2.0 * np.pi * ub, 2.0 * np.pi * ud
    z = np.stack([ra * np.cos(ta), ra * np.sin(ta), rc * np.cos(tc), rc * np.sin(tc)], axis=-1)    # [F][pairs][4]
    rad = np.stack([ra, rc], axis=-1)
    F = flo.shape[0]
    return z.reshape(F, 2 * pairs, 2)[:, :n_sym], rad.reshape(F, 2 * pairs)[:, :n_sym]


def transmit(points, seed, frame_ids, codewords, k, ebn0_db):
    """codewords [F][n_tx] -> (y [F][n_sym][2] float64 = c + sg z, bound unit [F][n_sym][2] = |c| + sg radius per coordinate, sg, sigma^2)"""
    pts = np.asarray(points, np.float32).astype(np.float64)
    m = bits_per_symbol(pts)
    n_tx = np.asarray(codewords).shape[1]
    nv = noise_var(k, n_tx, points, ebn0_db)
    sg = float(np.float32(np.sqrt(nv)))
    lab = labels(codewords, m)
    z, rad = normals(seed, frame_ids, lab.shape[1])
    c = pts[lab]
    return c + sg * z, np.abs(c) + sg * rad[..., None], sg, nv
