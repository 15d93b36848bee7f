"""Specification of product constellations (include/ldpc_hip.h ldpc_modulation_create_product, the built-ins LDPC_MOD_64QAM ..
LDPC_MOD_4096QAM; csrc/demap_product.h): numpy, float32 operation by operation.  What it shares with table objects -- the labelling, the
energy rule, the output formats, the channel's normals -- comes from tests/modulation_spec.py.  The library is built without
contraction, so the device kernels reproduce demap() bit for bit (tests/test_product_modulation_gpu.py).

Object         b = 1..6 bits an axis, m = 2 b bits per symbol; two level sets levels_i, levels_q [2^b] float32.  Of a symbol's m bits
               (the first one the MSB) the first b are the index iI into levels_i, the next b the index iQ into levels_q:
               label = (iI << b) | iQ, point = (levels_i[iI], levels_q[iQ]).  The materialised table is that for every label.
Built-ins      64QAM, 256QAM, 1024QAM, 4096QAM (b = 3, 4, 5, 6), both axes: position k = 0 .. 2^b - 1 has amplitude
               (2k - (2^b - 1)) / sqrt(2 (4^b - 1) / 3) and carries the label k ^ (k >> 1) (binary-reflected Gray); each level computed
               in double and rounded to float32 once.  No claim that these are any standard's labellings.
Energy         modulation_spec.energy of the materialised table: double, index order.
Noise variance sigma^2 = Es / (2 R m 10^(dB/10)), R = k / n_tx, in double.
Demapper       inv = float32(1 / (2 sigma^2)); for a sample (yI, yQ) and each axis A in {I, Q} with levels a_l
                 dx_l = fl(y_A - a_l), e_l = fl(dx_l dx_l)
                 m0_j / m1_j = min of e_l over the axis labels l whose bit j (MSB first, j = 0 .. b - 1) is 0 / 1
                 LLR_j = fl(fl(m0_j - m1_j) inv)
               Output element m s + j is I-bit j of symbol s, element m s + b + j its Q-bit j.  A NaN coordinate makes the b LLRs of its
               own axis NaN and leaves the other axis's as they are (the table rule makes all m NaN).
Relation       fl is monotone, so on the materialised table min_p fl(ex_i + ey_q) = fl(min ex + min ey): with E = the smallest e of the
               other axis, modulation_spec.symbol_llrs gives exactly fl(fl(fl(m0_j + E) - fl(m1_j + E)) inv) (two_d_from_axes below).
Outputs, channel: as modulation_spec (demap's zero tail and formats; normals(); y = fl(c + fl(sg z)))."""
import numpy as np

from tests import layered_i8_spec
from tests import modulation_spec as ms

QAM64, QAM256, QAM1024, QAM4096 = 6, 8, 10, 12
LLR_F32, LLR_F16, LLR_I8 = ms.LLR_F32, ms.LLR_F16, ms.LLR_I8


def builtin_levels(kind):
    """-> levels [2^b] float32 (both axes), b = kind / 2"""
    assert kind in (QAM64, QAM256, QAM1024, QAM4096) or kind == 4        # (4: the level set of the 16QAM table built-in)
    b = kind // 2
    n = 1 << b
    norm = np.sqrt(2.0 * float(n * n - 1) / 3.0)
    lev = np.zeros(n, np.float32)
    for k in range(n):
        lev[k ^ (k >> 1)] = np.float32(float(2 * k - (n - 1)) / norm)
    return lev


def bits_per_axis(levels_i, levels_q):
    li, lq = np.asarray(levels_i), np.asarray(levels_q)
    n = li.shape[0]
    b = n.bit_length() - 1
    assert li.ndim == 1 and li.shape == lq.shape and 1 <= b <= 6 and n == 1 << b
    return b


def materialise(levels_i, levels_q):
    """-> points [4^b][2] float32, pt[(iI << b) | iQ] = (levels_i[iI], levels_q[iQ])"""
    b = bits_per_axis(levels_i, levels_q)
    li, lq = np.asarray(levels_i, np.float32), np.asarray(levels_q, np.float32)
    p = np.arange(1 << (2 * b))
    return np.stack([li[p >> b], lq[p & ((1 << b) - 1)]], axis=1)


def energy(levels_i, levels_q):
    return ms.energy(materialise(levels_i, levels_q))


def noise_var(k, n_tx, levels_i, levels_q, ebn0_db):
    m = 2 * bits_per_axis(levels_i, levels_q)
    return energy(levels_i, levels_q) / (2.0 * (k / n_tx) * float(m) * 10.0 ** (ebn0_db / 10.0))


def _masks(b):
    lab = np.arange(1 << b)
    return [((lab >> (b - 1 - j)) & 1).astype(bool) for j in range(b)]


def axis_mins(levels, y):
    """y [...] float32, one coordinate -> (m0, m1) [..., b] float32 each: the smallest e_l per bit value"""
    lev = np.asarray(levels, np.float32)
    b = lev.shape[0].bit_length() - 1
    y = np.asarray(y, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = y[..., None] - lev
        e = dx * dx
        assert e.dtype == np.float32
        m0, m1 = np.empty(y.shape + (b,), np.float32), np.empty(y.shape + (b,), np.float32)
        for j, one in enumerate(_masks(b)):
            m0[..., j], m1[..., j] = np.minimum.reduce(e[..., ~one], axis=-1), np.minimum.reduce(e[..., one], axis=-1)
    return m0, m1


def axis_llrs(levels, y, inv):
    m0, m1 = axis_mins(levels, y)
    with np.errstate(invalid="ignore", over="ignore"):
        out = (m0 - m1) * np.float32(inv)
    assert out.dtype == np.float32
    return out


def symbol_llrs(levels_i, levels_q, sym, nv):
    """sym [..., 2] float32 -> LLRs [..., 2 b] float32: the I bits, then the Q bits"""
    bits_per_axis(levels_i, levels_q)
    sym = np.asarray(sym, np.float32)
    inv = np.float32(1.0 / (2.0 * float(nv)))
    return np.concatenate([axis_llrs(levels_i, sym[..., 0], inv), axis_llrs(levels_q, sym[..., 1], inv)], axis=-1)


def two_d_from_axes(levels_i, levels_q, sym, nv):
    """what modulation_spec.symbol_llrs gives on the materialised table, from the per-axis mins: fl(fl(fl(m0 + E) - fl(m1 + E)) inv),
    E = the smallest e of the other axis"""
    sym = np.asarray(sym, np.float32)
    inv = np.float32(1.0 / (2.0 * float(nv)))
    (i0, i1), (q0, q1) = axis_mins(levels_i, sym[..., 0]), axis_mins(levels_q, sym[..., 1])
    with np.errstate(invalid="ignore", over="ignore"):
        eI, eQ = np.minimum(i0[..., :1], i1[..., :1]), np.minimum(q0[..., :1], q1[..., :1])
        out = np.concatenate([((i0 + eQ) - (i1 + eQ)) * inv, ((q0 + eI) - (q1 + eI)) * inv], axis=-1)
    assert out.dtype == np.float32
    return out


def symbol_llrs_f64(levels_i, levels_q, sym, nv):
    """the per-axis formula in float64 on the same float32 inputs -> (LLRs [..., 2 b], m0 + m1 [..., 2 b])"""
    sym = np.asarray(sym, np.float32).astype(np.float64)
    inv = 1.0 / (2.0 * float(nv))
    outs, mags = [], []
    for lev, y in ((levels_i, sym[..., 0]), (levels_q, sym[..., 1])):
        lev = np.asarray(lev, np.float32).astype(np.float64)
        b = lev.shape[0].bit_length() - 1
        e = (y[..., None] - lev) ** 2
        for one in _masks(b):
            m0, m1 = e[..., ~one].min(axis=-1), e[..., one].min(axis=-1)
            outs.append((m0 - m1) * inv)
            mags.append(m0 + m1)
    return np.stack(outs, axis=-1), np.stack(mags, axis=-1)


def demap(levels_i, levels_q, sym, n_tx, N, nv, fmt=LLR_F32, qscale=4.0):
    """sym [B][n_sym][2] float32 -> [B][N] float32 / float16 / int8"""
    m = 2 * bits_per_axis(levels_i, levels_q)
    sym = np.asarray(sym, np.float32)
    B, ns = sym.shape[:2]
    assert ns == ms.symbols_per_frame(n_tx, m) and n_tx <= N
    llr = np.zeros((B, N), np.float32)
    llr[:, :n_tx] = symbol_llrs(levels_i, levels_q, sym, nv).reshape(B, ns * m)[:, :n_tx]
    if fmt == LLR_F32:
        return llr
    if fmt == LLR_F16:
        return ms.round_f16(llr)
    return layered_i8_spec.quantize(llr, qscale).astype(np.int8)


def transmit(levels_i, levels_q, seed, frame_ids, codewords, k, ebn0_db):
    """modulation_spec.transmit on the materialised points, for any m = 2 b:
    codewords [F][n_tx] -> (y [F][n_sym][2] float64 = c + sg z, bound unit [F][n_sym][2] = |c| + sg radius per coordinate, sg, sigma^2)"""
    m = 2 * bits_per_axis(levels_i, levels_q)
    pts = materialise(levels_i, levels_q).astype(np.float64)
    n_tx = np.asarray(codewords).shape[1]
    nv = noise_var(k, n_tx, levels_i, levels_q, ebn0_db)
    sg = float(np.float32(np.sqrt(nv)))
    lab = ms.labels(codewords, m)
    z, rad = ms.normals(seed, frame_ids, lab.shape[1])
    c = pts[lab]
    return c + sg * z, np.abs(c) + sg * rad[..., None], sg, nv
