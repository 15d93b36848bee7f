"""Specification of the fading channel and of the demapper with per-symbol channel state (include/ldpc_hip.h ldpc_fading,
ldpc_demap_dev_il_csi, ldpc_sim_transmit_il_fading, ldpc_sim_generate_mod_il_fading; csrc/fading.h): numpy, float32 operation by
operation.  What it shares with the AWGN path -- the labelling, the output formats, the stream-2 normals, the table -- comes from
tests/modulation_spec.py, tests/product_modulation_spec.py and tests/interleaver_spec.py.

Model          a coherent receiver with perfect channel knowledge: the phase is taken out and the samples are delivered equalised, so
               only the POWER gain a of a symbol appears.  The noise variance per real dimension of its sample is sigma^2 / a.
Blocks         symbol s of a frame lies in block q = s / block (block >= 1 symbols); all symbols of a block share one gain.
Draw           block pair Q = blocks 2Q and 2Q + 1: one Philox4x32-10 call, counter (frame lo, frame hi, Q, stream 3), key = seed; the
               uniforms and Box-Muller of the noise rule (modulation_spec.normals): (z0, z1) -> block 2Q, (z2, z3) -> block 2Q + 1.
Gain           mu = float32(sqrt(K / (K + 1))), sd = float32(sqrt(1 / (2 (K + 1)))), each computed in double and rounded once
               (K = the Rician factor, linear; 0 = Rayleigh);
                 hI = fl(mu + fl(sd z0)),  hQ = fl(sd z1),  a = max(fl(fl(hI hI) + fl(hQ hQ)), 2^-20)
               E[a] = 1 (before the floor) and Var[a] = (2K + 1) / (K + 1)^2.
Sample         sg_s = fl(sg / fl(sqrt a)),  y = fl(c + fl(sg_s z)) per coordinate, z the stream-2 normal of the AWGN rule; a = 1 gives
               sg_s = sg, the AWGN rule.
Demapper       inv = float32(1 / (2 sigma^2)),  inv_s = fl(inv a);  the LLRs of symbol s are the AWGN rule's with inv_s for inv:
               a table: fl(fl(m0_j - m1_j) inv_s); a product object: the per-axis form.  a = 0: zeros (an erasure); a NaN gain: NaN
               (int8: 0); a negative gain is the caller's error.
Outputs        demap_il_csi = deinterleave(the LLRs in transmitted order, in the output format), as interleaver_spec.demap_il.
As in modulation_spec the normals are float64 here: gains() and transmit() restate the device's float32 draw in float64 and carry
the unit of the GPU test's tolerance; gain_rule() and the demappers are the float32 rule itself."""
import numpy as np

from oracle import frame_source
from tests import interleaver_spec as ils
from tests import layered_i8_spec
from tests import modulation_spec as ms
from tests import product_modulation_spec as ps

FADING_STREAM = 3
FLOOR = 2.0 ** -20


def ricean(K):
    """-> (mu, sd) float32"""
    K = float(K)
    assert np.isfinite(K) and K >= 0.0
    return np.float32(np.sqrt(K / (K + 1.0))), np.float32(np.sqrt(1.0 / (2.0 * (K + 1.0))))


def block_normals(seed, frame_ids, n_blocks):
    """-> (z [F][n_blocks][2] float64: the two normals of every block, radius [F][n_blocks]: the Box-Muller radius of its pair half);
    the uniform rule of modulation_spec.normals on stream 3, one call per block pair"""
    flo, fhi, klo, khi = frame_source._split(seed, frame_ids)
    pairs = (n_blocks + 1) // 2
    Q = np.arange(pairs, dtype=np.uint64)
    r = frame_source.philox4x32_10((flo[:, None], fhi[:, None], Q[None, :], FADING_STREAM), (klo, khi))
    rf = r.astype(np.float32)
    one, s = np.float32(1.0), np.float32(2.0 ** -32)
    ua, ub = ((rf[0] + one) * s).astype(np.float64), (rf[1] * s).astype(np.float64)
    uc, ud = ((rf[2] + one) * s).astype(np.float64), (rf[3] * s).astype(np.float64)
    ra, rc = np.sqrt(-2.0 * np.log(ua)), np.sqrt(-2.0 * np.log(uc))
    ta, tc = 2.0 * np.pi * ub, 2.0 * np.pi * ud
    z = np.stack([ra * np.cos(ta), ra * np.sin(ta), rc * np.cos(tc), rc * np.sin(tc)], axis=-1)    # [F][pairs][4]
    rad = np.stack([ra, rc], axis=-1)
    F = flo.shape[0]
    return z.reshape(F, 2 * pairs, 2)[:, :n_blocks], rad.reshape(F, 2 * pairs)[:, :n_blocks]


def gain_rule(z0, z1, K):
    """the gain of a block from its two normals, one operation at a time in the dtype of z (float32: the device's rule)"""
    z0, z1 = np.asarray(z0), np.asarray(z1)
    t = z0.dtype.type
    assert z0.dtype == z1.dtype and t in (np.float32, np.float64)
    mu, sd = (t(v) for v in ricean(K))
    hI = mu + sd * z0
    hQ = sd * z1
    a = hI * hI + hQ * hQ
    assert a.dtype == z0.dtype
    return np.maximum(a, t(FLOOR))


def blocks_per_frame(n_sym, block):
    assert block >= 1
    return (n_sym + block - 1) // block


def gains(seed, frame_ids, n_sym, block, K):
    """-> (a [F][n_sym] float64, bound unit [F][n_sym]).  The unit: the device's hI and hQ are sums c + s z like a sample's coordinate,
    with the error unit |c| + s radius of modulation_spec.transmit, i.e. mu + sd radius and sd radius; through a = hI^2 + hQ^2 that is
    2 (|hI| (mu + sd radius) + |hQ| sd radius) to first order, plus a itself for the roundings of the two squares and the sum"""
    nb = blocks_per_frame(n_sym, block)
    z, rad = block_normals(seed, frame_ids, nb)
    mu, sd = (float(v) for v in ricean(K))
    hI, hQ = mu + sd * z[..., 0], sd * z[..., 1]
    a = gain_rule(z[..., 0], z[..., 1], K)
    unit = 2.0 * (np.abs(hI) * (mu + sd * rad) + np.abs(hQ) * sd * rad) + a
    q = np.arange(n_sym) // block
    return a[:, q], unit[:, q]


def sigma_rule(sg, a):
    """sg_s = fl(sg / fl(sqrt a)), float32"""
    a = np.asarray(a, np.float32)
    out = np.float32(sg) / np.sqrt(a)
    assert out.dtype == np.float32
    return out


def transmit(points, m, seed, frame_ids, tx_bits, nv, a, a_unit=None):
    """tx_bits [F][n_tx] in transmitted order, points [2^m][2] (materialised for a product object), a [F][n_sym] the gains ->
    (y [F][n_sym][2] float64 = c + sg_s z, bound unit [F][n_sym][2], sg).  The unit is modulation_spec.transmit's with sg_s for sg, plus
    the gain's: d sg_s = sg_s da / (2 a), so sg_s |z| a_unit / (2 a).  With a = 1 and no a_unit these are modulation_spec.transmit's
    values exactly"""
    pts = np.asarray(points, np.float32).astype(np.float64)
    assert pts.shape == (1 << m, 2)
    sg = np.float32(np.sqrt(nv))
    lab = ms.labels(tx_bits, m)
    z, rad = ms.normals(seed, frame_ids, lab.shape[1])
    sgs = sigma_rule(sg, a).astype(np.float64)[..., None]
    c = pts[lab]
    unit = np.abs(c) + sgs * rad[..., None]
    if a_unit is not None:
        unit = unit + sgs * np.abs(z) * (np.asarray(a_unit) / (2.0 * np.asarray(a, np.float64)))[..., None]
    return c + sgs * z, unit, float(sg)


def inv_rule(nv, a):
    """inv_s = fl(float32(1 / (2 sigma^2)) a), float32"""
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.float32(1.0 / (2.0 * float(nv))) * np.asarray(a, np.float32)
    assert out.dtype == np.float32
    return out


def symbol_llrs(points, sym, a, nv):
    """a table object: sym [..., 2] float32, a [...] float32 -> LLRs [..., m] float32, one float32 operation at a time"""
    pts = np.asarray(points, np.float32)
    m = ms.bits_per_symbol(pts)
    sym = np.asarray(sym, np.float32)
    inv_s = inv_rule(nv, a)
    assert inv_s.shape == sym.shape[:-1]
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
            out[..., j] = (m0 - m1) * inv_s
    return out


def symbol_llrs_product(levels_i, levels_q, sym, a, nv):
    """a product object: -> LLRs [..., 2 b] float32, the I bits, then the Q bits: fl(fl(m0_j - m1_j) inv_s) per axis"""
    ps.bits_per_axis(levels_i, levels_q)
    sym = np.asarray(sym, np.float32)
    inv_s = inv_rule(nv, a)
    assert inv_s.shape == sym.shape[:-1]
    outs = []
    with np.errstate(invalid="ignore", over="ignore"):
        for lev, y in ((levels_i, sym[..., 0]), (levels_q, sym[..., 1])):
            m0, m1 = ps.axis_mins(lev, y)
            o = (m0 - m1) * inv_s[..., None]
            assert o.dtype == np.float32
            outs.append(o)
    return np.concatenate(outs, axis=-1)


def _format(llr, fmt, qscale):
    if fmt == ms.LLR_F32:
        return llr
    if fmt == ms.LLR_F16:
        return ms.round_f16(llr)
    return layered_i8_spec.quantize(llr, qscale).astype(np.int8)


def demap_il_csi(points, sym, a, pos, N, nv, fmt=ms.LLR_F32, qscale=4.0):
    """a table object: sym [B][ceil(n_tx / m)][2] float32, a [B][ceil(n_tx / m)] float32 -> [B][N] float32 / float16 / int8"""
    n_tx = len(pos)
    B = np.asarray(sym).shape[0]
    tx = symbol_llrs(points, sym, a, nv).reshape(B, -1)[:, :n_tx]
    return ils.deinterleave(_format(np.ascontiguousarray(tx), fmt, qscale), pos, N)


def demap_il_csi_product(levels_i, levels_q, sym, a, pos, N, nv, fmt=ms.LLR_F32, qscale=4.0):
    """a product object"""
    n_tx = len(pos)
    B = np.asarray(sym).shape[0]
    tx = symbol_llrs_product(levels_i, levels_q, sym, a, nv).reshape(B, -1)[:, :n_tx]
    return ils.deinterleave(_format(np.ascontiguousarray(tx), fmt, qscale), pos, N)
