"""Specification of rate matching and HARQ soft combining (include/ldpc_hip.h ldpc_ratematch_*, ldpc_demap_dev_rm,
ldpc_ratematch_llr_dev, ldpc_ratematch_bits_dev, ldpc_sim_transmit_rm; csrc/ratematch.h): numpy, float32 one operation at a time.  The
LLR of one transmitted bit is NOT restated here: it is modulation_spec.symbol_llrs / product_modulation_spec.symbol_llrs (no channel
state) or fading_spec.symbol_llrs / symbol_llrs_product (a power gain per symbol); this file states what happens to those values.

Table          pos [E], any map into 0 .. N - 1, E >= 1: entries may repeat and E may exceed N.  Transmitted bit t is codeword bit
               pos[t]; symbol s carries transmitted bits m s .. m s + m - 1 (the labelling rule of modulation_spec; bits t >= E of
               the last symbol pad as 0 and have no LLR).  Positions no entry names are not sent in this round.
Circular rule  pos[t] = buf[(start + t) mod n_buf], buf the buffer's positions in its order (None: 0 .. n_buf - 1), start the offset
               of the redundancy version.  By formula: no claim that it is any standard's table.
Inverse        CSR: inv_t[inv_ptr[c] .. inv_ptr[c + 1]) = the t with pos[t] = c, ASCENDING.  fanin[c] = inv_ptr[c + 1] - inv_ptr[c].
Sum            position c with t_1 < t_2 < .. < t_r:  v = fl(fl(fl(l_t1 + l_t2) + l_t3) + ..), float32, left to right; r = 1: v = l_t1.
accumulate 0   out = fmt(v), the output conversions of modulation_spec (float32; fp16 clamped to +-65504; int8
               clip(rint(v qscale)), NaN -> 0); 0 where r = 0.
accumulate 1   onto old, the buffer's value in the same format:  float32 fl(old + v);  fp16 round_f16(fl(f32(old) + v)), a NaN stays;
               int8 clip(rint(fl(f32(old) + fl(v qscale))), -127, 127), and old where v is NaN.  r = 0: old.
Transmit       tx[f][t] = codeword[f][pos[t]]; the channel is fading_spec.transmit on those bits (a = 1: AWGN) with sigma^2 from the rate
               of this transmission, R = k / E."""
import numpy as np

from tests import fading_spec as fs
from tests import layered_i8_spec
from tests import modulation_spec as ms
from tests import product_modulation_spec as ps


def circular_positions(n_buf, start, E, buf=None):
    """-> pos [E] int32"""
    n_buf, start, E = int(n_buf), int(start), int(E)
    assert n_buf >= 1 and E >= 1 and 0 <= start < n_buf
    b = np.arange(n_buf, dtype=np.int64) if buf is None else np.asarray(buf, np.int64)
    assert b.shape == (n_buf,)
    return b[(start + np.arange(E, dtype=np.int64)) % n_buf].astype(np.int32)


def check(pos, N):
    pos = np.asarray(pos, np.int64)
    assert pos.ndim == 1 and pos.shape[0] >= 1 and N >= 1 and ((0 <= pos) & (pos < N)).all()
    return pos


def invert(pos, N):
    """-> (inv_ptr [N + 1], inv_t [E]) int32; a stable sort by position keeps every list ascending"""
    pos = check(pos, N)
    inv_t = np.argsort(pos, kind="stable").astype(np.int32)
    inv_ptr = np.concatenate([[0], np.cumsum(np.bincount(pos, minlength=N))]).astype(np.int32)
    return inv_ptr, inv_t


def fanin(pos, N):
    return np.bincount(check(pos, N), minlength=N).astype(np.int32)


def ratematch_bits(codewords, pos):
    """codewords [F][N] -> transmitted bits [F][E]"""
    cw = np.asarray(codewords)
    return cw[:, check(pos, cw.shape[1])]


def position_sums(llr_tx, pos, N):
    """llr_tx [F][E] float32 -> (v [F][N] float32, sent [N] bool): the left-to-right float32 sum per position, one addition at a time;
    v is 0 where nothing was sent"""
    x = np.asarray(llr_tx)
    assert x.dtype == np.float32 and x.ndim == 2 and x.shape[1] == len(pos)
    inv_ptr, inv_t = invert(pos, N)
    v = np.zeros((x.shape[0], N), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(N):
            ts = inv_t[inv_ptr[c]:inv_ptr[c + 1]]
            if len(ts):
                acc = x[:, ts[0]].copy()
                for t in ts[1:]:
                    acc = acc + x[:, t]
                    assert acc.dtype == np.float32
                v[:, c] = acc
    return v, np.diff(inv_ptr) > 0


def combine(v, sent, fmt=ms.LLR_F32, qscale=4.0, old=None):
    """the sums into the output format: old None = accumulate 0, else old [F][N] in the output dtype = accumulate 1"""
    v = np.asarray(v, np.float32)
    qs = np.float32(qscale)
    with np.errstate(invalid="ignore", over="ignore"):
        if old is None:
            if fmt == ms.LLR_F32:
                return v.copy()
            if fmt == ms.LLR_F16:
                return ms.round_f16(v)
            return layered_i8_spec.quantize(v, qscale).astype(np.int8)
        old = np.asarray(old)
        assert old.shape == v.shape
        if fmt == ms.LLR_F32:
            assert old.dtype == np.float32
            new = old + v
        elif fmt == ms.LLR_F16:
            assert old.dtype == np.float16
            new = ms.round_f16(old.astype(np.float32) + v)
        else:
            assert old.dtype == np.int8
            s = np.rint(old.astype(np.float32) + v * qs)
            assert s.dtype == np.float32
            new = np.where(np.isnan(v), old, np.clip(np.where(np.isnan(s), 0, s), -127, 127).astype(np.int8)).astype(np.int8)
        return np.where(sent[None, :], new, old).astype(old.dtype)


def ratematch_llr(llr_tx, pos, N, fmt=ms.LLR_F32, qscale=4.0, old=None):
    """the table alone: llr_tx [F][E] float32 -> [F][N]"""
    v, sent = position_sums(np.asarray(llr_tx, np.float32), pos, N)
    return combine(v, sent, fmt, qscale, old)


def bit_llrs(points, sym, E, nv, a=None):
    """a table object: sym [F][ceil(E / m)][2] float32, a [F][n_sym] float32 or None -> the LLRs of the E transmitted bits [F][E]"""
    sym = np.asarray(sym, np.float32)
    per = ms.symbol_llrs(points, sym, nv) if a is None else fs.symbol_llrs(points, sym, a, nv)
    assert sym.shape[1] == ms.symbols_per_frame(E, per.shape[-1])
    return np.ascontiguousarray(per.reshape(sym.shape[0], -1)[:, :E])


def bit_llrs_product(levels_i, levels_q, sym, E, nv, a=None):
    """a product object"""
    sym = np.asarray(sym, np.float32)
    per = ps.symbol_llrs(levels_i, levels_q, sym, nv) if a is None else fs.symbol_llrs_product(levels_i, levels_q, sym, a, nv)
    assert sym.shape[1] == ms.symbols_per_frame(E, per.shape[-1])
    return np.ascontiguousarray(per.reshape(sym.shape[0], -1)[:, :E])


def demap_rm(points, sym, pos, N, nv, fmt=ms.LLR_F32, qscale=4.0, a=None, old=None):
    """a table object: -> [F][N] float32 / float16 / int8"""
    return ratematch_llr(bit_llrs(points, sym, len(pos), nv, a), pos, N, fmt, qscale, old)


def demap_rm_product(levels_i, levels_q, sym, pos, N, nv, fmt=ms.LLR_F32, qscale=4.0, a=None, old=None):
    """a product object"""
    return ratematch_llr(bit_llrs_product(levels_i, levels_q, sym, len(pos), nv, a), pos, N, fmt, qscale, old)


def noise_var(k, E, points, ebn0_db):
    """sigma^2 per real dimension at the rate of one transmission, R = k / E: modulation_spec.noise_var's formula with E for n_tx;
    points [2^m][2], materialised for a product object (m up to 12)"""
    m = len(points).bit_length() - 1
    assert len(points) == 1 << m
    return ms.energy(points) / (2.0 * (k / E) * float(m) * 10.0 ** (ebn0_db / 10.0))
