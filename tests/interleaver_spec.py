"""Specification of the bit interleaver (include/ldpc_hip.h ldpc_interleaver_*, ldpc_demap_dev_il, ldpc_sim_transmit_il,
ldpc_sim_generate_mod_il, ldpc_interleave_bits_dev, ldpc_deinterleave_llr_dev; csrc/interleaver.h): numpy.  The interleaver moves values
and computes none: every expected LLR is a value of tests/modulation_spec.py or tests/product_modulation_spec.py at another place.

Table          pos [n_tx], injective into 0 .. N - 1, 1 <= n_tx <= N.  Transmitted bit t is codeword bit pos[t]; symbol s carries
               transmitted bits m s .. m s + m - 1, the first one the MSB of its label (the labelling rule of modulation_spec; bits
               t >= n_tx of the last symbol pad as 0).  The identity table is the behaviour without an interleaver.
Holes          the codeword positions no pos[t] names, ascending: punctured, LLR 0.
Block rule     codeword bit i = c rows + u is written into column c of a rows x cols matrix at row (u + twist[c]) mod rows; the matrix is
               read row by row, the columns in the order order[0 .. cols - 1]:
                 pos[r cols + j] = c rows + ((r - twist[c]) mod rows),  c = order[j].
               By formula: no claim that it is any standard's table.
Interleave     tx[f][t] = codeword[f][pos[t]].
Deinterleave   out[f][pos[t]] = llr_tx[f][t]; out[f][h] = 0 for every hole h; the element type is kept.
Demapper       demap_il = deinterleave(demap of the same samples with N = n_tx), in the output format: the formats round element by
               element, so rounding and moving commute."""
import numpy as np

from tests import modulation_spec as ms
from tests import product_modulation_spec as ps


def block_positions(rows, cols, twist=None, order=None):
    """-> pos [rows * cols] int32"""
    rows, cols = int(rows), int(cols)
    assert rows >= 1 and cols >= 1
    tw = np.zeros(cols, np.int64) if twist is None else np.asarray(twist, np.int64)
    od = np.arange(cols, dtype=np.int64) if order is None else np.asarray(order, np.int64)
    assert tw.shape == (cols,) and ((0 <= tw) & (tw < rows)).all() and sorted(od.tolist()) == list(range(cols))
    pos = np.empty(rows * cols, np.int64)
    for r in range(rows):
        for j in range(cols):
            c = int(od[j])
            pos[r * cols + j] = c * rows + (r - int(tw[c])) % rows
    return pos.astype(np.int32)


def check(pos, N):
    pos = np.asarray(pos, np.int64)
    assert pos.ndim == 1 and 1 <= pos.shape[0] <= N and ((0 <= pos) & (pos < N)).all() and len(set(pos.tolist())) == pos.shape[0]
    return pos


def holes(pos, N):
    """-> the punctured positions, ascending, int32"""
    pos = check(pos, N)
    used = np.zeros(N, bool)
    used[pos] = True
    return np.flatnonzero(~used).astype(np.int32)


def interleave(codewords, pos):
    """codewords [F][N] -> transmitted bits [F][n_tx]"""
    cw = np.asarray(codewords)
    return cw[:, check(pos, cw.shape[1])]


def deinterleave(llr_tx, pos, N):
    """llr_tx [F][n_tx] -> [F][N] of the same dtype, 0 at the holes"""
    x = np.asarray(llr_tx)
    pos = check(pos, N)
    assert x.ndim == 2 and x.shape[1] == pos.shape[0]
    out = np.zeros((x.shape[0], N), x.dtype)
    out[:, pos] = x
    return out


def pack(bits):
    """[F][n] 0/1 -> [F][ceil(n / 8)] uint8, bit i in byte i / 8 at bit i % 8 (LDPC_BITS_PACKED), pad bits 0"""
    return np.packbits(np.asarray(bits, np.uint8), axis=1, bitorder="little")


def demap_il(points, sym, pos, N, nv, fmt=ms.LLR_F32, qscale=4.0):
    """a table object: sym [B][ceil(n_tx / m)][2] float32 -> [B][N] float32 / float16 / int8"""
    n_tx = len(pos)
    return deinterleave(ms.demap(points, sym, n_tx, n_tx, nv, fmt, qscale), pos, N)


def demap_il_product(levels_i, levels_q, sym, pos, N, nv, fmt=ps.LLR_F32, qscale=4.0):
    """a product object"""
    n_tx = len(pos)
    return deinterleave(ps.demap(levels_i, levels_q, sym, n_tx, n_tx, nv, fmt, qscale), pos, N)


def iq_alternating(pos, m):
    """the table of an I/Q-alternating labelling of a product constellation of m = 2 b bits: pos'[m s + 2 j] = pos[m s + j],
    pos'[m s + 2 j + 1] = pos[m s + b + j]; len(pos) must be a multiple of m"""
    pos = np.asarray(pos)
    b = m // 2
    assert m == 2 * b and pos.shape[0] % m == 0
    p = pos.reshape(-1, 2, b)                               # [s][axis][j]
    return np.ascontiguousarray(p.transpose(0, 2, 1)).reshape(-1).astype(np.int32)
