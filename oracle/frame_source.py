"""CPU restatement of the device frame source (TEST INFRASTRUCTURE; nothing under ecc_ldpc_amd/ imports it).

Restated from the header comment and the kernels of ecc_ldpc_amd/csrc/sim.hip (sim_msg_kernel, sim_frame_kernel) and the
host code of sim_generate, in plain numpy, vectorised over frames:

  randomness   Philox4x32-10 keyed by the 64-bit seed (key = (seed lo, seed hi)), counter = (frame lo, frame hi, index, stream);
               stream 0 = message words, stream 1 = noise;
  message      word w of frame f = output word 0 of counter (f lo, f hi, w, 0), the last word masked to k;
               bit i of word w = message bit 32 w + i;
  noise        one Philox call per group g of four positions 4g .. 4g+3, counter (f lo, f hi, g, 1); Box-Muller on
               (r0, r1) -> positions 4g (cos), 4g+1 (sin) and on (r2, r3) -> 4g+2 (cos), 4g+3 (sin); the uniforms are
               formed in float32 exactly as the kernel forms them, everything after that is float64 here (the kernel's
               logf / sqrtf / sincospif are what the GPU test's tolerance is about);
  channel      sigma^2 = 1/(2 (k/n_tx) 10^(dB/10)) in double; sg = float32(sqrt sigma^2), sc = float32(2/sigma^2) as the host
               rounds them; llr = sc ((2b-1) + sg z); positions n_tx .. N-1 are 0.
"""
from __future__ import annotations

import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)
_2M32 = np.float32(2.0 ** -32)


def philox4x32_10(counter, key):
    """counter: four 32-bit words, key: two (ints or arrays that broadcast together) -> the four output words [4][...] uint32.
    Each word lives in a uint64 lane so that the 32 x 32 -> 64 multiplies are exact."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in (*counter, *key)])
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK          # bumped after each round
    return np.stack([c0, c1, c2, c3]).astype(np.uint32)


def _split(seed, frame_ids):
    seed = int(seed)
    assert 0 <= seed < 2 ** 64
    f = np.asarray(frame_ids, dtype=np.uint64)
    return f & _MASK, f >> _S32, seed & 0xFFFFFFFF, seed >> 32


def message_words(seed, frame_ids, k):
    """-> [F][ceil(k/32)] uint32"""
    flo, fhi, klo, khi = _split(seed, frame_ids)
    kw = (k + 31) // 32
    w = np.arange(kw, dtype=np.uint64)
    out = philox4x32_10((flo[:, None], fhi[:, None], w[None, :], 0), (klo, khi))[0]
    if k % 32:
        out[:, -1] &= np.uint32((1 << (k % 32)) - 1)
    return out


def message_bits(seed, frame_ids, k):
    """-> [F][k] uint8"""
    words = message_words(seed, frame_ids, k)
    bits = (words[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(words.shape[0], -1)[:, :k].astype(np.uint8)


def normals(seed, frame_ids, n_tx):
    """-> (z [F][n_tx] float64, radius [F][n_tx] float64: the Box-Muller radius of the pair each sample belongs to)"""
    flo, fhi, klo, khi = _split(seed, frame_ids)
    groups = (n_tx + 3) // 4
    g = np.arange(groups, dtype=np.uint64)
    r = philox4x32_10((flo[:, None], fhi[:, None], g[None, :], 1), (klo, khi))
    rf = r.astype(np.float32)                                        # uint32 -> float32, round to nearest even
    one = np.float32(1.0)
    ua, ub = ((rf[0] + one) * _2M32).astype(np.float64), (rf[1] * _2M32).astype(np.float64)     # float32 products, then widened
    uc, ud = ((rf[2] + one) * _2M32).astype(np.float64), (rf[3] * _2M32).astype(np.float64)
    ra, rc = np.sqrt(-2.0 * np.log(ua)), np.sqrt(-2.0 * np.log(uc))
    ta, tc = 2.0 * np.pi * ub, 2.0 * np.pi * ud
    z = np.stack([ra * np.cos(ta), ra * np.sin(ta), rc * np.cos(tc), rc * np.sin(tc)], axis=-1)
    rad = np.stack([ra, ra, rc, rc], axis=-1)
    F = flo.shape[0]
    return z.reshape(F, 4 * groups)[:, :n_tx], rad.reshape(F, 4 * groups)[:, :n_tx]


def scales(k, n_tx, ebn0_db):
    """-> (sg, sc): sigma and 2/sigma^2 as the float32 values the host hands to the kernel, widened to float64"""
    s2 = 1.0 / (2.0 * (k / n_tx) * 10.0 ** (ebn0_db / 10.0))
    return float(np.float32(np.sqrt(s2))), float(np.float32(2.0 / s2))


def llrs(seed, frame_ids, codewords, k, n_tx, N, ebn0_db):
    """codewords [F][>= n_tx] 0/1 -> (llr [F][N] float64, radius [F][n_tx], sg, sc)"""
    z, rad = normals(seed, frame_ids, n_tx)
    sg, sc = scales(k, n_tx, ebn0_db)
    x = 2.0 * np.asarray(codewords)[:, :n_tx].astype(np.float64) - 1.0
    llr = np.zeros((z.shape[0], N), np.float64)
    llr[:, :n_tx] = sc * (x + sg * z)
    return llr, rad, sg, sc
