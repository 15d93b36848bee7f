"""(CPU) the int8 fixed-point layered min-sum specification, tests/layered_i8_spec.py: hand-worked rows, the quantiser's corner cases,
a pin against the Double oracle (oracle.decode_layered, min-sum, one row per layer), and the build's three int8 kernel instances
(csrc/layered_csr.hip layered_csr_kernel<DCLASS, int8_t>) in the code-object metadata: present, no scratch, no spilled VGPR."""
import os
import re

import numpy as np
import pytest

from ecc_ldpc_amd import build as B
from oracle import oracle
from tests import layered_i8_spec as spec
from tests.helpers import load


def _row(lam, msg=None):
    lam = np.asarray([lam], np.int32)
    msg = np.zeros_like(lam) if msg is None else np.asarray([msg], np.int32)
    nl, nm, odd, flip = spec.row_update(lam, msg)
    return nl[0].tolist(), nm[0].tolist(), bool(odd[0]), bool(flip[0])


def test_row_weight3_by_hand():
    # t = (5, -3, 1): signs (0, 1, 0), xor 1; weight odd -> message k negative iff 1 ^ 1 ^ s_k = s_k.  m1 = 1, m2 = 3: n1 = 5 >> 2 = 1,
    # n2 = 11 >> 2 = 2.  Edges 0 and 1 get magnitude n1 = 1, edge 2 (the minimum) gets n2 = 2.
    nl, nm, odd, flip = _row((5, -3, 1))
    assert nm == [1, -1, 2] and nl == [6, -4, 3]
    assert odd is False and flip is False             # hard = (1, 0, 1): even parity; no decision changed


def test_row_with_a_zero_difference():
    # a zero counts as non-negative and is the minimum: every other edge gets n(0) = (0 + 2) >> 2 = 0, the zero edge n(m2)
    nl, nm, odd, flip = _row((0, 7, -9, 4))           # weight 4 (even), signs (0, 0, 1, 0): xor 1 -> negative iff 1 ^ s_k
    assert nm == [-3, 0, 0, 0]                        # m2 = 4: (12 + 2) >> 2 = 3; the -0 of edges 1 and 3 is 0
    assert nl == [-3, 7, -9, 4] and odd is False and flip is False    # hard(0) = hard(-3) = 0
    # the difference lam - msg can be zero with lam != 0
    nl, nm, _, _ = _row((6, -8), (6, 2))              # t = (0, -10): even weight, xor 1 -> negative iff 1 ^ s_k
    assert nm == [-8, 0] and nl == [-8, -10]          # edge 0 (the minimum): n(10) = 32 >> 2 = 8; edge 1: n(0) = 0


def test_row_with_tied_minima():
    # |t| = (4, 4, 9): m1 = m2 = 4 with multiplicity, n1 = n2 = 14 >> 2 = 3; both tied edges are "the minimum" and get n2 = n1
    nl, nm, odd, flip = _row((4, -4, 9))
    assert nm == [3, -3, 3] and nl == [7, -7, 12]     # weight odd, xor 1: negative iff s_k
    assert odd is False and flip is False


def test_three_quarters_rounds_half_up():
    for m, n in ((0, 0), (1, 1), (2, 2), (3, 2), (4, 3), (5, 4), (6, 5), (127, 95), (222, 167)):
        assert (3 * m + 2) >> 2 == n
        nl, nm, _, _ = _row((m, 100))                 # weight 2, both positive: each edge gets +n(the other)
        assert nm == [(3 * 100 + 2) >> 2, n]


def test_sum_clips_at_127():
    nl, nm, odd, flip = _row((120, 100, -126))        # t as given; weight odd, xor 1: negative iff s_k
    assert nm == [75, 90, -75]                        # m1 = 100 -> 75, m2 = 120 -> 90
    assert nl == [127, 127, -127]                     # 195, 190, -201 clipped
    nl, nm, _, _ = _row((127, 127), (-100, -100))     # t = 227 is not clamped: n(227) = 170
    assert nm == [170, 170] and nl == [127, 127]
    # the flip is taken after the clip, from the stored cell: t + msg = -2 turns a 1 into a 0
    nl, nm, odd, flip = _row((1, -4))                 # even weight, xor 1: negative iff 1 ^ s_k -> (-, +); n(4) = 3, n(1) = 1
    assert nm == [-3, 1] and nl == [-2, -3] and odd is True and flip is True


def test_quantiser():
    q = spec.quantize
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, 127.5, -127.5, 0.49, 3.5], np.float32)
    assert q(x, 1.0).tolist() == [0, 2, 2, 0, -2, -2, 126, 127, -127, 0, 4]                  # ties go to even
    assert q(np.array([0.125, 0.375, 0.625, -0.375], np.float32), 4.0).tolist() == [0, 2, 2, -2]
    assert q(np.array([np.inf, -np.inf, np.nan, 1e30, -1e30], np.float32), 4.0).tolist() == [127, -127, 0, 127, -127]
    assert q(np.array([-128, -127, 127, 0, 5], np.int8)).tolist() == [-127, -127, 127, 0, 5]  # native int8: as it is, -128 as -127
    assert q(np.array([-128], np.int8), 3.3).tolist() == [-127]                               # (the scale plays no part)
    # a double is converted to float32 FIRST: 0.625 + 2^-30 is a tie once it is a float, not before
    d = np.array([0.625 + 2.0 ** -30], np.float64)
    assert q(d, 4.0).tolist() == [2] and int(np.rint(d[0] * 4.0)) == 3
    # ONE float32 multiply: 3.3f is not 3.3, and the product is rounded to float32 before rint
    v = np.float32(float.fromhex("0x1.f83e10p+0"))   # v * 3.3f = 6.5000000014 exactly, 6.5 (a tie -> 6) once rounded to float32
    assert float(v) * float(np.float32(3.3)) > 6.5 and np.float32(v * np.float32(3.3)) == 6.5
    assert q(np.array([v]), 3.3).tolist() == [6] and q(np.array([float(v)], np.float64), 3.3).tolist() == [6]
    assert q(np.array([1.0], np.float16), 3.3).tolist() == [3] and q(np.array([1.0], np.float16), 3.3).dtype == np.int32


def test_quantiser_on_non_finite_input_of_every_element_type():
    """include/ldpc_hip.h, non-finite channel LLRs, rule 1: +inf -> 127, -inf -> -127, NaN of either sign -> 0, whatever the buffer's type"""
    q = spec.quantize
    h = np.array([0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01], np.uint16).view(np.float16)       # +inf, -inf, NaN, -NaN, a signalling NaN
    assert np.isinf(h[:2]).all() and np.isnan(h[2:]).all() and np.signbit(h).tolist() == [False, True, False, True, False]
    for qs in (4.0, 3.3, 0.01):
        assert q(h, qs).tolist() == [127, -127, 0, 0, 0]
    f = np.array([0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000], np.uint32).view(np.float32)
    assert q(f, 4.0).tolist() == [0, 0, 127, -127]
    d = np.array([1e300, -1e300, np.nan, -np.nan, np.inf, 3e38], np.float64)                 # 1e300 is an infinity once it is a float
    assert q(d, 4.0).tolist() == [127, -127, 0, 0, 127, 127] and q(d, 1e-38).tolist() == [127, -127, 0, 0, 127, 3]
    # after the quantiser the frame is an ordinary frame: a decode with NaNs equals the decode with zeros in their place
    c = load("moon.7.13")
    _, llr = c.frames(4, 3.0, seed=9)
    p, z = llr.astype(np.float16), llr.astype(np.float16)
    p[0, 2], p[1, 4], p[2, :] = h[2], h[3], h[4]
    z[0, 2], z[1, 4], z[2, :] = 0, 0, 0
    a = spec.decode_minsum_i8_layered(c.graph, q(p, 4.0), 10)
    b = spec.decode_minsum_i8_layered(c.graph, q(z, 4.0), 10)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.isfinite(a[3]).all()


def test_decoder_stopping_rule_and_final_lam():
    c = load("moon.7.13")
    g = c.graph
    z = np.zeros((1, c.N), np.int32)                                    # all-zero LLRs: hard = 0, syndrome zero before sweep 1
    bits, its, conv, lam = spec.decode_minsum_i8_layered(g, z, 10)
    assert conv[0] and its[0] == 0 and not bits.any() and not lam.any()
    _, llr = c.frames(4, 0.0, seed=5)
    qv = spec.quantize(llr, 3.3)
    bits, its, conv, lam = spec.decode_minsum_i8_layered(g, qv, 0, qscale=3.3)   # no sweeps: the channel's decisions as stored
    syn0 = np.array([not oracle_syndrome_zero(g, qv[f] > 0) for f in range(4)])
    assert np.array_equal(conv, ~syn0) and (its == 0).all()
    assert np.array_equal(bits, (qv > 0).astype(np.uint8))
    assert np.array_equal(lam, qv.astype(np.float64) / np.float64(np.float32(3.3)))


def oracle_syndrome_zero(g, hard):
    rp, ci = np.asarray(g.row_ptr), np.asarray(g.col_idx)
    return all(not (np.count_nonzero(hard[ci[rp[m]:rp[m + 1]]]) & 1) for m in range(len(rp) - 1))


@pytest.mark.parametrize("name,db,F", [("1920.1280.3.303", 2.0, 64), ("1920.1280.3.303", 1.2, 96), ("jpl.1024.4.5", 3.0, 48)])
def test_pin_against_the_double_oracle(name, db, F):
    """int8 (qscale 4, 30 sweeps) next to the Double layered oracle, one row per layer, on the same frames: identical bits on every
    frame both report converged; the flags agree on at least 90 % of the frames."""
    c = load(name)
    _, llr = c.frames(F, db, seed=4242)
    lp = np.arange(c.M + 1)
    bits, its, conv, _ = spec.decode_minsum_i8_layered(c.graph, spec.quantize(llr, 4.0), 30, qscale=4.0)
    ref = [oracle.decode_layered(c.graph, lp, "min", 30, llr[f]) for f in range(F)]
    oconv = np.array([bool(r["converged"]) for r in ref])
    obits = np.stack([r["bits"] for r in ref])
    both = conv & oconv
    agree = int((conv == oconv).sum())
    print(f"{name} {db} dB: flags agree on {agree}/{F} frames, both converged {int(both.sum())}, "
          f"int8 converged {int(conv.sum())}, Double {int(oconv.sum())}")
    assert np.array_equal(bits[both], obits[both])
    assert agree >= 0.9 * F


def test_int8_instances_exist_and_use_no_scratch():
    path = os.path.join(os.path.dirname(B.__file__), "build", "layered_csr-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), f"no device assembly at {path}: build first (python ecc_ldpc_amd/build.py)"
    text = open(path).read()
    for dclass in (8, 20, 32):
        m = re.search(r"\.name:\s+_ZN4ldpc18layered_csr_kernelILi%dEaEE\S*\n((?:\s+\.[a-z_]+:.*\n)+)" % dclass, text)
        assert m, f"layered_csr_kernel<{dclass}, signed char>: no code-object metadata"
        f = {k: int(v) for k, v in re.findall(r"\.([a-z_]+):\s+(\d+)", m.group(1))}
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (dclass, f)
