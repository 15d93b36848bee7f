"""(CPU) tests/layered_rule_spec.py, the specification of the per-context check-node rule (cn_scale, cn_offset) of the on-chip layered
min-sum kernel for any H: at (3/4, 0) it is the three shipped specifications bit for bit (those are pinned to the Double oracle, so this
pins the new module); the integer transform against exact arithmetic; the cap of 511 never binds at the default; the f32 instance is
homogeneous under powers of two; a non-default rule changes results; and the build's nine rule instances use no scratch."""
import os
import re

import numpy as np
import pytest

from ecc_ldpc_amd import build as B
from oracle import emulate_f16 as em
from tests import layered_f32_spec as f32spec
from tests import layered_i8_spec as i8spec
from tests import layered_rule_spec as spec
from tests.helpers import load

# the cases of tests/test_layered_i8_spec.py test_pin_against_the_double_oracle (qscale 4, 30 sweeps, seed 4242)
I8_CASES = [("1920.1280.3.303", 2.0, 64), ("1920.1280.3.303", 1.2, 96), ("jpl.1024.4.5", 3.0, 48)]
# the cases of tests/test_layered_f32_emulation.py: the two codes pinned to the Double oracle (16 frames, 25 sweeps) and the
# 1920.1280.A frames that leave the float range (f32: the veto; fp16: lam saturates)
FLOAT_CASES = [(name, dbs, "oracle") for name, dbs in f32spec.ORACLE_CASES] + [("1920.1280.A", (2.0, 3.0), "exact")]


def _i8_frames(name, db, F):
    c = load(name)
    _, llr = c.frames(F, db, seed=4242)
    return c.graph, i8spec.quantize(llr, 4.0)


def _float_frames(name, dbs, kind):
    G = f32spec._named(name)
    return G, (f32spec.oracle_inputs(G, dbs) if kind == "oracle" else f32spec.exact_inputs(G, dbs))


def _equal(got, ref):
    return all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got[:4], ref[:4]))


# ---- 1. the default is the shipped specifications
@pytest.mark.parametrize("name,db,F", I8_CASES)
def test_default_is_the_int8_specification(name, db, F):
    g, q = _i8_frames(name, db, F)
    ref = i8spec.decode_minsum_i8_layered(g, q, 30, qscale=4.0)
    assert spec.int_params(0.75, 0.0, 4.0) == (12, 0)
    assert _equal(spec.decode_i8(g, q, 30, 4.0, 0.75, 0.0), ref)
    assert ref[2].any() and (ref[1] > 1).any()


@pytest.mark.parametrize("name,dbs,kind", FLOAT_CASES)
def test_default_is_the_f32_specification(monkeypatch, name, dbs, kind):
    G, llr = _float_frames(name, dbs, kind)
    bits, its, conv, lam, vetoed = f32spec.emulate(monkeypatch, G, llr, 25)
    assert _equal(spec.decode_float(G, llr, 25, 0.75, 0.0, "f32"), (bits, its, conv, lam))
    assert vetoed.any() == (kind == "exact")


@pytest.mark.parametrize("name,dbs,kind", FLOAT_CASES[:2])     # (the emulation has no CPU test of its own: the two codes pinned to the oracle)
def test_default_is_the_fp16_specification(name, dbs, kind):
    G, llr = _float_frames(name, dbs, kind)
    ref = em.decode_minsum_f16_layered(f32spec._emu_graph(G), llr, 25)
    assert _equal(spec.decode_float(G, llr, 25, 0.75, 0.0, "f16"), ref)


# ---- 2. the integer transform against exact arithmetic
def test_integer_transform_is_exact():
    m = np.arange(1024)
    for a in range(1, 17):
        for b in range(0, 33):
            exact = [min(max((2 * a * int(x) + 16) // 32 - b, 0), 511) for x in m]      # floor(a m / 16 + 1/2) - b, clipped
            assert spec.int_rule(m, a, b).tolist() == exact, (a, b)
    assert np.array_equal(spec.int_rule(m[:511], 12, 0), (3 * m[:511] + 2) >> 2)        # the default is the shipped 3/4 (|t| <= 510 there)
    # the integers of a context: ties to even, alpha clipped into 1..16 sixteenths, beta in steps of 1 / qscale
    assert spec.int_params(0.875, 0.0) == (14, 0) and spec.int_params(0.8125, 0.25) == (13, 1) and spec.int_params(1.0, 0.5) == (16, 2)
    assert spec.int_params(0.78125, 0.625) == (12, 2) and spec.int_params(0.84375, 0.375) == (14, 2)     # 12.5 -> 12, 13.5 -> 14; 2.5 -> 2, 1.5 -> 2
    assert spec.int_params(0.04, 0.0)[0] == 1 and spec.int_params(1.0, 0.5, 3.3)[1] == 2


# ---- 3. the cap never binds at the default
@pytest.mark.parametrize("name,db,F", I8_CASES)
def test_cap_never_binds_at_the_default(name, db, F):
    g, q = _i8_frames(name, db, F)
    peak = [None]
    spec.decode_i8(g, q, 30, 4.0, 0.75, 0.0, peak=peak)
    assert 0 < peak[0] < 384, peak                                     # the induction's bound is 383
    assert int(spec.int_rule(510, 12, 0)) == 383 and int(spec.int_rule(638, 16, 0)) == 511 and int(spec.int_rule(511, 16, 0)) == 511


# ---- 4. power-of-two homogeneity of the f32 instance
@pytest.mark.parametrize("alpha,beta", [(0.8125, 0.25)])
def test_f32_instance_is_homogeneous_under_powers_of_two(alpha, beta):
    """LLRs and beta times 2^3 and 2^-3: every product, difference and compare scales exactly (largest |LLR| here about 30, far from
    overflow and from the subnormals), so bits, sweeps and flags are identical and final_lam is scaled exactly -- beta enters where
    the magnitudes are made and nowhere else"""
    G, llr = _float_frames("1920.1280.3.303", (1.5, 2.5), "oracle")
    ref = spec.decode_float(G, llr, 25, alpha, beta, "f32")
    assert ref[2].any() and (ref[1] > 1).any() and np.isfinite(ref[3]).all()
    for s in (np.float32(8.0), np.float32(0.125)):
        got = spec.decode_float(G, llr * s, 25, alpha, float(np.float32(beta) * s), "f32")
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
        assert np.array_equal(got[3], ref[3] * s)
    off = spec.decode_float(G, llr * np.float32(8.0), 25, alpha, beta, "f32")         # beta NOT scaled: another decoder
    assert not np.array_equal(off[1], ref[1]) or not np.array_equal(off[3], ref[3] * np.float32(8.0))


# ---- 5. the rule bites
@pytest.mark.parametrize("cell", ["f16", "f32", "i8"])
def test_rule_bites(cell):
    G, llr = _float_frames("1920.1280.3.303", (1.5, 2.5), "oracle")
    base = spec.decode(cell, G, llr, 25)
    for alpha, beta in ((1.0, 0.5), (0.875, 0.0)):
        got = spec.decode(cell, G, llr, 25, alpha, beta)
        assert not np.array_equal(got[1], base[1]) or not np.array_equal(got[3], base[3]), (cell, alpha, beta)


def test_scale_one_is_the_plain_minimum():
    l = np.array([[5.5, -3.25, 1.5, -7.0]], np.float32)                # msg = 0, so t = l; even weight, signs (0, 1, 0, 1): xor 0
    for store in (em.r16, spec.f32_cast):
        nw, nm, odd, flip = spec.row_update_float(l, np.zeros_like(l), 1.0, 0.0, store)
        assert np.abs(nm[0]).tolist() == [1.5, 1.5, 3.25, 1.5]         # each edge: the smallest |t| of the OTHER edges
        assert (nm[0] < 0).tolist() == [False, True, False, True]      # even weight, even number of negatives: the sign of t_k
        assert nw[0].tolist() == [7.0, -4.75, 4.75, -8.5]
    nl, nm, odd, flip = spec.row_update_i8(np.array([[22, -13, 6, -28]]), np.zeros((1, 4), np.int32), 16, 0)
    assert nm[0].tolist() == [6, -6, 13, -6] and nl[0].tolist() == [28, -19, 19, -34]
    # and the offset is taken from that minimum, never below zero
    nl, nm, _, _ = spec.row_update_i8(np.array([[22, -13, 1, -28]]), np.zeros((1, 4), np.int32), 16, 2)
    assert nm[0].tolist() == [0, 0, 11, 0]
    _, nm, _, _ = spec.row_update_float(l, np.zeros_like(l), 1.0, 2.0, spec.f32_cast)
    assert np.abs(nm[0]).tolist() == [0.0, 0.0, 1.25, 0.0]
    # a NaN stays a NaN, an infinity an infinity (what the f32 instance's veto has to go on seeing)
    assert np.isnan(spec.float_rule(np.float32(np.nan), 1.0, 0.5)) and np.isposinf(spec.float_rule(np.float32(np.inf), 0.875, 0.5))
    assert spec.float_rule(np.float32(0.25), 1.0, 0.5) == 0 and not np.signbit(spec.float_rule(np.float32(0.25), 1.0, 0.5))


@pytest.mark.parametrize("cell", ["f16", "f32", "i8"])
def test_a_row_without_edges_changes_nothing(cell):
    """rows of weight 0 (even parity, no message, no lam write) are skipped: the same arrays with them and without"""
    G, llr = _float_frames("moon.7.13", (1.0, 3.0), "oracle")
    rp = np.asarray(G.rp).tolist()
    M = len(rp) - 1
    for at in (M, M // 2, 0):                                       # a last, a middle and a first row
        rp.insert(at, rp[at])
    H = f32spec.Graph(rp, G.ci, G.N)
    assert H.M == M + 3 and (np.diff(H.rp) == 0).sum() == 3 and np.diff(H.rp)[[0, -1]].tolist() == [0, 0]
    for alpha, beta in ((0.75, 0.0), (1.0, 0.5)):
        ref = spec.decode(cell, G, llr, 25, alpha, beta)
        assert ref[2].any() and (ref[1] > 1).any()
        assert _equal(spec.decode(cell, H, llr, 25, alpha, beta), ref)


# ---- 6. the build's rule instances
def test_rule_instances_exist_and_use_no_scratch():
    path = os.path.join(os.path.dirname(B.__file__), "build", "layered_csr-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(path):
        pytest.skip(f"no device assembly at {path}: build first (python ecc_ldpc_amd/build.py)")
    text = open(path).read()
    for cell in ("DF16_", "f", "a"):
        for dclass in (8, 20, 32):
            m = re.search(r"\.max_flat_workgroup_size:\s+(\d+)\n\s+\.name:\s+_ZN4ldpc18layered_csr_kernelILi%dENS_5RuledI%sEEEE\S*\n((?:\s+\.[a-z_]+:.*\n)+)" % (dclass, cell), text)
            assert m, f"layered_csr_kernel<{dclass}, Ruled<{cell}>>: no code-object metadata"
            f = {k: int(v) for k, v in re.findall(r"\.([a-z_]+):\s+(\d+)", m.group(2))}
            assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (dclass, cell, f)
            assert int(m.group(1)) == (512 if dclass == 32 else 1024), (dclass, cell, m.group(1))     # the heavy-row instances stay at 512 threads


# ---- 7. what the library decides before it needs a device
def test_out_of_range_rules_and_misplaced_name_suffixes_are_refused_without_a_gpu():
    import ecc_ldpc_amd as E
    from tests.helpers import CODES
    code = load("moon.7.13").hip_code(E)
    nan, inf = float("nan"), float("inf")
    for cell, kw in (("f16", dict(cn_scale=nan)), ("f16", dict(cn_scale=inf)), ("f16", dict(cn_scale=1.25)), ("f16", dict(cn_scale=-0.5)),
                     ("f32", dict(cn_offset=nan)), ("f32", dict(cn_offset=inf)), ("f32", dict(cn_offset=-0.25)),
                     ("i8", dict(cn_scale=0.03)), ("i8", dict(cn_scale=1.0, cn_offset=32.0))):
        with pytest.raises(E.LdpcError) as e:
            E.Decoder(code, "min", cell, 8, schedule="layered", **kw)
        assert e.value.code == -1 and ("cn_scale" in str(e.value) or "cn_offset" in str(e.value)), (cell, kw, str(e.value))
    for name in ("ldpc/hip-minsum-i8-s1-o0.5/moon.7.13/20", "ldpc/hip-minsum-s0.875/moon.7.13/20", "ldpc/hip-tanh-layered-s1/moon.7.13/20",
                 "ldpc/hip-minsum-layered-i8-o0.5-s1/moon.7.13/20", "ldpc/hip-minsum-layered-i8-s1.0.0/moon.7.13/20"):
        with pytest.raises(E.LdpcError) as e:
            E.ECC(CODES, name, max_batch=4)
        assert e.value.code == -8, (name, str(e.value))
