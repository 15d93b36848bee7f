"""CPU: the specification of product constellations (tests/product_modulation_spec.py) against the table rule of
tests/modulation_spec.py, against its own float64 formula and against the properties a demapper must have, and the host-only product
object of the built library (ldpc_modulation_create_product, ldpc_modulation_axis_levels; no GPU needed).

Bounds, with u = 2^-24:
  per-axis against the table rule   the table rule on the materialised points is exactly fl(fl(fl(m0 + E) - fl(m1 + E)) inv) (E = the
      smallest e of the other axis; asserted bit for bit), the per-axis rule is fl(fl(m0 - m1) inv).  The first carries the roundings
      of the two sums (u (m0 + E), u (m1 + E)), of the difference and of the product (u |m0 - m1| each), the second those of its
      difference and product: five roundings, |difference| <= u inv (m0 + m1 + 2 E + 4 |m0 - m1|) to first order.  The test allows
      the second-order terms a factor 1 + 1e-6 and one denormal step.
  per-axis float32 against float64  dx = fl(y - a) rounds once and enters squared, the product rounds once: each e_l is within 3 u e_l;
      the difference and the product with inv round once each (u |m0 - m1| both, to first order): |error| <= (3 u (m0 + m1) +
      2 u |m0 - m1|) inv <= 5 u (m0 + m1) inv, plus one ulp of the result for the rounding of inv itself."""
import ctypes as C

import numpy as np
import pytest

import ecc_ldpc_amd as E
from tests import modulation_spec as ms
from tests import product_modulation_spec as ps

U = 2.0 ** -24


def _uneven(b, seed):
    """a non-uniform level set [2^b], labels shuffled, no two levels equal"""
    rng = np.random.default_rng(seed)
    lev = np.sort(rng.uniform(-1.5, 1.5, 1 << b)) + np.arange(1 << b) * 0.05
    return rng.permutation(lev).astype(np.float32)


def _level_sets(b):
    """name -> (levels_i, levels_q): equal uniform axes, unequal scaling, two different non-uniform sets"""
    n = 1 << b
    uni = ((2.0 * np.arange(n) - (n - 1)) / np.sqrt(2.0 * (n * n - 1) / 3.0)).astype(np.float32)
    return {"uniform": (uni, uni), "scaled": (uni, (uni * np.float32(0.37)).astype(np.float32)), "uneven": (_uneven(b, 10 + b), _uneven(b, 20 + b))}


def _samples(li, lq, n, seed, spread=0.3):
    """[n][2] float32: a point plus noise; from the front: every point itself, +-0, a coordinate exactly on a level with the other off
    it, the midpoint of every pair of neighbouring levels on either axis"""
    rng = np.random.default_rng(seed)
    pts = ps.materialise(li, lq)
    y = (pts[rng.integers(0, len(pts), n)] + rng.normal(0.0, spread, (n, 2))).astype(np.float32)
    sp = [pts, np.array([[0.0, 0.0], [-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0]], np.float32)]
    for ax, lev in ((0, li), (1, lq)):
        s = np.sort(lev)
        mid = ((s[1:] + s[:-1]) * np.float32(0.5)).astype(np.float32)
        for vals in (lev, mid):
            blk = np.full((len(vals), 2), np.float32(0.123), np.float32)
            blk[:, ax] = vals
            sp.append(blk)
    sp = np.concatenate(sp)
    assert len(sp) < n
    y[:len(sp)] = sp
    return y


@pytest.mark.parametrize("b", [1, 2, 3])
@pytest.mark.parametrize("which", ["uniform", "scaled", "uneven"])
def test_relation_to_the_table_rule(b, which):
    li, lq = _level_sets(b)[which]
    pts = ps.materialise(li, lq)
    assert ms.bits_per_symbol(pts) == 2 * b
    worst, equal = 0.0, []
    for nv, spread in ((0.09, 0.3), (1e-3, 0.3), (0.5, 1.0)):
        y = _samples(li, lq, 4096, 31 * b + len(which), spread)
        table = ms.symbol_llrs(pts, y, nv)
        exact = ps.two_d_from_axes(li, lq, y, nv)
        assert np.array_equal(table.view(np.uint32), exact.view(np.uint32)), "the table rule is not fl(fl(fl(m0 + E) - fl(m1 + E)) inv)"
        axis = ps.symbol_llrs(li, lq, y, nv)
        inv = float(np.float32(1.0 / (2.0 * nv)))
        (i0, i1), (q0, q1) = ps.axis_mins(li, y[:, 0]), ps.axis_mins(lq, y[:, 1])
        eI, eQ = np.minimum(i0[:, :1], i1[:, :1]).astype(np.float64), np.minimum(q0[:, :1], q1[:, :1]).astype(np.float64)
        m0, m1 = np.concatenate([i0, q0], 1).astype(np.float64), np.concatenate([i1, q1], 1).astype(np.float64)
        other = np.concatenate([np.broadcast_to(eQ, i0.shape), np.broadcast_to(eI, q0.shape)], 1)
        bound = U * inv * (m0 + m1 + 2.0 * other + 4.0 * np.abs(m0 - m1)) * (1.0 + 1e-6) + 2.0 ** -149
        diff = np.abs(axis.astype(np.float64) - table.astype(np.float64))
        worst = max(worst, float((diff / bound).max()))
        assert (diff <= bound).all(), (b, which, nv, float((diff / bound).max()))
        equal.append(float((axis.view(np.uint32) == table.view(np.uint32)).mean()))
        assert ((axis > 0) == (table > 0))[(m0 != m1) & (table != 0)].all()
    print(f"b={b} {which}: worst |axis - table| / bound = {worst:.3f}; bitwise equal on {min(equal):.3f} .. {max(equal):.3f} of the LLRs")


@pytest.mark.parametrize("b", [1, 2, 3, 4, 5, 6])
def test_spec_against_float64(b):
    worst = 0.0
    for which, (li, lq) in _level_sets(b).items():
        for nv, spread, scale in ((0.09, 0.3, 1.0), (1e-3, 0.05, 1.0), (0.5, 1.0, 1.0), (1e-3, 0.3, 1e3)):
            y = _samples(li, lq, 4096 + (1 << (2 * b)), 17 + b, spread) * np.float32(scale)
            got = ps.symbol_llrs(li, lq, y, nv).astype(np.float64)
            want, mag = ps.symbol_llrs_f64(li, lq, y, nv)
            inv = 1.0 / (2.0 * nv)
            bound = 5.0 * U * mag * inv * (1.0 + 1e-6) + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            worst = max(worst, float((np.abs(got - want) / bound).max()))
            assert (np.abs(got - want) <= bound).all(), (b, which, nv)
    print(f"b={b}: worst |f32 - f64| / bound = {worst:.3f}")


@pytest.mark.parametrize("b", [1, 2, 3, 4, 5, 6])
def test_hard_decision_is_the_nearest_point(b):
    for which, (li, lq) in _level_sets(b).items():
        y = _samples(li, lq, 4096 + (1 << (2 * b)), 5 + b, 0.2)
        llr = ps.symbol_llrs(li, lq, y, 0.05)
        (i0, i1), (q0, q1) = ps.axis_mins(li, y[:, 0]), ps.axis_mins(lq, y[:, 1])
        m0, m1 = np.concatenate([i0, q0], 1), np.concatenate([i1, q1], 1)
        # the nearest point by the rule's own float32 distances: per axis the label of the smallest e_l
        near = []
        for lev, c in ((li, y[:, 0]), (lq, y[:, 1])):
            dx = c[:, None] - lev
            near.append(np.argmin(dx * dx, axis=1))
        label = (near[0] << b) | near[1]
        bits = (label[:, None] >> (2 * b - 1 - np.arange(2 * b))) & 1
        decided = m0 != m1
        assert decided.mean() > 0.95
        assert ((llr > 0).astype(np.int64) == bits)[decided].all(), (b, which)
        assert (llr[~decided] == 0).all()
        # and by float64 distances to the 4^b materialised points, wherever the two classes are not within rounding of a tie
        clear = np.abs(m0.astype(np.float64) - m1) > 1e-5 * (m0.astype(np.float64) + m1)
        p64 = ps.materialise(li, lq).astype(np.float64)
        for lo in range(0, len(y), 512):
            blk = y[lo:lo + 512].astype(np.float64)
            lab2 = ((blk[:, None, :] - p64[None]) ** 2).sum(-1).argmin(1)
            bits2 = (lab2[:, None] >> (2 * b - 1 - np.arange(2 * b))) & 1
            c = clear[lo:lo + 512]
            assert ((llr[lo:lo + 512] > 0).astype(np.int64) == bits2)[c].all(), (b, which)
        assert clear.mean() > 0.95


def test_nan_stays_on_its_axis():
    li, lq = _level_sets(3)["uneven"]
    y = np.array([[np.nan, 0.3], [0.3, np.nan], [np.inf, -0.2], [0.1, -np.inf], [np.nan, np.nan]], np.float32)
    llr = ps.symbol_llrs(li, lq, y, 0.1)
    nan = np.isnan(llr)
    assert nan[0, :3].all() and not nan[0, 3:].any() and nan[1, 3:].all() and not nan[1, :3].any()
    assert nan[2, :3].all() and not nan[2, 3:].any() and nan[3, 3:].all() and not nan[3, :3].any() and nan[4].all()   # inf - inf
    ref = ps.symbol_llrs(li, lq, np.array([[0.3, 0.3]], np.float32), 0.1)
    assert np.array_equal(llr[0, 3:].view(np.uint32), ref[0, 3:].view(np.uint32)) and np.array_equal(llr[1, :3].view(np.uint32), ref[0, :3].view(np.uint32))
    q = ps.demap(li, lq, y[None], 30, 33, 0.1, ps.LLR_I8)
    assert (q[0, :3] == 0).all() and (q[0, 3:6] != 0).any() and (q[0, 30:] == 0).all()


@pytest.mark.parametrize("kind", [ps.QAM64, ps.QAM256, ps.QAM1024, ps.QAM4096])
def test_builtin_levels(kind):
    b = kind // 2
    lev = ps.builtin_levels(kind)
    assert lev.shape == (1 << b,) and lev.dtype == np.float32
    es = ps.energy(lev, lev)
    print(f"kind {kind}: Es - 1 = {es - 1.0:.3e}")
    assert abs(es - 1.0) <= 1e-6
    # Gray: the labels of adjacent positions differ in exactly one bit; positions ascend in amplitude, evenly spaced
    order = np.argsort(lev)
    assert all(bin(int(order[k]) ^ int(order[k + 1])).count("1") == 1 for k in range(len(order) - 1))
    assert [int(v) for v in order] == [k ^ (k >> 1) for k in range(1 << b)]
    step = np.diff(lev[order].astype(np.float64))       # each level is rounded to float32 once: two roundings a step
    n = 1 << b
    assert (np.abs(step - 2.0 / np.sqrt(2.0 * (n * n - 1) / 3.0)) <= 2.0 * U * float(np.abs(lev).max())).all()
    assert ps.materialise(lev, lev).shape == (1 << kind, 2)


def test_builtin_levels_meet_the_shipped_tables():
    # b = 2: the level set of the 16QAM table built-in, as uint32
    l16 = ps.builtin_levels(4)
    q16 = ms.builtin(ms.QAM16)
    assert np.array_equal(ps.materialise(l16, l16).view(np.uint32), q16.view(np.uint32))
    assert np.array_equal(l16.view(np.uint32), q16[:4, 1].view(np.uint32)) and np.array_equal(l16.view(np.uint32), q16[::4, 0].view(np.uint32))
    # 64QAM: grid64's level set, up to labelling
    g = ms.grid64()
    l64 = ps.builtin_levels(ps.QAM64)
    assert np.array_equal(np.sort(l64).view(np.uint32), g[:8, 1].view(np.uint32)) and np.array_equal(np.sort(l64).view(np.uint32), g[::8, 0].view(np.uint32))
    nat = np.sort(l64)
    assert np.array_equal(ps.materialise(nat, nat).view(np.uint32), g.view(np.uint32))


def test_product_object_of_the_library():
    """host only: needs the built library, not a GPU.  Fails on a library without ldpc_modulation_create_product"""
    L = E.lib()
    for name, kind in (("64qam", ps.QAM64), ("256qam", ps.QAM256), ("1024qam", ps.QAM1024), ("4096qam", ps.QAM4096)):
        lev = ps.builtin_levels(kind)
        for mod in (E.Modulation(name), E.Modulation(kind)):
            assert mod.bits == kind
            li, lq = mod.axis_levels
            assert np.array_equal(li.view(np.uint32), lev.view(np.uint32)) and np.array_equal(lq.view(np.uint32), lev.view(np.uint32)), name
            assert np.array_equal(mod.points.view(np.uint32), ps.materialise(lev, lev).view(np.uint32))
            assert mod.energy == ps.energy(lev, lev) and abs(mod.energy - 1.0) < 1e-6
            for n_tx in (0, 1, kind, kind + 1, 1917, 1920):
                assert mod.symbols(n_tx) == ms.symbols_per_frame(n_tx, kind)
            assert L.ldpc_modulation_points(mod._h, None) == 1 << kind
            assert L.ldpc_modulation_axis_levels(mod._h, None, None) == kind // 2
            mod.close()
    for b in (1, 2, 3, 4, 5, 6):
        li, lq = _uneven(b, 40 + b), _uneven(b, 50 + b)
        mod = E.Modulation.product(li, lq)
        assert mod.bits == 2 * b
        gi, gq = mod.axis_levels
        assert np.array_equal(gi.view(np.uint32), li.view(np.uint32)) and np.array_equal(gq.view(np.uint32), lq.view(np.uint32))
        pts = ps.materialise(li, lq)
        assert np.array_equal(mod.points.view(np.uint32), pts.view(np.uint32)) and mod.energy == ps.energy(li, lq)
        only_q = np.zeros(1 << b, np.float32)
        assert L.ldpc_modulation_axis_levels(mod._h, None, only_q.ctypes.data_as(C.POINTER(C.c_float))) == b and np.array_equal(only_q, lq)
        if b <= 3:                                         # the same constellation as a table: Es, and so sigma, bit for bit
            tab = E.Modulation(pts)
            assert tab.bits == 2 * b and tab.energy == mod.energy and tab.axis_levels is None
            assert L.ldpc_modulation_axis_levels(tab._h, None, None) == 0
            tab.close()
        mod.close()
    # the 16QAM built-in stays a table object; its level set as a product object is the same constellation
    q16 = E.Modulation("16qam")
    assert q16.axis_levels is None
    l16 = ps.builtin_levels(4)
    p16 = E.Modulation.product(l16, l16)
    assert np.array_equal(p16.points.view(np.uint32), q16.points.view(np.uint32)) and p16.energy == q16.energy
    p16.close(); q16.close()
    # refusals
    ok = np.zeros(128, np.float32)
    fp = ok.ctypes.data_as(C.POINTER(C.c_float))
    for b in (0, 7, -1):
        assert not L.ldpc_modulation_create_product(b, fp, fp) and L.ldpc_last_error_code() == -1
    assert not L.ldpc_modulation_create_product(2, None, fp) and L.ldpc_last_error_code() == -1
    assert not L.ldpc_modulation_create_product(2, fp, None) and L.ldpc_last_error_code() == -1
    for bad in (np.nan, np.inf, -np.inf):
        for axis in (0, 1):
            lv = [_uneven(2, 1), _uneven(2, 2)]
            lv[axis][3] = bad
            with pytest.raises(E.LdpcError) as e:
                E.Modulation.product(*lv)
            assert e.value.code == -1
    with pytest.raises(E.LdpcError):
        E.Modulation.product(np.zeros(3, np.float32), np.zeros(3, np.float32))
    with pytest.raises(E.LdpcError):
        E.Modulation.product(np.zeros(4, np.float32), np.zeros(8, np.float32))
    assert not L.ldpc_modulation_create(7, fp) and L.ldpc_last_error_code() == -1          # tables stay at m <= 6
    for kind in (0, 5, 7, 9, 11, 13, -3):
        assert not L.ldpc_modulation_create_builtin(kind) and L.ldpc_last_error_code() == -1
    assert L.ldpc_modulation_axis_levels(None, fp, fp) == -1


def test_product_kernels_spill_nothing():
    """every instance of csrc/demap_product.hip and csrc/sim_mod_product.hip: 0 bytes of scratch, no spilled VGPR or SGPR, by the
    code-object metadata of the build's device assembly -- the check build.py makes.  6 x (3 formats x 2 store forms, less the three
    int8 cases that have no vector store) demappers, as many fused kernels, 6 transmit kernels"""
    import os

    from ecc_ldpc_amd import build as B
    objdir = os.path.join(os.path.dirname(B.__file__), "build")
    res = B.product_resources(objdir)
    assert len(res) == 33 + 33 + 6, f"{len(res)} product kernels in the device assembly of {objdir}: build first (python ecc_ldpc_amd/build.py)"
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] <= 128, (name, r)           # what the b = 6 fused instances take; 4 waves per SIMD
