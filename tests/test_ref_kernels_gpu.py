"""The float `cuda-arraylet2` route against the REFERENCE'S OWN KERNELS: cudabits/arraylet2.cu + common.h compiled for gfx950 by
oracle/ref_kernels.py (build() does it where a checkout of the reference lies) and launched by tests/ref_kernels.py with the
reference's launch shapes.  Until here the oracle variant "cuda32", oracle/literal.py::ldpc_cuda_arraylet2 and the device mode
LDPC_TANH_CUDA32 were three readings of those files by the same readers; a misreading shared by all three passed every test.

a, b: the rotation, column side and row side, against c.graph's edge list alone.  c: one check-node update from the oracle's states,
the reference's kernel against the oracle and the project's device mode against the reference's kernel.  d: one variable-node update,
bit for bit.  e: free-running decodes through the reference's launch sequence (Arraylet2.hs:151-273, restated here).  f: its parity
kernel where the answer does not depend on workgroup order.  cudabits/two_arrays.cu's selfProduct is not built (oracle/ref_kernels.py
says why).  Nothing here reads the reference's checkout: every test skips when oracle/_ref/arraylet2.co is absent."""
import functools

import numpy as np
import pytest

from oracle import literal, oracle
from tests import ref_kernels as rk
from tests.helpers import load, synthetic

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rk.available(), reason="oracle/_ref/arraylet2.co is absent: build() makes it where a checkout of the reference lies")]

ONE_LAUNCH = ["jpl.1024.4.5", "small-2x4-sz32", "jpl.4096.4.5"]       # rowCount x colCount x sz: 384 x 44 x 32, 64 x 4 x 32, 1536 x 44 x 128
FREE_RUNNING = ["jpl.1024.4.5", "small-2x4-sz32"]
CLAMP32 = np.float32(rk.CLAMP)


def code(name):
    return load(name) if name.startswith("jpl.") else synthetic(name)


@functools.lru_cache(maxsize=None)
def slots(name):
    c = code(name)
    return rk.edge_slots(c.graph, c.sz, c.offsets)


@pytest.fixture
def ref(request, hip):
    c = code(request.param)
    r = rk.RefArraylet2(c.sz, c.offsets)
    r.code = c
    yield r
    r.check_guards()              # the fill pattern on both sides of every buffer the test used
    r.close()


def to_slots(name, per_edge):
    """edge order -> [rowCount * colCount] float32, absent slots 0"""
    c = code(name)
    a = np.zeros(c.M * c.offsets.shape[1], np.float32)
    a[slots(name)] = np.asarray(per_edge, np.float32)
    return a


def test_the_launcher_refuses_what_the_kernels_would_index_out_of(hip):
    """the reference's kernels check no bounds: every refusal comes before a launch (nothing is launched in this test)"""
    ok = np.zeros((2, 4), np.int32)                                      # lam: 128 floats, mLet: 256
    for sz, offsets in ((32, np.full((1, 4), 32, np.int32)),            # an offset of sz: no rotation of a circulant of that size
                        (32, np.full((1, 4), -2, np.int32)),            # (i + sz - off) % sz of a negative number
                        (2, np.zeros((1, 4), np.int32)),                # rowCount 2: selfProduct's grid of rowCount / 4 is empty
                        (6, np.zeros((1, 4), np.int32)),                # rowCount 6: its last two rows belong to no workgroup
                        (32, np.zeros((1, 257), np.int32))):            # a workgroup of 4 * 257 threads
        with pytest.raises(ValueError, match="refused"):
            rk.RefArraylet2(sz, offsets)
    r = rk.RefArraylet2(32, ok)
    wide = rk.RefArraylet2(32, np.zeros((1, 65), np.int32))
    try:
        lam, m, done = r.lam_buf(), r.mlet_buf(), r.done_buf()
        for call in (lambda: r.selfProduct(lam, m, m),                  # one array for both
                     lambda: r.selfProduct(m, m, r.mlet_buf()),         # a buffer of another size as lam
                     lambda: r.updateLam(lam, lam),
                     lambda: r.updateLam(lam, wide.mlet_buf()),         # another launcher's buffer
                     lambda: r.tanhTransform(m, done),                  # ints for floats
                     lambda: r.parityRowResults(lam, lam),
                     lambda: r.updateLam(lam.t, m),                     # a bare tensor: no guard regions
                     lambda: wide.parityRowResults(wide.done_buf(), wide.lam_buf())):   # 65 threads: two waves at its conditional barrier
            with pytest.raises(ValueError, match="refused"):
                call()
        small = rk.RefArraylet2(4, np.zeros((1, 4), np.int32))          # rowCount 4: fine for selfProduct, no whole workgroup of tanhTransform
        with pytest.raises(ValueError, match="refused"):
            small.tanhTransform(small.mlet_buf(), small.lam_buf())
        small.close()
        r.check_guards()
    finally:
        r.close()
        wide.close()


# ---- a -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", ONE_LAUNCH, indirect=True)
def test_a_update_lam_sums_each_column_over_the_graphs_edges(ref):
    """updateLam with lam = 0 and a distinct integer in every present slot (all below 2^24: every float sum is exact) equals the
    per-column sum over c.graph's edge list -- the `sz - off` rotation of common.h:163-164 is not used to say what is expected"""
    c = ref.code
    s = slots(c.name)
    v = (s + 1).astype(np.float64)                                       # the slot's own number, from 1: absent slots hold 0
    want = np.zeros(c.N)
    np.add.at(want, c.graph.col_idx, v)
    assert want.max() < 2 ** 24
    lam, newMLet = ref.lam_buf(), ref.mlet_buf(to_slots(c.name, v))
    ref.updateLam(lam, newMLet)
    got = lam.get()
    assert np.array_equal(got, want.astype(np.float32)), np.nonzero(got != want)[0][:8]


# ---- b -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", ONE_LAUNCH, indirect=True)
def test_b_tanh_transform_reads_the_column_of_the_rows_one(ref):
    """tanhTransform with mLet = 0 and distinct lam[n] in (-4, 4): slot (j, i) is tanh(-lam[n] / 2) for n the column of H's one in row
    j, block column i -- within 2 ulp of float (the kernel rounds the device's double tanh to float; a wrong column is off by far
    more: neighbouring values differ by 8/N in lam).  Absent slots keep what they held."""
    c = ref.code
    s = slots(c.name)
    lam32 = (-4.0 + 8.0 * (np.arange(c.N) + 0.5) / c.N).astype(np.float32)
    assert len(np.unique(lam32)) == c.N and np.abs(lam32).max() < 4
    before = np.full(c.M * c.offsets.shape[1], 7.0, np.float32)          # 7: no tanh; present slots 0
    before[s] = 0
    mLet, lam = ref.mlet_buf(before), ref.lam_buf(lam32)
    ref.tanhTransform(mLet, lam)
    got = mLet.get()
    want = np.tanh(-(lam32[c.graph.col_idx].astype(np.float64)) / 2).astype(np.float32)
    err = np.abs(got[s].astype(np.float64) - want) / np.spacing(np.abs(want))
    print(f"{c.name}: tanhTransform worst error {err.max():.2f} ulp of float, {np.mean(got[s] == want):.4f} of the slots identical")
    assert err.max() <= 2
    absent = np.ones(len(got), bool)
    absent[s] = False
    assert (got[absent] == 7.0).all()


# ---- c, d: teacher-forced states ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def states(name):
    """(orig, lam, ne, ne', lam') as tests/test_cuda32_gpu.py builds them: the oracle's cuda32 traces of one frame each at 2.0, 3.5 and
    6.0 dB, first six turns, and last the `strong` state (|LLR| 15..30), where the clamp fires.  Computed once, never written to."""
    c = code(name)
    llr = np.concatenate([c.frames(8, db, 6300 + i)[1] for i, db in enumerate((2.0, 3.5, 6.0))]).astype(np.float32)
    out = []
    for f in (0, 9, 17):
        o = oracle.decode(c.graph, "cuda32", 6, llr[f].astype(np.float64), trace=True)
        ne = np.zeros(c.E)
        for n in range(o["iters"]):
            out.append((llr[f].astype(np.float64), o["trace_lam"][n], ne, o["trace_ne"][n], o["trace_lam"][n + 1]))
            ne = o["trace_ne"][n]
    rng = np.random.default_rng(7)
    strong = (np.where(rng.random(c.N) < 0.5, 1.0, -1.0) * rng.uniform(15.0, 30.0, c.N)).astype(np.float32).astype(np.float64)
    ne2, lam2, _ = oracle.step(c.graph, "cuda32", strong, strong, np.zeros(c.E))
    out.append((strong, strong, np.zeros(c.E), ne2, lam2))
    for s in out:
        for a in s:
            a.setflags(write=False)
    return out


def held_to(got, want, what):
    """the bars of tests/test_cuda32_gpu.py: relative 1e-5 away from the clamp, absolute 1.5 within 3.0 of it (there a message is the
    atanh of a float an ulp from 1: an ulp of the product moves it by ~0.35) -> (worst relative error away from it, share identical)"""
    near = np.abs(np.abs(want) - rk.CLAMP) < 3.0
    rel = np.abs(got - want) / np.maximum(1, np.abs(want))
    worst, worst_near = rel[~near].max(initial=0), np.abs(got - want)[near].max(initial=0)
    assert worst <= 1e-5 and worst_near <= 1.5, (what, worst, worst_near)
    return worst, float(np.mean(got == want))


@pytest.mark.parametrize("ref", ONE_LAUNCH, indirect=True)
def test_c_self_product_against_the_oracle_and_the_device_mode_against_it(ref, hip):
    c = ref.code
    st, s = states(c.name), slots(c.name)
    lam, mLet, newMLet = ref.lam_buf(), ref.mlet_buf(), ref.mlet_buf()
    present = np.zeros(mLet.n, bool)
    present[s] = True
    kernel = []
    for orig, l, ne, _, _ in st:
        lam.put(l.astype(np.float32))
        mLet.put(to_slots(c.name, ne))
        newMLet.t.zero_()
        ref.selfProduct(lam, mLet, newMLet)
        out = newMLet.get()
        assert (out[~present] == 0).all()                                # arraylet2.cu:65: an absent slot is not written
        kernel.append(out[s].astype(np.float64))
    dec = hip.Decoder(c.hip_code(hip), "cuda32", "f32", len(st))
    dn, _, _ = dec.debug_step(np.stack([x[0] for x in st]), np.stack([x[1] for x in st]), np.stack([x[2] for x in st]))
    dec.close()
    a = [held_to(kernel[i], x[3], (c.name, "reference kernel vs oracle", i)) for i, x in enumerate(st)]
    b = [held_to(dn[i], kernel[i], (c.name, "device mode vs reference kernel", i)) for i in range(len(st))]
    # the strong state: the messages exactly at the clamp are the same ones in all three
    at = [np.abs(x) == CLAMP32 for x in (st[-1][3], kernel[-1], dn[-1])]
    assert at[0].sum() > 0 and np.array_equal(at[0], at[1]) and np.array_equal(at[1], at[2])
    for what, r in (("reference kernel vs oracle cuda32", a), ("device mode LDPC_TANH_CUDA32 vs reference kernel", b)):
        print(f"{c.name} {what}: worst relative error away from the clamp {max(x[0] for x in r):.2e}, "
              f"{np.mean([x[1] for x in r]):.4f} of the messages bit-identical, over {len(st)} updates ({int(at[0].sum())} messages at the clamp)")


@pytest.mark.parametrize("ref", ONE_LAUNCH, indirect=True)
def test_d_update_lam_is_the_oracles_next_lam_bit_for_bit(ref):
    """lam <- the channel floats, newMLet <- the oracle's messages as floats: updateLam is IEEE float addition in ascending block-row
    order with no library call in it, so its output EQUALS the oracle's next lam"""
    c = ref.code
    lam, newMLet = ref.lam_buf(), ref.mlet_buf()
    for i, (orig, _, _, ne2, lam2) in enumerate(states(c.name)):
        lam.put(orig.astype(np.float32))
        newMLet.put(to_slots(c.name, ne2))
        ref.updateLam(lam, newMLet)
        got = lam.get()
        assert np.array_equal(got, lam2.astype(np.float32)), (c.name, i, int((got != lam2.astype(np.float32)).sum()))


# ---- e -------------------------------------------------------------------------------------------------------------------------------
def free_running_frames(name):
    c = code(name)
    if name == "jpl.1024.4.5":
        return np.concatenate([c.frames(8, db, 6300 + i)[1] for i, db in enumerate((2.0, 3.5, 6.0))]).astype(np.float32), 40
    return np.concatenate([c.frames(4, db, 6100 + i)[1] for i, db in enumerate((1.0, 3.0, 6.0))]).astype(np.float32), 15


def reference_decode(ref, bufs, orig32, max_iterations):
    """the closure of GPU/CUDA/Arraylet2.hs:151-273 with the reference's kernels; -> (bits, turns, converged).  bufs: [lam, orig,
    mLet, newMLet], allocated once per decoder as at :119-138 (mLet and newMLet change places at every turn and stay so between
    frames; newMLet is never cleared)"""
    c = ref.code
    lam, orig = bufs[0], bufs[1]
    orig.put(orig32)                                                     # :158
    lam.put(orig32)                                                      # :159
    bufs[2].t.zero_()                                                    # :164-165 memset mLet'
    iters = 0
    while True:                                                          # :167 go
        if iters >= max_iterations:                                      # :168 the result is orig_lam_dev
            return (orig.get() > 0).astype(np.uint8), iters, False       # :273 hard (common.h:180-182 / Reference.hs: v > 0)
        # :176-193 parityRowResults and `done > 0`: some row of H . hard(lam) is odd.  Taken on the host from lam read back, with
        # c.graph: row 0's workgroup resets *done and may run after another row has set it (test f), so the kernel's answer is not
        # the decision when workgroups race
        h = (lam.get() > 0).astype(np.int64)
        parity = bool((np.add.reduceat(h[c.graph.col_idx], c.graph.row_ptr[:-1]) & 1).any())
        if not parity:                                                   # :196-198 the result is lam_dev
            return h.astype(np.uint8), iters, True
        ref.selfProduct(lam, bufs[2], bufs[3])                           # :214-226
        lam.t.copy_(orig.t)                                              # :242 copyArray orig_lam_dev lam_dev
        bufs[2], bufs[3] = bufs[3], bufs[2]                              # :244 swapRefs
        ref.updateLam(lam, bufs[2])                                      # :248-262 with `newMLet` as bound at :171: what selfProduct wrote
        iters += 1                                                       # :264


def agree(got, want, what):
    """the bars of test_parity_mode_against_the_oracle_variant: flags equal on >= 95 % of the frames, hard bits equal on those, turn
    counts equal on >= 90 % of those and nowhere more than one apart"""
    (b, it, cv), (ob, oi, oc) = got, want
    same = cv.astype(bool) == oc.astype(bool)
    assert same.mean() >= 0.95 and np.array_equal(b[same], ob[same]), (what, same.mean())
    assert (it[same] == oi[same]).mean() >= 0.9 and np.abs(it[same].astype(int) - oi[same].astype(int)).max() <= 1, what
    return f"{what}: flags equal on {int(same.sum())}/{len(same)} frames, bits equal on those, turns equal on {int((it[same] == oi[same]).sum())}"


@pytest.mark.parametrize("ref", FREE_RUNNING, indirect=True)
def test_e_free_running_decode_through_the_references_launch_sequence(ref):
    c = ref.code
    llr, turns = free_running_frames(c.name)
    want = oracle.decode_batch(c.graph, "cuda32", turns, llr.astype(np.float64), nthreads=8)
    assert 0 < want[2].sum() < len(llr), "the frames must leave the oracle with converged and unconverged ones"   # the 5 % is a cap
    bufs = [ref.lam_buf(), ref.lam_buf(), ref.mlet_buf(), ref.mlet_buf()]
    out = [reference_decode(ref, bufs, llr[f], turns) for f in range(len(llr))]
    got = (np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]))
    print(agree(got, want, f"{c.name} reference kernels vs oracle cuda32"))
    if c.name == "small-2x4-sz32":
        lit = [literal.ldpc_cuda_arraylet2(c.sz, c.offsets, turns, llr[f]) for f in range(len(llr))]
        lit = (np.stack([o[0] for o in lit]), np.array([o[1] for o in lit]), np.array([o[2] for o in lit]))
        print(agree(got, lit, f"{c.name} reference kernels vs oracle/literal.py"))


# ---- f -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", ONE_LAUNCH, indirect=True)
def test_f_parity_row_results_where_workgroup_order_cannot_matter(ref):
    """Row 0's workgroup writes *done = 0 (common.h:217-219) whenever it runs, also after another row's workgroup has written 1: in
    general the kernel's answer depends on the order in which workgroups run.  Only two cases do not.  A codeword: no row writes 1, row
    0 writes 0, so a 1 put there beforehand must be gone.  A word that leaves ROW 0 unsatisfied: row 0's own workgroup writes 0 and
    then 1, every other workgroup writes 1 or nothing, so the answer is 1 in every order.  Nothing else is asserted, and the launch is
    not repeated to look for the race."""
    c = ref.code
    if c.name.startswith("jpl."):
        cw = c.encode(np.random.default_rng(31).integers(0, 2, c.k).astype(np.uint8))
    else:
        cw = np.zeros(c.N, np.uint8)
    assert not (np.add.reduceat(cw[c.graph.col_idx].astype(np.int64), c.graph.row_ptr[:-1]) & 1).any()
    word = np.where(cw > 0, 3.0, -3.0).astype(np.float32)               # hard(v) = v > 0
    lam, done = ref.lam_buf(word), ref.done_buf(1)
    ref.parityRowResults(done, lam)
    assert done.get()[0] == 0
    n = c.graph.col_idx[c.graph.row_ptr[0] + 1]                          # a column of row 0's support
    word[n] = -word[n]
    lam.put(word)
    done.put(np.array([0], np.int32))
    ref.parityRowResults(done, lam)
    assert done.get()[0] == 1
