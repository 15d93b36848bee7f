"""GPU: the two-stage decode (ldpc_cascade_create / ldpc_cascade_decode_dev, csrc/cascade.hip) against its specification
tests/cascade_spec.py, np.array_equal everywhere.  The expected result is always cascade_spec.compose over decoders that exist without the
cascade: each context's own plain decode_batch on the GPU, called once on the full batch and once on the failed rows -- and, for the pair the
feature was written for, the two CPU specifications those kernels reproduce bit for bit.

Pairs: (a) codes/jpl.1024.4.5 as CSR, fp16 cells, 3/4 min-sum then A-min*; (b) the same H handed over quasi-cyclic to the on-chip layered
kernel, then the CSR A-min* f32 context -- two code objects of one H; (c) "w20" of tests/layered_shapes.py (N = 4099, odd: fp16 and int8
rows sit at every alignment), int8 then f32 A-min* fed f32 and fp16 LLRs, int8 then int8 with another scale fed int8 LLRs; (d)
codes/1920.1280.3.303, flooding min-sum then flooding tanh."""
import functools

import numpy as np
import pytest

from oracle import channel
from tests import cascade_spec as spec
from tests import layered_aminstar_spec as aminstar
from tests import layered_i8_spec as i8
from tests import layered_rule_spec as rule
from tests import layered_shapes as S
from tests.helpers import load

pytestmark = pytest.mark.gpu

SWEEPS = 20
NAMES = ("bits", "iters", "converged", "stage", "stats")


@functools.lru_cache(maxsize=None)
def _jpl_frames():
    """the stream tests/test_cascade_spec.py draws: all-zero frames of codes/jpl.1024.4.5 at 3.0 dB, seed 5; shared, never written"""
    llr = channel.frames(np.zeros((600, 1408), np.uint8), 3.0, 1024, 1280, 1408, seed=5).astype(np.float32)
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def _w_frames(name, F, db, seed=300):
    llr = S.case(name).frames(F, db, seed)
    llr.setflags(write=False)
    return llr


def _csr_code(hip, c):
    return hip.Code.from_csr(c.graph.row_ptr, c.graph.col_idx, c.N)


def _pair_a(hip, F, cell="f16"):
    c = load("jpl.1024.4.5")
    d1 = hip.Decoder(_csr_code(hip, c), "min", cell, F, schedule="layered", path="fused")
    d2 = hip.Decoder(_csr_code(hip, c), "min", cell, F, schedule="layered", cn_rule="aminstar")
    assert d1.kernel_name == "ldpc::layered_csr_kernel<20>" and "MinStar<" in d2.kernel_name, (d1.kernel_name, d2.kernel_name)
    return d1, d2


def _stage(dec, max_iters):
    return lambda x: dec.decode_batch(np.ascontiguousarray(x), max_iters)


def _same(got, want, what):
    for n, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, n, g, w)


def _check(hip, cas, llr, mi1, mi2, what):
    """one cascade call against compose over the two contexts' own decode_batch -> the result"""
    want = spec.compose(_stage(cas.dec1, mi1), _stage(cas.dec2, mi2), llr, cas.capacity)
    got = cas.decode_batch(np.array(llr), mi1, mi2)             # (writable: the arrays travel through torch tensors)
    _same(got, want, what)
    return got


def _share_ok(stats, F):
    return 0.05 * F <= int(stats[0]) <= 0.60 * F


def test_pair_a_against_the_cpu_specifications_and_the_contexts(hip):
    F = 256
    llr = _jpl_frames()[:F]
    g = load("jpl.1024.4.5").graph
    d1, d2 = _pair_a(hip, F)
    cas = hip.Cascade(d1, d2)
    assert cas.capacity == F and cas.nbytes >= F * 1408 * 5
    got = _check(hip, cas, llr, SWEEPS, SWEEPS, "pair a")
    want = spec.compose(lambda x: rule.decode_float(g, x, SWEEPS, 0.75, 0.0, "f16"), lambda x: aminstar.decode_float(g, x, SWEEPS, "f16"), llr, F)
    _same(got, want, "pair a, CPU specifications")
    bits, iters, conv, stage, stats = got
    assert _share_ok(stats, F) and stats[1] == stats[0] and 0 < stats[2] < stats[1], stats      # some go on, some of them are repaired, some fail again
    assert np.array_equal(stage == 2, d1.decode_batch(llr, SWEEPS)[2] == 0)
    assert (bits[:, :1024] != 0).any(axis=1).sum() < (d1.decode_batch(llr, SWEEPS)[0][:, :1024] != 0).any(axis=1).sum()
    cas.close(); d1.close(); d2.close()


def test_pair_b_quasi_cyclic_on_chip_then_csr_aminstar(hip):
    F = 256
    llr = _jpl_frames()[:F]
    c = load("jpl.1024.4.5")
    d1 = hip.Decoder(hip.Code.from_qc(c.sz, c.offsets), "min", "f32", F, schedule="layered")
    d2 = hip.Decoder(_csr_code(hip, c), "min", "f32", F, schedule="layered", cn_rule="aminstar")
    assert d1.path == "fused" and "fused_layered_kernel" in d1.kernel_name, d1.kernel_name
    assert d2.kernel_name == "ldpc::layered_csr_kernel<20, ldpc::MinStar<float>>", d2.kernel_name
    cas = hip.Cascade(d1, d2, F // 2)
    got = _check(hip, cas, llr, SWEEPS, SWEEPS, "pair b")
    assert _share_ok(got[4], F) and got[4][1] == got[4][0] and got[4][2] < got[4][1], got[4]
    cas.close(); d1.close(); d2.close()


def test_pair_c_odd_n_every_alignment_and_input_format(hip):
    name, F, mi = "w20", 48, 12
    g = S.case(name)
    assert g.N % 2 == 1
    llr = _w_frames(name, F, 5.0)
    d1 = hip.Decoder(g.code(hip, g.layer_ptr), "min", "i8", F, schedule="layered")
    d2 = hip.Decoder(g.code(hip, g.layer_ptr), "min", "f32", F, schedule="layered", cn_rule="aminstar")
    d3 = hip.Decoder(g.code(hip, g.layer_ptr), "min", "i8", F, schedule="layered", cn_scale=0.875)
    cas = hip.Cascade(d1, d2)
    for x in (llr, llr.astype(np.float16)):
        got = _check(hip, cas, x, mi, mi, (name, str(x.dtype)))
        assert _share_ok(got[4], F), got[4]
    cas8 = hip.Cascade(d1, d3, F - 1)
    q = i8.quantize(llr, 4.0).astype(np.int8)                   # (-127 .. 127: what an "i8" context makes of these LLRs)
    got = _check(hip, cas8, q, mi, mi, (name, "int8"))
    assert _share_ok(got[4], F), got[4]
    # int8 LLRs need two int8 contexts: refused up front, nothing decoded
    with pytest.raises(hip.LdpcError) as e:
        cas.decode_batch(q.copy(), mi, mi)
    assert e.value.code == -5 and "llr_fmt" in str(e.value)
    for o in (cas, cas8, d1, d2, d3):
        o.close()


def test_pair_d_flooding_min_sum_then_tanh(hip):
    F = 64
    c = load("1920.1280.3.303")
    _, llr = c.frames(F, 1.5, seed=31)                          # (the CPU oracle: 9 of these 64 are not converged after 30 min-sum turns)
    llr = llr.astype(np.float32)
    d1 = hip.Decoder(c.hip_code(hip, prefer_qc=False), "min", "f32", F)
    d2 = hip.Decoder(c.hip_code(hip, prefer_qc=False), "tanh", "f32", F)
    assert d1.schedule == d2.schedule == "flooding"
    cas = hip.Cascade(d1, d2, 32)
    got = _check(hip, cas, llr, 30, 50, "pair d")
    assert _share_ok(got[4], F) and got[4][1] == got[4][0], got[4]
    cas.close(); d1.close(); d2.close()


def test_batch_sizes_capacities_and_a_cascade_used_again(hip):
    """batches of 1, 63, 64, 65 and 257 on ONE cascade, one after the other: padding and idx of a call must not leak into the next; then the
    capacity at, one below and far below the number of failures; then a batch without a failure"""
    F = 257
    llr = _jpl_frames()[:F]
    d1, d2 = _pair_a(hip, F)
    cas = hip.Cascade(d1, d2)
    for n in (257, 1, 63, 64, 65):
        _check(hip, cas, llr[F - n:], SWEEPS, SWEEPS, ("batch", n))
    full = _check(hip, cas, llr[:256], SWEEPS, SWEEPS, "capacity = batch")
    failed = np.flatnonzero(full[3] == 2)
    n = int(full[4][0])
    assert n == len(failed) >= 3
    ok = int(np.flatnonzero(full[3] == 1)[0])
    assert _check(hip, cas, llr[ok:ok + 1], SWEEPS, SWEEPS, "a batch of one that sends nothing")[4].tolist() == [0, 0, 0]
    assert _check(hip, cas, llr[failed[0]:failed[0] + 1], SWEEPS, SWEEPS, "a batch of one that goes on")[4][:2].tolist() == [1, 1]
    cas.close()
    for cap in (n, n - 1, 1):
        cas = hip.Cascade(d1, d2, cap)
        assert cas.capacity == cap
        bits, iters, conv, stage, stats = _check(hip, cas, llr[:256], SWEEPS, SWEEPS, ("capacity", cap))
        assert stats[0] == n and stats[1] == cap
        assert np.array_equal(np.flatnonzero(stage == 2), failed[:cap])           # the first `cap` in frame order; the others keep stage 1's result
        assert not conv[failed[cap:]].any() and (iters[failed[cap:]] == SWEEPS).all()
        # the next call on the same cascade has no failure: the noiseless codeword repeated
        clean = np.full((40, 1408), -8.0, np.float32)
        got = _check(hip, cas, clean, SWEEPS, SWEEPS, "no failure")
        assert got[4].tolist() == [0, 0, 0] and (got[3] == 1).all() and got[2].all() and not got[0].any() and not got[1].any()
        cas.close()
    d1.close(); d2.close()


@pytest.mark.parametrize("F", [1025, 2049])
def test_past_the_select_kernels_chunks(hip, F):
    """more frames than one, and than two, chunks of the select kernel's 1024; max_iters1 = 0 sends every frame on"""
    g = S.case("w8")
    llr = np.tile(_w_frames("w8", 64, 5.0), (-(-F // 64), 1))[:F].copy()
    edge = sorted({0, 1023, 1024, F - 1})
    llr[edge] = -8.0                                           # frames that stop before the first sweep, at the chunk edges
    d1 = hip.Decoder(g.code(hip, g.layer_ptr), "min", "f16", F, schedule="layered", path="fused")
    d2 = hip.Decoder(g.code(hip, g.layer_ptr), "min", "f16", F, schedule="layered", cn_rule="aminstar")
    cas = hip.Cascade(d1, d2)
    got = _check(hip, cas, llr, 0, 6, ("w8", F))
    assert got[4][0] == got[4][1] == F - len(edge) and (got[3][edge] == 1).all()
    cas.close()
    cap = {1025: 1000, 2049: 1030}[F]                          # overflow: the cut falls inside the first chunk, inside the second
    cas = hip.Cascade(d1, d2, cap)
    got = _check(hip, cas, llr, 0, 6, ("w8", F, "capacity", cap))
    assert got[4][0] == F - len(edge) and got[4][1] == cap < got[4][0] and int((got[3] == 2).sum()) == cap
    cas.close(); d1.close(); d2.close()


def test_null_outputs_and_the_callers_stream(hip):
    import torch
    F = 96
    llr = _jpl_frames()[300:300 + F]
    d1, d2 = _pair_a(hip, F)
    cas = hip.Cascade(d1, d2, 40)
    want = _check(hip, cas, llr, SWEEPS, SWEEPS, "all outputs")
    assert want[4][1] > 0
    dev = torch.device("cuda", 0)
    d_llr = torch.from_numpy(llr.copy()).to(dev)

    def run(skip=(), stream=None):
        out = {"bits": torch.zeros((F, 1408), dtype=torch.uint8, device=dev), "iters": torch.full((F,), -7, dtype=torch.int32, device=dev),
               "converged": torch.full((F,), 9, dtype=torch.uint8, device=dev), "stage": torch.full((F,), 9, dtype=torch.uint8, device=dev),
               "stats": torch.full((3,), -7, dtype=torch.int32, device=dev)}
        torch.cuda.synchronize(dev)
        p = {k: (None if k in skip else v.data_ptr()) for k, v in out.items()}
        cas.decode_batch_dev(d_llr.data_ptr(), p["bits"], F, SWEEPS, SWEEPS, p["iters"], p["converged"], p["stage"], p["stats"], stream.cuda_stream if stream else None)
        stream.synchronize() if stream else d1.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    fresh = {"iters": -7, "converged": 9, "stage": 9, "stats": -7}
    for skip in ((), ("iters",), ("converged",), ("stage",), ("stats",), ("iters", "converged", "stage", "stats")):
        got = run(skip)
        for n, w in zip(NAMES, want):
            if n in skip:
                assert (got[n] == fresh[n]).all(), (skip, n)  # not written
            else:
                assert np.array_equal(got[n].view(w.dtype), w), (skip, n)
    got = run(stream=torch.cuda.Stream(dev))
    for n, w in zip(NAMES, want):
        assert np.array_equal(got[n].view(w.dtype), w), ("caller's stream", n)
    cas.close(); d1.close(); d2.close()


def test_one_context_twice(hip):
    """ctx1 == ctx2: few sweeps, then many, on the same context"""
    F = 64
    llr = _jpl_frames()[:F]
    d1, d2 = _pair_a(hip, F)
    cas = hip.Cascade(d2, d2)
    got = _check(hip, cas, llr, 3, SWEEPS, "one context")
    assert got[4][0] > got[4][2]
    cas.close(); d1.close(); d2.close()


def test_refusals_name_the_argument(hip):
    import torch
    F = 8
    d1, d2 = _pair_a(hip, F)
    g = S.case("w8")
    other = hip.Decoder(g.code(hip, g.layer_ptr), "min", "f16", F, schedule="layered")
    L = hip.lib()

    def refused(call, code, word):
        with pytest.raises(hip.LdpcError) as e:
            call()
        assert e.value.code == code and word in str(e.value), (word, str(e.value))

    refused(lambda: hip.Cascade(None, d2, 1), -1, "ctx1")
    refused(lambda: hip.Cascade(d1, None, 1), -1, "ctx2")
    refused(lambda: hip.Cascade(d1, other), -1, "N = ")
    for cap in (0, -1, F + 1):
        refused(lambda: hip.Cascade(d1, d2, cap), -1, "capacity")
    if L.ldpc_device_count() > 1:
        far = hip.Decoder(_csr_code(hip, load("jpl.1024.4.5")), "min", "f16", F, schedule="layered", device=1)
        refused(lambda: hip.Cascade(d1, far), -1, "device")
        far.close()
    cas = hip.Cascade(d1, d2)
    dev = torch.device("cuda", 0)
    d_llr = torch.full((F, 1408), -8.0, dtype=torch.float32, device=dev)
    d_bits = torch.full((F, 1408), 5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    a, b = d_llr.data_ptr(), d_bits.data_ptr()
    refused(lambda: cas.decode_batch_dev(a, b, -1, 1, 1), -1, "batch")
    refused(lambda: cas.decode_batch_dev(a, b, F + 1, 1, 1), -1, "batch")
    refused(lambda: cas.decode_batch_dev(a, b, F, -1, 1), -1, "max_iters1")
    refused(lambda: cas.decode_batch_dev(a, b, F, 1, -2), -1, "max_iters2")
    refused(lambda: cas.decode_batch_dev(a, b, F, 1, 1, llr_fmt=7), -1, "llr_fmt")
    refused(lambda: cas.decode_batch_dev(a, None, F, 1, 1), -1, "d_bits")
    refused(lambda: cas.decode_batch_dev(None, b, F, 1, 1), -1, "d_llr")
    refused(lambda: cas.decode_batch_dev(a + 2, b, F - 1, 1, 1), -1, "aligned")
    refused(lambda: cas.decode_batch_dev(a, b, F, 1, 1, llr_fmt="i8"), -5, "llr_fmt")
    assert L.ldpc_cascade_decode_dev(None, 1, 1, F, a, 0, b, None, None, None, None, None) == -1 and "cascade" in hip.last_error()
    assert L.ldpc_cascade_capacity(None) == -1 and L.ldpc_cascade_bytes(None) == 0
    cas.decode_batch_dev(None, None, 0, 1, 1)                  # batch = 0 succeeds and touches nothing
    d1.synchronize()
    assert (d_bits.cpu().numpy() == 5).all()                   # no refused call wrote anything
    cas.decode_batch_dev(a, b, F, 1, 1)
    d1.synchronize()
    assert not d_bits.cpu().numpy().any()
    # a cascade whose context is gone refuses; destroying it is still fine
    other2 = hip.Decoder(_csr_code(hip, load("jpl.1024.4.5")), "min", "f16", F, schedule="layered")
    gone = hip.Cascade(d1, other2)
    other2.close()
    refused(lambda: gone.decode_batch_dev(a, b, F, 1, 1), -1, "ctx2")
    gone.close()
    cas.close(); d1.close(); d2.close(); other.close()


def test_the_contexts_outlive_their_cascade(hip):
    F = 32
    llr = _jpl_frames()[:F]
    d1, d2 = _pair_a(hip, F)
    before = d1.decode_batch(llr, SWEEPS), d2.decode_batch(llr, SWEEPS)
    cas = hip.Cascade(d1, d2, 7)
    _check(hip, cas, llr, SWEEPS, SWEEPS, "before the destroy")
    cas.close()
    cas.close()                                                # (idempotent)
    after = d1.decode_batch(llr, SWEEPS), d2.decode_batch(llr, SWEEPS)
    for x, y in zip(before[0] + before[1], after[0] + after[1]):
        assert np.array_equal(x, y)
    d1.close(); d2.close()
