"""GPU: the host-pointer entry points (ldpc_decode_batch / _f16 / _f64 / _packed on pageable buffers) in front of every
on-chip kernel family, against ONE device launch of the same frames and against the Double oracle (or its fp16 emulation).

An on-chip context whose max_batch exceeds 8192 frames does not decode a host call in one launch: api.cc splits it into
8192-frame chunks (kHostChunk) and runs them on two streams, so that one chunk's copies overlap another chunk's decode.  A
chunk that is never decoded, or decoded from another chunk's LLRs, leaves its rows with whatever the slot held before -- the
previous chunk's or the previous call's results -- so every comparison here is exact, the outputs start as sentinels, and each
entry point is called twice with different frames.  Every frame has its own noise (random codewords where the code has an
encoder), at Eb/N0 from below the waterfall to above it, so no stale row matches by accident.

Also: more than 65 535 frames in one call of the frame source and of the packed-result kernel, whose grids have a row per
frame."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ecc_ldpc_amd._lib import check, ptr
from oracle import emulate_f16 as em
from oracle import oracle
from tests.helpers import CODES, iters_agree, load, synthetic

pytestmark = pytest.mark.gpu

CHUNK = 8192                       # api.cc kHostChunk
BIG = 2 * CHUNK + 3                # three chunks on two slots, the last one of three frames
SEAMS = [0, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 2]
EDGES = [1, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1]   # 16: the latency path's largest batch, 17: the first staged one
S_BIT, S_IT, S_CV = 0xA5, -7, 0x5A                      # output sentinels: no decoder writes these
POOL = 128                                              # codewords per code, tiled under fresh noise


class Case:
    def __init__(self, id, code, variant, dtype, kernel, check, schedule="flooding", env=None, iters=50, db=(1.0, 4.0)):
        self.id, self.code, self.variant, self.dtype, self.kernel, self.check = id, code, variant, dtype, kernel, check
        self.schedule, self.env, self.iters, self.db = schedule, env or {}, iters, db


# one case per on-chip rung of select.cc's ladder; `kernel`: what kernel_name must start with after a decode (so that a case
# cannot move to another kernel unnoticed); `check`: the bar against the specification at the seams (part c)
CASES = [
    Case("split-min-jpl4096", "jpl.4096.4.5", "min", "f32", "ldpc::fused_split_kernel<float, ", "f32"),
    Case("split-tanh-jpl1024", "jpl.1024.4.5", "tanh", "f32", "ldpc::fused_split_kernel<float, ", "f32"),
    Case("split-round16-jpl1024", "jpl.1024.4.5", "min", "f16", "ldpc::fused_split_kernel<float, ", "round16"),
    Case("msg-min-jpl1024", "jpl.1024.4.5", "min", "f32", "ldpc::fused_msg_kernel<float, ", "f32", env={"LDPC_FUSED_KERNEL": "msg"}),
    Case("msg-f64-jpl1024", "jpl.1024.4.5", "min", "f64", "ldpc::fused_msg_kernel<double, ", "f64"),
    Case("jit-split-ira", "ira-12x24-sz64", "min", "f32", "ldpc_jit_split_minsum_sz64_", "f32", db=(0.5, 3.5)),
    Case("pk16-jpl1024", "jpl.1024.4.5", "min", "f16pk", "ldpc::fused_pk16_kernel<", "pk16"),
    Case("jit-pk16-ira", "ira-12x24-sz64", "min", "f16pk", "ldpc_jit_pk16_minsum_sz64_", "pk16", db=(0.5, 3.5)),
    Case("layered-jpl1024", "jpl.1024.4.5", "min", "f32", "ldpc::fused_layered_kernel<", "layered", schedule="layered", iters=40),
    Case("layered-pk16-jpl1024", "jpl.1024.4.5", "min", "f16pk", "ldpc::fused_layered_pk16_kernel<", "pk16-layered",
         schedule="layered", iters=40),
    Case("jit-layered-ira", "ira-12x24-sz64", "min", "f32", "ldpc_jit_layered_minsum_sz64_", "layered", schedule="layered",
         iters=40, db=(0.5, 3.5)),
    Case("csr-tanh-1920.303", "1920.1280.3.303", "tanh", "f32", "ldpc::fused_csr_batched_kernel<float, ", "f32", db=(0.5, 3.5)),
    Case("csr-min-1920.A", "1920.1280.A", "min", "f32", "ldpc::fused_csr_batched_kernel<float, ", "f32", db=(0.5, 3.5)),
    Case("csr-moon", "moon.7.13", "min", "f32", "ldpc::fused_csr_kernel<float, ", "f32", iters=20, db=(0.0, 6.0)),
]


def _code(name):
    return load(name) if "." in name else synthetic(name)


def _hip_code(hip, c):
    return c.hip_code(hip) if c.offsets is not None else c.hip_code(hip, prefer_qc=False)


@functools.lru_cache(maxsize=None)
def _codewords(name):
    """POOL random codewords where the code has an encoder, else the all-zero codeword"""
    c = _code(name)
    if getattr(c, "gq", None) is None and getattr(c, "G", None) is None:
        return np.zeros((1, c.N), np.uint8)
    rng = np.random.default_rng(17)
    return np.stack([c.encode(rng.integers(0, 2, c.k).astype(np.uint8)) for _ in range(POOL)])


def frames(name, F, db, seed):
    """[F][N] float32 LLRs (oracle/channel.py's model): codewords drawn from the pool, Eb/N0 uniform in db, fresh noise per frame"""
    c, cw = _code(name), _codewords(name)
    rng = np.random.default_rng(seed)
    s2 = (1.0 / (2.0 * (c.k / c.n_tx) * 10.0 ** (rng.uniform(db[0], db[1], F) / 10.0))).astype(np.float32)
    pick = rng.integers(0, len(cw), F)
    llr = np.zeros((F, c.N), np.float32)
    for f0 in range(0, F, 4096):
        sl = slice(f0, min(F, f0 + 4096))
        y = 2.0 * cw[pick[sl], : c.n_tx].astype(np.float32) - 1.0
        y += np.sqrt(s2[sl])[:, None] * rng.standard_normal(y.shape, dtype=np.float32)
        llr[sl, : c.n_tx] = (2.0 / s2[sl])[:, None] * y
    return llr


def host_decode(hip, dec, llr, iters, packed=False, pinned=False):
    """a host-pointer entry point on buffers that start as sentinels -> (bits or packed bits, iters, converged).  pinned: the LLRs
    and every output in page-locked memory (ldpc_host_alloc), so that every copy of the chunked pipeline is asynchronous"""
    L, F, N = hip.lib(), llr.shape[0], dec.code.N
    assert llr.flags.c_contiguous and llr.dtype in (np.float16, np.float32)
    f16 = llr.dtype == np.float16
    pins = []

    def buf(shape, dtype, fill):
        if not pinned:
            return np.full(shape, fill, dtype)
        pins.append(hip.PinnedArray(shape, dtype))
        pins[-1].array[...] = fill
        return pins[-1].array

    x = buf(llr.shape, llr.dtype, llr) if pinned else llr
    out = buf((F, (N + 7) // 8 if packed else N), np.uint8, S_BIT)
    its = buf((F,), np.int32, S_IT)
    cv = buf((F,), np.uint8, S_CV)
    if packed:
        check(L.ldpc_decode_batch_packed(dec._h, iters, F, x.ctypes.data_as(C.c_void_p), int(f16), ptr(out, C.c_uint8),
                                         ptr(its, C.c_int32), ptr(cv, C.c_uint8)))
    elif f16:
        check(L.ldpc_decode_batch_f16(dec._h, iters, F, x.ctypes.data_as(C.c_void_p), ptr(out, C.c_uint8), ptr(its, C.c_int32),
                                      ptr(cv, C.c_uint8)))
    else:
        check(L.ldpc_decode_batch(dec._h, iters, F, ptr(x, C.c_float), ptr(out, C.c_uint8), ptr(its, C.c_int32), ptr(cv, C.c_uint8)))
    res = tuple(np.array(a) for a in (out, its, cv))   # (copies: the page-locked buffers are freed below)
    for b in pins:
        b.close()
    return res


def device_decode(dec, llr, iters):
    """the same frames in ONE ldpc_decode_batch_dev launch (device buffers, sentinel-filled) -> (bits, iters, converged)"""
    F, N = llr.shape
    x = torch.from_numpy(llr).cuda()
    bits = torch.full((F, N), S_BIT, dtype=torch.uint8, device="cuda")
    its = torch.full((F,), S_IT, dtype=torch.int32, device="cuda")
    cv = torch.full((F,), S_CV, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()   # (the context's stream does not order against torch's)
    dec.decode_batch_dev(x.data_ptr(), bits.data_ptr(), F, iters, its.data_ptr(), cv.data_ptr(), None, llr_f16=llr.dtype == np.float16)
    dec.synchronize()
    return bits.cpu().numpy(), its.cpu().numpy(), cv.cpu().numpy()


def assert_decoded(res, iters, what):
    bits, its, cv = res
    assert bits.max() <= 1, f"{what}: a bit that is not 0 or 1 (an output row nobody wrote)"
    assert its.min() >= 0 and its.max() <= iters and cv.max() <= 1, what


def assert_same(got, want, what):
    for name, g, w in zip(("bits", "iters", "converged"), got, want):
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))
        assert len(bad) == 0, f"{what}: {name} of {len(bad)} frames differ from one launch, first {bad[:8].tolist()}"


def packbits(bits):
    return np.packbits(bits, axis=1, bitorder="little")


@pytest.fixture(scope="module", params=CASES, ids=[k.id for k in CASES])
def case(request, hip):
    """one case's contexts (max_batch 2*8192+3 and 8193), two frame sets, and their one-launch results"""
    k = request.param
    c = _code(k.code)
    with pytest.MonkeyPatch.context() as mp:
        for var, val in k.env.items():
            mp.setenv(var, val)
        code = _hip_code(hip, c)
        big = hip.Decoder(code, k.variant, k.dtype, BIG, path="fused", schedule=k.schedule)
        small = hip.Decoder(code, k.variant, k.dtype, CHUNK + 1, path="fused", schedule=k.schedule)
    sets = [frames(k.code, BIG, k.db, 9100 + s) for s in range(2)]
    ref = [device_decode(big, x, k.iters) for x in sets]
    for r in ref:
        assert_decoded(r, k.iters, "one launch")
        assert 0 < r[2].sum() < BIG, "the frames must hold converged and failed ones"
    assert big.path == small.path == "fused" and big.kernel_name.startswith(k.kernel), big.kernel_name
    if k.id == "csr-min-1920.A":
        assert big.kernel_name.endswith(", 2, false>"), big.kernel_name   # the OSH = 2 instance
    yield k, c, big, small, sets, ref
    big.close()
    small.close()


def test_pipeline_equals_one_launch(hip, case):
    """2*8192+3 frames through the chunked pipeline: identical to one device launch, for f32 and fp16 LLRs and packed results;
    the second frame set finds the first one's results in the slots"""
    k, c, big, small, sets, ref = case
    for s in range(2):
        got = host_decode(hip, big, sets[s], k.iters)
        assert_decoded(got, k.iters, f"{k.id} f32 set {s}")
        assert_same(got, ref[s], f"{k.id} f32 set {s}")
    for s in range(2):
        x16 = sets[s].astype(np.float16)
        want = device_decode(big, x16, k.iters)
        assert_decoded(want, k.iters, f"{k.id} one launch fp16 set {s}")
        got = host_decode(hip, big, x16, k.iters)
        assert_decoded(got, k.iters, f"{k.id} fp16 set {s}")
        assert_same(got, want, f"{k.id} fp16 set {s}")
        # packed results: f32 LLRs for the first set, fp16 for the second
        pk, its, cv = host_decode(hip, big, sets[s] if s == 0 else x16, k.iters, packed=True)
        want = ref[s] if s == 0 else want
        assert_same((pk, its, cv), (packbits(want[0]),) + want[1:], f"{k.id} packed set {s}")


def test_chunk_and_latency_edges(hip, case):
    """a context of 8193 frames (two slots, the last chunk of one frame): batches at the latency path's edge and the chunk's"""
    k, c, big, small, sets, ref = case
    for i, n in enumerate(EDGES):
        s = i % 2   # consecutive calls on different frames
        got = host_decode(hip, small, np.ascontiguousarray(sets[s][:n]), k.iters)
        assert_decoded(got, k.iters, f"{k.id} batch {n}")
        assert_same(got, tuple(r[:n] for r in ref[s]), f"{k.id} batch {n}")
    assert small.kernel_name.startswith(k.kernel), small.kernel_name


def test_seams_against_the_specification(hip, case):
    """the frames next to every chunk seam and 40 others, decoded through the pipeline, against the Double oracle (the fp16
    emulation for packed fp16 arithmetic) with the bars of each family's own tests"""
    k, c, big, small, sets, ref = case
    rng = np.random.default_rng(9200)
    idx = np.array(SEAMS + sorted(rng.choice(np.setdiff1d(np.arange(BIG), SEAMS), 40, replace=False).tolist()))
    x = sets[0]
    if k.check == "f64":
        # the f64 entry point through the per-slot final-LLR buffers: bits, iterations and final LLRs bit-exact
        bits, its, cv, lam = big.decode_batch(x.astype(np.float64), k.iters, want_lam=True)
        for f in idx:
            o = oracle.decode(c.graph, k.variant, k.iters, x[f].astype(np.float64))
            assert its[f] == o["iters"] and bool(cv[f]) == o["converged"], f
            assert np.array_equal(bits[f], o["bits"]) and np.array_equal(lam[f], o["lam"]), f
        assert_same((bits, its, cv), ref[0], f"{k.id} f64 entry point")   # (f32 LLRs widened: the same decode)
        return
    bits, its, cv = host_decode(hip, big, x, k.iters)
    bits, its, cv = bits[idx], its[idx], cv[idx]
    if k.check in ("f32", "round16"):
        xs = x[idx].astype(np.float64) if k.check == "f32" else em.r16(x[idx]).astype(np.float64)
        ob, oi, oc = oracle.decode_batch(c.graph, k.variant, k.iters, xs, nthreads=8)
        assert np.array_equal(bits, ob) and np.array_equal(cv, oc) and iters_agree(its, oi), k.id
    elif k.check == "layered":
        # tests/test_layered_fused_gpu.py's bar (f32 against the Double specification of the serial schedule): flags >= 90 %,
        # bits exact wherever the flags agree, sweeps >= 85 % of those
        lp = np.arange(0, c.M + 1, c.sz)
        ref_l = [oracle.decode_layered(c.graph, lp, k.variant, k.iters, x[f].astype(np.float64)) for f in idx]
        same = cv.astype(bool) == np.array([o["converged"] for o in ref_l])
        assert same.mean() >= 0.90, same.mean()
        assert all(np.array_equal(bits[i], ref_l[i]["bits"]) for i in np.flatnonzero(same)), k.id
        assert (its == np.array([o["iters"] for o in ref_l]))[same].mean() >= 0.85, k.id
    else:
        emulate = em.decode_minsum_pk16 if k.check == "pk16" else em.decode_minsum_pk16_layered
        eb, ei, ec = emulate(c.graph, x[idx], k.iters)[:3]
        assert np.array_equal(bits, eb) and np.array_equal(its, ei) and np.array_equal(cv.astype(bool), ec), k.id


@pytest.mark.parametrize("buffers", ["pageable", "pinned-packed"])
def test_long_chunks_never_decode_at_once(hip, buffers):
    """1920.1280.A min-sum, 200 iterations below the waterfall: each chunk's decode (the persistent CSR kernel, which hands out
    frames through one work counter per context) runs far longer than the next chunk's copy.  3*8192+1 frames, two calls with
    different frames, each identical to one device launch.

    pinned-packed: ldpc_decode_batch_packed has no zero-copy branch, so with page-locked LLRs and outputs it runs the chunked
    pipeline with every copy asynchronous -- chunk k+1's copy ends while chunk k's decode still runs on the other slot stream, and
    only the ordering of the decodes (api.cc decode_chunk) keeps chunk k+1's reset of the counter out of chunk k's launch.
    pageable: a copy into pageable memory returns when it is done, so the host enqueues chunk k+1 only after chunk k's decode has
    ended (measured on MI355X: no two decode kernels overlapped in a kernel trace); this variant checks the byte path's results."""
    c = load("1920.1280.A")
    F, iters = 3 * CHUNK + 1, 200
    dec = hip.Decoder(_hip_code(hip, c), "min", "f32", F, path="fused")
    for s in range(2):
        x = frames(c.name, F, (0.0, 1.0), 9300 + s)
        want = device_decode(dec, x, iters)
        assert dec.kernel_name.startswith("ldpc::fused_csr_batched_kernel<float, ") and dec.kernel_name.endswith(", 2, false>")
        assert (want[1] == iters).mean() > 0.25, "many frames must run to the iteration limit"
        if buffers == "pageable":
            got = host_decode(hip, dec, x, iters)
            assert_decoded(got, iters, f"set {s}")
            assert_same(got, want, f"set {s}")
        else:
            got = host_decode(hip, dec, x, iters, packed=True, pinned=True)
            assert_same(got, (packbits(want[0]),) + want[1:], f"packed, page-locked, set {s}")
    dec.close()


def test_more_than_65535_frames_in_one_call(hip):
    """the frame source and the packed-result kernel with 65 543 frames in one call (grids with one row per frame): frames depend on
    (seed, f) only, and the packed bits are the byte path's bits, LSB first"""
    F, split = 65543, 40000
    ecc = hip.ECC(CODES, "ldpc/hip-minsum/jpl.1024.4.5/50/4/5", max_batch=F)
    N, k = ecc.code.N, ecc.message_length
    one = torch.full((F, N), float("nan"), dtype=torch.float32, device="cuda")
    two = torch.full((F, N), float("nan"), dtype=torch.float32, device="cuda")
    m1 = torch.full((F, k), 7, dtype=torch.uint8, device="cuda")
    m2 = torch.full((F, k), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ecc.sim.generate(77, 0, F, 3.2, one.data_ptr(), m1.data_ptr())
    ecc.sim.generate(77, 0, split, 3.2, two.data_ptr(), m2.data_ptr())
    ecc.sim.generate(77, split, F - split, 3.2, two[split:].data_ptr(), m2[split:].data_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(one).all()) and int(m1.max()) <= 1, "a frame the source did not write"
    assert torch.equal(one, two) and torch.equal(m1, m2)
    assert not torch.equal(one[F - 1], one[F - 1 - split])                       # (the frames do differ)
    bits = torch.full((F, N), S_BIT, dtype=torch.uint8, device="cuda")
    packed = torch.full((F, (N + 7) // 8), S_BIT, dtype=torch.uint8, device="cuda")
    its = torch.full((F,), S_IT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ecc.decoder.decode_batch_dev(one.data_ptr(), bits.data_ptr(), F, 50, its.data_ptr(), None, None)
    ecc.decoder.decode_batch_dev_packed(one.data_ptr(), packed.data_ptr(), F, 50, None, None, None)
    ecc.decoder.synchronize()
    b = bits.cpu().numpy()
    assert b.max() <= 1 and int(its.min()) >= 0
    assert np.array_equal(packed.cpu().numpy(), packbits(b))
    assert (b[:, :k] != m1.cpu().numpy()).any(axis=1).mean() < 0.5                # decoded: mostly the messages sent
    ecc.close()
