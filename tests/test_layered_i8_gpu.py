"""GPU: the int8 fixed-point layered min-sum decoder (LDPC_I8, csrc/layered_csr.hip layered_csr_kernel<DCLASS, int8_t>) against its
specification tests/layered_i8_spec.py: bits, sweeps, flags and final_lam, bit for bit -- every input format, both prologue paths,
every row-weight class, more frames than resident workgroups -- and what the dtype selects and refuses."""
import functools

import numpy as np
import pytest

from oracle import channel
from tests import layered_i8_spec as spec
from tests.helpers import CODES, load

pytestmark = pytest.mark.gpu

KERNEL = "layered_csr_kernel"


class Graph:
    """a CSR matrix with what the specification and the frames need"""

    def __init__(self, rp, ci, N, k=None, cw=None):
        self.row_ptr, self.col_idx, self.N = np.asarray(rp, np.int32), np.asarray(ci, np.int32), int(N)
        self.M = len(self.row_ptr) - 1
        self.k = k if k is not None else max(self.N - self.M, 1)
        self.cw = np.zeros(self.N, np.uint8) if cw is None else cw      # a codeword (the all-zero one unless the code has an encoder)
        self.qc = None                                                    # (sz, offsets) when the code is handed over quasi-cyclic

    def frames(self, F, db, seed):
        return channel.frames(np.tile(self.cw, (F, 1)), db, self.k, self.N, self.N, seed).astype(np.float32)

    def permuted(self, hip):
        perm, lp = hip.Code.csr_layer_order(self.row_ptr, self.col_idx, self.N, 0)
        prp, pci = hip.Code.permute_rows(self.row_ptr, self.col_idx, perm)
        return Graph(prp, pci, self.N, self.k, self.cw), lp

    def code(self, hip, layer_ptr=None):
        if self.qc is not None:
            return hip.Code.from_qc(*self.qc)                             # layers: the block rows
        c = hip.Code.from_csr(self.row_ptr, self.col_idx, self.N)
        if layer_ptr is not None:
            c.set_layers(layer_ptr)
        return c


def _named(name, qc=False):
    c = load(name)
    cws, _ = c.frames(1, 3.0, seed=9)
    g = Graph(c.graph.row_ptr, c.graph.col_idx, c.N, c.k, cws[0])
    if qc:
        g.qc = (c.sz, c.offsets)
    return g


def _random_irregular(M=300, N=60001, seed=11):
    """the graph of tests/test_layered_csr_gpu.py: rows of weight 2..14; N odd and above 32 767 (element-wise prologue, byte addresses)"""
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(N, int(rng.integers(2, 15)), replace=False)) for _ in range(M)]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return Graph(rp, np.concatenate(rows).astype(np.int32), N, N - M)


def _heavy(weight=27, seed=3):
    """N = 200 (a multiple of 8: the wide prologue): one row of the given weight, forty of weight 2..6"""
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(200, weight, replace=False))] + [np.sort(rng.choice(200, int(rng.integers(2, 7)), replace=False)) for _ in range(40)]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return Graph(rp, np.concatenate(rows).astype(np.int32), 200, 160)


@functools.lru_cache(maxsize=None)
def _graph(name):
    return {"random": _random_irregular, "heavy27": _heavy, "jpl.1024.4.5": lambda: _named("jpl.1024.4.5", qc=True)}.get(name, lambda: _named(name))()


def _llr(G, dbs, seed=100):
    """8 noisy frames at two Eb/N0, an all-zero frame, a noiseless codeword at +-100 (it saturates at any scale >= 1.27)"""
    noisy = np.concatenate([G.frames(4, db, seed + i) for i, db in enumerate(dbs)])
    return np.concatenate([noisy, np.zeros((1, G.N), np.float32), np.where(G.cw, 100.0, -100.0).astype(np.float32)[None]])


def _check_exact(dec, G, llr, max_iters, qscale, what):
    """f64 LLRs in, final_lam out, against the specification; -> the specification's result"""
    ref = spec.decode_minsum_i8_layered(G, spec.quantize(llr, qscale), max_iters, qscale)
    b, i, c, l = dec.decode_batch(llr.astype(np.float64), max_iters, want_lam=True)
    assert np.array_equal(i, ref[1]), (what, i, ref[1])
    assert np.array_equal(c.astype(bool), ref[2]), what
    assert np.array_equal(b, ref[0]), what
    assert np.array_equal(l, ref[3]), what
    return ref


def _same(got, ref, what):
    assert np.array_equal(got[1], ref[1]), (what, got[1], ref[1])
    assert np.array_equal(got[2].astype(bool), ref[2]) and np.array_equal(got[0], ref[0]), what


CASES = [("moon.7.13", "file", (1.0, 3.0)), ("1920.1280.3.303", "file", (1.5, 2.5)), ("1920.1280.3.303", "helper", (1.5, 2.5)),
         ("jpl.1024.4.5", "qc", (2.5, 3.5)), ("random", "file", (5.0, 7.0)), ("heavy27", "file", (2.0, 5.0))]


@pytest.mark.parametrize("name,order,dbs", CASES)
def test_bit_exact_against_specification(hip, name, order, dbs):
    G, lp = _graph(name), None
    if order == "helper":
        G, lp = G.permuted(hip)
    llr = _llr(G, dbs)
    dec = hip.Decoder(G.code(hip, lp), "min", "i8", len(llr) + 1, schedule="layered")
    assert dec.path == "fused" and KERNEL in dec.kernel_name and dec.qscale == 4.0
    for mi in (0, 1, 25):
        ref = _check_exact(dec, G, llr, mi, 4.0, (name, order, mi))
        # native int8 LLRs, with a frame of -128 (taken as -127: every decision 0, a codeword before sweep 1)
        q8 = np.concatenate([spec.quantize(llr, 4.0).astype(np.int8), np.full((1, G.N), -128, np.int8)])
        rq = spec.decode_minsum_i8_layered(G, spec.quantize(q8), mi, 4.0)
        assert all(np.array_equal(a[:-1], b) for a, b in zip(rq[:3], ref[:3])) and rq[2][-1] and rq[1][-1] == 0 and not rq[0][-1].any()
        _same(dec.decode_batch(q8, mi), rq, (name, order, mi, "int8"))


@pytest.mark.parametrize("name", ["heavy27", "random"])      # N = 200: the wide prologue for frames 16-byte aligned; N = 60 001: element-wise
@pytest.mark.parametrize("qscale", [4.0, 3.3])
def test_input_formats_agree(hip, name, qscale):
    """f32, fp16, f64 and native int8 LLRs on ONE context: identical results when the int8 array is quantize(the f32 array).  The LLRs
    are fp16 values, so that all three float formats hold the same numbers; 3.3 is no power of two: the ONE float32 multiply shows"""
    G = _graph(name)
    l16 = _llr(G, (5.0, 6.5) if name == "random" else (2.0, 5.0), seed=500).astype(np.float16)
    l16[0, :8] = [0.4545, 0.7578, 1.364, -0.1515, 2.576, -1.97, 3.182, 0.0]      # products next to x.5 at scale 3.3
    l32 = l16.astype(np.float32)
    q = spec.quantize(l32, qscale)
    dec = hip.Decoder(G.code(hip), "min", "i8", len(l32), schedule="layered", qscale=qscale)
    assert dec.qscale == float(np.float32(qscale))
    ref = _check_exact(dec, G, l32, 25, qscale, (name, qscale, "f64"))
    for x in (l32, l16, q.astype(np.int8)):
        _same(dec.decode_batch(x, 25), ref, (name, qscale, x.dtype))
        p, i, c = dec.decode_batch_packed(x, 25)
        assert np.array_equal(p, np.packbits(ref[0], axis=1, bitorder="little")) and np.array_equal(i, ref[1]), (name, qscale, x.dtype, "packed")
    bits1, it1, cv1 = dec.decode_one(l32[3].astype(np.float64), 25)           # the latency path
    assert np.array_equal(bits1, ref[0][3]) and it1 == ref[1][3] and cv1 == bool(ref[2][3])


def test_many_frames_packed_and_page_locked(hip):
    """more frames than resident workgroups, so that workgroups take further frames from the counter: 600, because a frame of 60 KB
    lets TWO workgroups share each of the 256 CUs (the 300 frames that exceed the fp16 kernel's one per CU would all be resident here);
    packed bits; int8 LLRs in page-locked host memory, bits written to page-locked memory (the kernel reads 1 byte per element over the
    bus)"""
    G, lp = _graph("random").permuted(hip)
    F = 600
    llr = np.concatenate([G.frames(F // 3, 5.0, 200), G.frames(F - F // 3, 6.5, 201)])
    q8 = spec.quantize(llr, 4.0).astype(np.int8)
    dec = hip.Decoder(G.code(hip, lp), "min", "i8", F, schedule="layered")
    ref = spec.decode_minsum_i8_layered(G, q8, 25, 4.0)
    assert 0 < ref[2].sum() < F and (ref[1] > 1).any()              # some frames converge, some run out of sweeps
    _same(dec.decode_batch(llr, 25), ref, "f32")
    _same(dec.decode_batch(q8, 25), ref, "int8")
    p, i, c = dec.decode_batch_packed(q8, 25)
    assert np.array_equal(p, np.packbits(ref[0], axis=1, bitorder="little")) and np.array_equal(i, ref[1]) and np.array_equal(c.astype(bool), ref[2])
    pin_in, pin_out = hip.PinnedArray(q8.shape, np.int8), hip.PinnedArray(q8.shape, np.uint8)
    pin_in.array[:] = q8
    b, i, c = dec.decode_batch(pin_in.array, 25, out_bits=pin_out.array)
    assert b is pin_out.array
    _same((b, i, c), ref, "page-locked int8")


def test_threads_per_workgroup_do_not_change_results(hip, monkeypatch):
    G, lp = _graph("1920.1280.3.303").permuted(hip)
    llr = _llr(G, (1.5, 2.5), seed=700)
    ref = spec.decode_minsum_i8_layered(G, spec.quantize(llr, 4.0), 25, 4.0)
    seen = set()
    for t in (None, "64", "512"):
        if t is None:
            monkeypatch.delenv("LDPC_LAYERED_CSR_THREADS", raising=False)
        else:
            monkeypatch.setenv("LDPC_LAYERED_CSR_THREADS", t)
        dec = hip.Decoder(G.code(hip, lp), "min", "i8", len(llr), schedule="layered")
        seen.add(dec.kernel_geometry[0])
        _same(dec.decode_batch(llr, 25), ref, t)
    assert len(seen) >= 2, seen


def test_selection_and_refusals(hip):
    for name in ("moon.7.13", "1920.1280.3.303", "jpl.1024.4.5"):
        G = _graph(name)
        for path in ("auto", "fused"):
            d = hip.Decoder(G.code(hip), "min", "i8", 8, schedule="layered", path=path)
            assert d.path == "fused" and KERNEL in d.kernel_name and "signed char" in d.kernel_name, (name, path, d.path, d.kernel_name)
            assert d.kernel_geometry[1] == 1 and d.kernel_geometry[0] % 64 == 0
        for kw in (dict(variant="min", schedule="flooding"), dict(variant="tanh", schedule="layered"), dict(variant="min", schedule="layered", path="flood")):
            with pytest.raises(hip.LdpcError) as e:
                hip.Decoder(G.code(hip), dtype="i8", max_batch=8, **kw)
            assert e.value.code == -5 and "LDPC_I8" in str(e.value), kw
    with pytest.raises(hip.LdpcError) as e:                     # a row record holds 27 sign bits
        hip.Decoder(_heavy(28).code(hip), "min", "i8", 8, schedule="layered")
    assert e.value.code == -5 and "27" in str(e.value)
    G = _graph("moon.7.13")
    with pytest.raises(hip.LdpcError) as e:
        hip.Decoder(G.code(hip), "min", "i8", 8, schedule="layered", qscale=-1)
    assert e.value.code == -1
    for bad in (float("inf"), float("nan")):
        with pytest.raises(hip.LdpcError) as e:
            hip.Decoder(G.code(hip), "min", "i8", 8, schedule="layered", qscale=bad)
        assert e.value.code == -1
    d16 = hip.Decoder(G.code(hip), "min", "f16", 8, schedule="layered")
    assert d16.qscale == 0.0
    q8 = np.zeros((4, G.N), np.int8)
    with pytest.raises(hip.LdpcError) as e:                     # int8 LLRs: LDPC_I8 contexts only
        d16.decode_batch(q8, 5)
    assert e.value.code == -5 and "LDPC_I8" in str(e.value)
    with pytest.raises(hip.LdpcError) as e:
        d16.decode_batch_packed(q8, 5)
    assert e.value.code == -5
    d8 = hip.Decoder(G.code(hip), "min", "i8", 8, schedule="layered")
    for call in (lambda: d8.decode_trace(np.zeros((2, G.N)), 3), lambda: d8.debug_step(np.zeros((1, G.N)), np.zeros((1, G.N)), np.zeros((1, len(G.col_idx)))),
                 lambda: _graph("jpl.1024.4.5").code(hip).jit_source("min", "i8", "layered")):
        with pytest.raises(hip.LdpcError) as e:
            call()
        assert e.value.code == -5
    ecc = hip.ECC(CODES, "ldpc/hip-minsum-layered-i8/1920.1280.3.303/50/1/3", max_batch=4)
    assert ecc.decoder.path == "fused" and KERNEL in ecc.decoder.kernel_name and "signed char" in ecc.decoder.kernel_name and ecc.decoder.qscale == 4.0
    assert hip.lib().ldpc_abi_version() == 3
