"""GPU: the on-chip layered min-sum kernel for ANY parity-check matrix with fp16 lam storage (csrc/layered_csr.hip) against its
specification, oracle/emulate_f16.py decode_minsum_f16_layered (rows in ascending order): bits, sweeps, flags and the LLRs a frame
stops with, bit for bit -- in file order and in the order ldpc_csr_layer_order proposes, merged layers or not."""
import numpy as np
import pytest

from oracle import channel
from oracle import emulate_f16 as em
from tests import dvbs2_natural
from tests.helpers import CODES, load

pytestmark = pytest.mark.gpu

KERNEL = "layered_csr_kernel"


class Graph:
    """a CSR matrix with what the emulation and the frames need"""

    def __init__(self, rp, ci, N, k=None):
        self.rp, self.ci, self.N = np.asarray(rp, np.int32), np.asarray(ci, np.int32), int(N)
        self.M = len(self.rp) - 1
        self.k = k if k is not None else max(self.N - self.M, 1)

    def frames(self, F, db, seed):     # the all-zero codeword + noise (a codeword of every linear code)
        return channel.frames(np.zeros((F, self.N), np.uint8), db, self.k, self.N, self.N, seed).astype(np.float32)

    def permuted(self, hip, max_rows=0):
        perm, lp = hip.Code.csr_layer_order(self.rp, self.ci, self.N, max_rows)
        prp, pci = hip.Code.permute_rows(self.rp, self.ci, perm)
        return Graph(prp, pci, self.N, self.k), lp

    def code(self, hip, layer_ptr=None):
        c = hip.Code.from_csr(self.rp, self.ci, self.N)
        if layer_ptr is not None:
            c.set_layers(layer_ptr)
        return c


def _emu_graph(G):
    class _G:
        pass
    g = _G()
    g.M, g.N, g.E = G.M, G.N, len(G.ci)
    g.row_ptr, g.col_idx = G.rp.astype(np.int64), G.ci.astype(np.int64)
    return g


def _named(name):
    c = load(name)
    return Graph(c.graph.row_ptr, c.graph.col_idx, c.N, c.k)


def _random_irregular(M=300, N=60001, seed=11):
    """rows of weight 2..14, mixed inside every layer; N not a multiple of 8, a frame of 120 KB: one workgroup per CU"""
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(N, int(rng.integers(2, 15)), replace=False)) for _ in range(M)]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return Graph(rp, np.concatenate(rows).astype(np.int32), N, N - M)


def _check_exact(dec, G, llr, max_iters, what):
    bits, its, conv, lam = em.decode_minsum_f16_layered(_emu_graph(G), llr, max_iters)
    b, i, c, l = dec.decode_batch(llr.astype(np.float64), max_iters, want_lam=True)
    assert np.array_equal(i, its), (what, i, its)
    assert np.array_equal(c.astype(bool), conv), what
    assert np.array_equal(b, bits), what
    assert np.array_equal(l, lam.astype(np.float64)), what
    return bits, its, conv


def test_selection(hip):
    for name in ("moon.7.13", "1920.1280.3.303", "1920.1280.A"):
        G = _named(name)
        for path in ("auto", "fused"):
            d = hip.Decoder(G.code(hip), "min", "f16", 8, schedule="layered", path=path)
            assert d.path == "fused" and KERNEL in d.kernel_name, (name, path, d.path, d.kernel_name)
            assert d.kernel_geometry[1] == 1 and d.kernel_geometry[0] % 64 == 0
        d32 = hip.Decoder(G.code(hip), "min", "f32", 8, schedule="layered")
        assert d32.path == "flood" and KERNEL not in d32.kernel_name
        with pytest.raises(hip.LdpcError) as e:
            hip.Decoder(G.code(hip), "tanh", "f16", 8, schedule="layered")
        assert e.value.code == -5
        with pytest.raises(hip.LdpcError) as e:                 # an explicit HBM path stays refused
            hip.Decoder(G.code(hip), "min", "f16", 8, schedule="layered", path="flood")
        assert e.value.code == -5
    rng = np.random.default_rng(3)
    heavy = [np.sort(rng.choice(200, 28, replace=False))] + [np.sort(rng.choice(200, 4, replace=False)) for _ in range(40)]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in heavy])])
    with pytest.raises(hip.LdpcError) as e:                     # a row record holds 27 sign bits
        hip.Decoder(Graph(rp, np.concatenate(heavy), 200).code(hip), "min", "f16", 8, schedule="layered")
    assert e.value.code == -5 and "27" in str(e.value)
    big = Graph(np.arange(0, 3 * 40 + 1, 3), np.concatenate([np.sort(rng.choice(90000, 3, replace=False)) for _ in range(40)]), 90000)
    with pytest.raises(hip.LdpcError) as e:                     # 180 KB of fp16 LLRs
        hip.Decoder(big.code(hip), "min", "f16", 8, schedule="layered")
    assert e.value.code == -5 and "LDS" in str(e.value)
    ecc = hip.ECC(CODES, "ldpc/hip-minsum-layered-f16/1920.1280.3.303/50/1/3", max_batch=4)   # record names: file order
    assert ecc.decoder.path == "fused" and KERNEL in ecc.decoder.kernel_name


@pytest.mark.parametrize("name,dbs", [("moon.7.13", (1.0, 3.0)), ("1920.1280.3.303", (1.5, 2.5)), ("1920.1280.A", (2.0, 3.0)), ("random", (2.0, 4.0))])
@pytest.mark.parametrize("order", ["file", "helper"])
def test_bit_exact_against_emulation(hip, name, dbs, order):
    G = _random_irregular() if name == "random" else _named(name)
    lp = None
    if order == "helper":
        G, lp = G.permuted(hip)
    F = 8
    llr = np.concatenate([G.frames(F // 2, db, 100 + i) for i, db in enumerate(dbs)])
    llr[0] = 0.0                                                           # all-zero LLRs: the syndrome is zero before sweep 1
    llr[1] = -6.0                                                          # the noiseless all-zero codeword
    dec = hip.Decoder(G.code(hip, lp), "min", "f16", F, schedule="layered")
    assert KERNEL in dec.kernel_name
    for mi in (0, 1, 25):
        _check_exact(dec, G, llr, mi, (name, order, mi))


def test_inputs_outputs_and_many_frames(hip):
    """more frames than resident workgroups (one per CU at 120 KB of LDS), N not a multiple of 8; f32, f16 and f64 LLRs, packed
    bits, LLRs in page-locked host memory"""
    G, lp = _random_irregular().permuted(hip)
    F = 300
    llr = np.concatenate([G.frames(F // 2, 2.0, 200), G.frames(F - F // 2, 3.5, 201)])
    dec = hip.Decoder(G.code(hip, lp), "min", "f16", F, schedule="layered")
    bits, its, conv = _check_exact(dec, G, llr, 25, "f64")
    for x in (llr, llr.astype(np.float16)):
        b, i, c = dec.decode_batch(x, 25)
        ref = em.decode_minsum_f16_layered(_emu_graph(G), x.astype(np.float32), 25) if x.dtype == np.float16 else (bits, its, conv)
        assert np.array_equal(b, ref[0]) and np.array_equal(i, ref[1]) and np.array_equal(c.astype(bool), ref[2]), x.dtype
    p, i, c = dec.decode_batch_packed(llr, 25)
    assert np.array_equal(p, np.packbits(bits, axis=1, bitorder="little")) and np.array_equal(i, its)
    pin_in, pin_out = hip.PinnedArray(llr.shape, np.float32), hip.PinnedArray(llr.shape, np.uint8)
    pin_in.array[:] = llr
    b, i, c = dec.decode_batch(pin_in.array, 25, out_bits=pin_out.array)
    assert np.array_equal(b, bits) and np.array_equal(i, its) and np.array_equal(c.astype(bool), conv)


def test_merging_is_result_neutral(hip):
    G, lp = _named("1920.1280.A").permuted(hip)
    llr = np.concatenate([G.frames(6, 2.0, 300), G.frames(6, 3.0, 301)])
    one = hip.Decoder(G.code(hip), "min", "f16", 12, schedule="layered")          # one row per layer: merged into the same steps
    lay = hip.Decoder(G.code(hip, lp), "min", "f16", 12, schedule="layered")
    a, b = one.decode_batch(llr.astype(np.float64), 30, want_lam=True), lay.decode_batch(llr.astype(np.float64), 30, want_lam=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    capped, lpc = _named("1920.1280.A").permuted(hip, max_rows=64)                  # smaller layers, another order: still the emulation
    _check_exact(hip.Decoder(capped.code(hip, lpc), "min", "f16", 12, schedule="layered"), capped, llr, 30, "max_rows=64")


def test_dvbs2_structured_natural_order(hip):
    rp, ci = dvbs2_natural.csr()
    N, M, Q = dvbs2_natural.N, dvbs2_natural.M, dvbs2_natural.Q
    # the quasi-cyclic route cannot take it: blocks with two circulants (ldpc_code_create_qc holds one rotation per block), and
    # such a block row is no column-disjoint layer
    doubles = {k: v for k, v in dvbs2_natural.qc_blocks().items() if len(v) > 1}
    assert len({g for _, g in doubles}) >= 3
    for (r, g) in list(doubles)[:3]:
        rows = r + Q * np.arange(M // Q)
        cols = np.concatenate([ci[rp[m]:rp[m + 1]] for m in rows])
        assert len(np.unique(cols)) < len(cols), (r, g)
    assert np.array_equal(ci[rp[0]:rp[1]][-1:], [dvbs2_natural.K])             # check 0 sees parity bit 0 only: no wrap
    G, lp = Graph(rp, ci, N, dvbs2_natural.K).permuted(hip)
    llr = np.concatenate([G.frames(2, db, 400 + i) for i, db in enumerate((1.0, 1.5, 2.0))])
    dec = hip.Decoder(G.code(hip, lp), "min", "f16", len(llr), schedule="layered")
    assert dec.path == "fused" and KERNEL in dec.kernel_name
    bits, its, conv = _check_exact(dec, G, llr, 20, "dvbs2")
    flood = hip.Decoder(G.code(hip, lp), "min", "f32", len(llr), schedule="layered", path="flood")
    fb, fi, fc = flood.decode_batch(llr, 20)
    both = conv & fc.astype(bool)
    assert both.sum() >= 2 and np.array_equal(bits[both], fb[both])
