"""GPU: the per-context check-node rule (ldpc_ctx_config cn_scale / cn_offset) of the on-chip layered min-sum kernel for any H
(csrc/layered_csr.hip layered_csr_kernel<DCLASS, Ruled<LT>>) against its specification tests/layered_rule_spec.py: bits, sweeps, flags and
final_lam, bit for bit, for the three lam cell types; the default rule unchanged; the input formats; what a rule selects and refuses.

Graphs and the 10-frame input are those of tests/test_layered_i8_gpu.py: eight noisy frames at that test's two Eb/N0 (the lower one is
where, with beta = 0.5 and qscale 4, magnitudes really are cut to zero; at the higher one frames of every code converge, so that the
rule shows in sweeps and final_lam), an all-zero frame and a saturating noiseless codeword."""
import numpy as np
import pytest

from tests import layered_rule_spec as spec
from tests.helpers import CODES
# the graphs ARE those of the int8 test: taken from its module, which is left as it is
from tests.test_layered_i8_gpu import KERNEL, _graph, _heavy, _llr

pytestmark = pytest.mark.gpu

RULES = [(1.0, 0.5), (0.875, 0.0), (0.8125, 0.25)]
# (graph, order, the two Eb/N0 of tests/test_layered_i8_gpu.py CASES)
CASES = [("moon.7.13", "file", (1.0, 3.0)), ("1920.1280.3.303", "helper", (1.5, 2.5)), ("jpl.1024.4.5", "qc", (2.5, 3.5)), ("random", "file", (5.0, 7.0)),
         ("heavy27", "file", (2.0, 5.0))]


def _setup(hip, name, order, dbs):
    G, lp = _graph(name), None
    if order == "helper":
        G, lp = G.permuted(hip)
    return G, lp, _llr(G, dbs)


def _reference(cell, G, llr, max_iters, alpha, beta):
    return spec.decode(cell, G, llr, max_iters, alpha, beta, 4.0)


def _check_exact(dec, cell, G, llr, max_iters, alpha, beta, what):
    """f64 LLRs in, final_lam out, against the specification; -> the specification's result"""
    ref = _reference(cell, G, llr, max_iters, alpha, beta)
    b, i, c, l = dec.decode_batch(llr.astype(np.float64), max_iters, want_lam=True)
    assert np.array_equal(i, ref[1]), (what, i, ref[1])
    assert np.array_equal(c.astype(bool), ref[2]), what
    assert np.array_equal(b, ref[0]), what
    assert np.array_equal(l, np.asarray(ref[3], np.float64)), what
    return ref


@pytest.mark.parametrize("cell", ["f16", "f32", "i8"])
@pytest.mark.parametrize("name,order,dbs", CASES)
def test_bit_exact_against_specification(hip, name, order, dbs, cell):
    G, lp, llr = _setup(hip, name, order, dbs)
    if cell == "f32" and G.N > 40952:            # 4 N bytes of LDS: refused, with or without a rule
        with pytest.raises(hip.LdpcError) as e:
            hip.Decoder(G.code(hip, lp), "min", "f32", len(llr), schedule="layered", cn_scale=1.0, cn_offset=0.5)
        assert e.value.code == -5 and "cn_scale" in str(e.value) and "LDS" in str(e.value)
        return
    base = {mi: _reference(cell, G, llr, mi, 0.75, 0.0) for mi in (1, 25)}
    for alpha, beta in RULES:
        dec = hip.Decoder(G.code(hip, lp), "min", cell, len(llr) + 1, schedule="layered", cn_scale=alpha, cn_offset=beta)
        assert dec.path == "fused" and KERNEL + "<" in dec.kernel_name and "Ruled<" in dec.kernel_name, dec.kernel_name
        assert (dec.cn_scale, dec.cn_offset) == (alpha, beta)          # (exact in sixteenths and quarters: the int8 context reports the same)
        differs = False
        for mi in (0, 1, 25):
            ref = _check_exact(dec, cell, G, llr, mi, alpha, beta, (name, order, cell, alpha, beta, mi))
            if mi:
                differs |= not all(np.array_equal(a, b) for a, b in zip(ref, base[mi]))
        # the specification's own result is not the default rule's: a kernel that ignored the fields would have failed above
        assert differs, (name, cell, alpha, beta)
        dec.close()
    if cell == "i8":   # beta = 0.5 at qscale 4 is b = 2: magnitudes 1 and 2 exist on these frames and are cut to zero
        q = spec.quantize(llr, 4.0)
        assert ((np.abs(q) > 0) & (np.abs(q) <= 2)).any()


@pytest.mark.parametrize("cell", ["f16", "f32", "i8"])
def test_default_unchanged(hip, cell):
    """an explicit (0.75, 0) is the context without the fields: the same kernel, the same arrays"""
    G, lp, llr = _setup(hip, "1920.1280.3.303", "helper", (1.5, 2.5))
    kw = dict(schedule="layered", path="fused")
    plain = hip.Decoder(G.code(hip, lp), "min", cell, len(llr), **kw)
    explicit = hip.Decoder(G.code(hip, lp), "min", cell, len(llr), cn_scale=0.75, cn_offset=0.0, **kw)
    assert plain.kernel_name == explicit.kernel_name and KERNEL + "<" in plain.kernel_name and "Ruled" not in plain.kernel_name
    assert (plain.cn_scale, plain.cn_offset) == (explicit.cn_scale, explicit.cn_offset) == (0.75, 0.0)
    a = plain.decode_batch(llr.astype(np.float64), 25, want_lam=True)
    b = explicit.decode_batch(llr.astype(np.float64), 25, want_lam=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    ref = _reference(cell, G, llr, 25, 0.75, 0.0)
    assert np.array_equal(a[0], ref[0]) and np.array_equal(a[1], ref[1]) and np.array_equal(a[3], np.asarray(ref[3], np.float64))
    # the flooding kernels compute 3/4 min, and say so
    flooding = hip.Decoder(G.code(hip), "min", "f32", 4)
    assert (flooding.cn_scale, flooding.cn_offset) == (0.75, 0.0)
    assert hip.Decoder(G.code(hip), "tanh", "f32", 4).cn_scale == 0.0


def test_input_formats_agree(hip):
    """an int8 context with rule (1, 0.5): f32, fp16, f64 and native int8 LLRs, from host memory and from device memory"""
    import torch
    G = _graph("heavy27")
    l16 = _llr(G, (2.0, 5.0), seed=500).astype(np.float16)
    l32 = l16.astype(np.float32)
    q8 = spec.quantize(l32, 4.0).astype(np.int8)
    dec = hip.Decoder(G.code(hip), "min", "i8", len(l32), schedule="layered", cn_scale=1.0, cn_offset=0.5)
    ref = _check_exact(dec, "i8", G, l32, 25, 1.0, 0.5, "f64")
    assert ref[2].any() and (ref[1] > 0).any()
    dev = torch.device("cuda:0")
    for x, kw in ((l32, {}), (l16, dict(llr_f16=True)), (q8, dict(llr_i8=True))):
        got = dec.decode_batch(x, 25)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2].astype(bool), ref[2]), x.dtype
        dx = torch.from_numpy(x.view(np.int16) if x.dtype == np.float16 else x).to(dev)
        bits = torch.empty(l32.shape, dtype=torch.uint8, device=dev)
        its = torch.empty(len(l32), dtype=torch.int32, device=dev)
        conv = torch.empty(len(l32), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        dec.decode_batch_dev(dx.data_ptr(), bits.data_ptr(), len(l32), 25, its.data_ptr(), conv.data_ptr(), None, **kw)
        dec.synchronize()
        assert np.array_equal(bits.cpu().numpy(), ref[0]) and np.array_equal(its.cpu().numpy(), ref[1]), (x.dtype, "device")
        assert np.array_equal(conv.cpu().numpy().astype(bool), ref[2]), (x.dtype, "device")


def test_selection_and_refusals(hip):
    rule = dict(cn_scale=1.0, cn_offset=0.5)
    for name in ("moon.7.13", "jpl.1024.4.5"):
        G = _graph(name)
        for cell in ("f16", "f32", "i8"):
            for path in ("auto", "fused"):
                d = hip.Decoder(G.code(hip), "min", cell, 8, schedule="layered", path=path, **rule)
                assert d.path == "fused" and KERNEL + "<" in d.kernel_name and "Ruled<" in d.kernel_name, (name, cell, path, d.path, d.kernel_name)
                assert (d.cn_scale, d.cn_offset) == (1.0, 0.5)
    G = _graph("jpl.1024.4.5")
    unsupported = [dict(variant="min", dtype="f32", schedule="flooding"), dict(variant="tanh", dtype="f32", schedule="layered"),
                   dict(variant="tanh-cm", dtype="f64", schedule="flooding", path="flood"), dict(variant="min", dtype="f64", schedule="flooding", sum_order="arraylet", path="flood"),
                   dict(variant="min", dtype="f64", schedule="layered"), dict(variant="min", dtype="f16pk", schedule="layered"),
                   dict(variant="min", dtype="f16", schedule="layered", path="flood"), dict(variant="min", dtype="i8", schedule="layered", path="flood"),
                   dict(variant="min", dtype="i8", schedule="flooding")]
    for kw in unsupported:
        with pytest.raises(hip.LdpcError) as e:
            hip.Decoder(G.code(hip), max_batch=8, **kw, **rule)
        assert e.value.code == -5 and "cn_scale" in str(e.value), (kw, str(e.value))
    with pytest.raises(hip.LdpcError) as e:                     # the kernel's own limits apply: a row record holds 27 sign bits
        hip.Decoder(_heavy(28).code(hip), "min", "f16", 8, schedule="layered", **rule)
    assert e.value.code == -5 and "27" in str(e.value) and "cn_scale" in str(e.value)
    d = hip.Decoder(G.code(hip), "min", "f16", 8, schedule="layered", **rule)
    for call in (lambda: d.decode_trace(np.zeros((2, G.N)), 3), lambda: d.debug_step(np.zeros((1, G.N)), np.zeros((1, G.N)), np.zeros((1, len(G.col_idx))))):
        with pytest.raises(hip.LdpcError) as e:
            call()
        assert e.value.code == -5 and "cn_scale" in str(e.value)
    M = _graph("moon.7.13")
    nan, inf = float("nan"), float("inf")
    invalid = [("f16", dict(cn_scale=nan)), ("f16", dict(cn_scale=inf)), ("f16", dict(cn_scale=-inf)), ("f16", dict(cn_scale=1.25)), ("f16", dict(cn_scale=-0.5)),
               ("f32", dict(cn_offset=nan)), ("f32", dict(cn_offset=inf)), ("f32", dict(cn_offset=-inf)), ("f32", dict(cn_offset=-0.25)),
               ("i8", dict(cn_scale=0.03)), ("i8", dict(cn_scale=1.0, cn_offset=32.0)), ("i8", dict(cn_scale=1.0, cn_offset=0.5, qscale=300.0))]
    for cell, kw in invalid:
        with pytest.raises(hip.LdpcError) as e:
            hip.Decoder(M.code(hip), "min", cell, 8, schedule="layered", **kw)
        assert e.value.code == -1, (cell, kw, str(e.value))
    assert hip.Decoder(M.code(hip), "min", "f16", 8, schedule="layered", cn_scale=0.03).cn_scale == float(np.float32(0.03))     # float cells take it
    d8 = hip.Decoder(M.code(hip), "min", "i8", 8, schedule="layered", cn_scale=0.8, cn_offset=0.3, qscale=3.0)                # 12.8 -> 13; 0.9 -> 1
    assert d8.cn_scale == 13 / 16 and d8.cn_offset == float(np.float32(1.0) / np.float32(3.0))
    # the code-name grammar
    ecc = hip.ECC(CODES, "ldpc/hip-minsum-layered-i8-s1-o0.5/1920.1280.3.303/50/1/3", max_batch=4)
    assert ecc.decoder.path == "fused" and KERNEL + "<" in ecc.decoder.kernel_name and "Ruled<" in ecc.decoder.kernel_name and "signed char" in ecc.decoder.kernel_name
    assert (ecc.decoder.cn_scale, ecc.decoder.cn_offset) == (1.0, 0.5) and ecc.name.startswith("ldpc/hip-minsum-layered-i8-s1-o0.5/")
    ecc = hip.ECC(CODES, "ldpc/hip-minsum-layered-f16-s0.875/1920.1280.3.303/50/1/3", max_batch=4)
    assert (ecc.decoder.cn_scale, ecc.decoder.cn_offset) == (0.875, 0.0) and KERNEL + "<" in ecc.decoder.kernel_name and "Ruled<" in ecc.decoder.kernel_name
    for bad in ("ldpc/hip-minsum-i8-s1-o0.5/1920.1280.3.303/50/1/3", "ldpc/hip-minsum-s1-o0.5/1920.1280.3.303/50/1/3", "ldpc/hip-tanh-layered-s1/1920.1280.3.303/50/1/3",
                "ldpc/hip-minsum-layered-i8-o0.5-s1/1920.1280.3.303/50/1/3", "ldpc/hip-minsum-layered-i8-s1.0.0/1920.1280.3.303/50/1/3"):
        with pytest.raises(hip.LdpcError) as e:
            hip.ECC(CODES, bad, max_batch=4)
        assert e.value.code == -8, bad
    assert hip.lib().ldpc_abi_version() == 3                    # fields and functions were added, no signature changed
