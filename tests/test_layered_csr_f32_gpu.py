"""GPU: the f32-lam instances of the on-chip layered min-sum kernel for ANY parity-check matrix (csrc/layered_csr.hip,
layered_csr_kernel<DCLASS, float>): selection, then bits, sweeps, flags and the LLRs a frame stops with, bit for bit, against
  * the project's own HBM kernel (flood.hip layered_kernel<float, min-sum>, path="flood") on the same code and layers,
  * an independent specification (tests/layered_f32_spec.py: oracle/emulate_f16.py decode_minsum_f16_layered with a float32 cast in
    place of its fp16 rounding, and the non-finite veto on top),
  * the Double oracle where float and Double agree (flags, sweeps, bits),
in file order and in the order ldpc_csr_layer_order proposes, merged layers or not."""
import numpy as np
import pytest

from oracle import oracle
from tests import dvbs2_short
from tests import layered_f32_spec as spec
from tests.helpers import load
from tests.layered_f32_spec import Graph

pytestmark = pytest.mark.gpu

KERNEL = "layered_csr_kernel"
NAMED = ("moon.7.13", "1920.1280.3.303", "1920.1280.A")


def _f32(hip, code, F, **kw):
    dec = hip.Decoder(code, "min", "f32", F, schedule="layered", path="fused", **kw)
    assert dec.path == "fused" and KERNEL in dec.kernel_name and "float" in dec.kernel_name, (dec.path, dec.kernel_name)
    return dec


def _same(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x), np.asarray(y)
        if x.dtype == bool or y.dtype == bool:
            x, y = x.astype(bool), y.astype(bool)
        assert np.array_equal(x, y), (what, "output %d of %d" % (k, len(a)))


def _check_emulation(monkeypatch, dec, G, llr, max_iters, what):
    bits, its, conv, lam, vetoed = spec.emulate(monkeypatch, G, llr, max_iters)
    got = dec.decode_batch(llr.astype(np.float64), max_iters, want_lam=True)
    _same(got, (bits, its, conv, lam.astype(np.float64)), what)
    return bits, its, conv, vetoed


def test_selection(hip, monkeypatch):
    for name in NAMED:
        G = spec._named(name)
        w = int(np.diff(G.rp).max())
        dclass = 8 if w <= 8 else 20 if w <= 20 else 32         # the instance the heaviest row picks
        d = hip.Decoder(G.code(hip), "min", "f32", 8, schedule="layered", path="fused")
        assert d.path == "fused" and KERNEL in d.kernel_name and "float" in d.kernel_name, (name, d.path, d.kernel_name)
        assert d.kernel_geometry[1] == 1 and d.kernel_geometry[0] % 64 == 0
        auto = hip.Decoder(G.code(hip), "min", "f32", 8, schedule="layered")             # LDPC_PATH_AUTO is not re-routed
        assert auto.path == "flood" and KERNEL not in auto.kernel_name, (name, auto.path, auto.kernel_name)
        for path in ("auto", "fused"):                                                   # the fp16 instances keep their names
            d16 = hip.Decoder(G.code(hip), "min", "f16", 8, schedule="layered", path=path)
            assert d16.path == "fused" and d16.kernel_name == f"ldpc::layered_csr_kernel<{dclass}>", (name, path, d16.kernel_name)
        assert d.kernel_name == f"ldpc::layered_csr_kernel<{dclass}, float>", d.kernel_name
        with pytest.raises(hip.LdpcError) as e:
            hip.Decoder(G.code(hip), "tanh", "f32", 8, schedule="layered", path="fused")
        assert e.value.code == -5
    rng = np.random.default_rng(3)
    heavy = [np.sort(rng.choice(200, 28, replace=False))] + [np.sort(rng.choice(200, 4, replace=False)) for _ in range(40)]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in heavy])])
    with pytest.raises(hip.LdpcError) as e:                     # a row record holds 27 sign bits
        hip.Decoder(Graph(rp, np.concatenate(heavy), 200).code(hip), "min", "f32", 8, schedule="layered", path="fused")
    assert e.value.code == -5 and "27" in str(e.value)
    big = Graph(np.arange(0, 3 * 40 + 1, 3), np.concatenate([np.sort(rng.choice(41000, 3, replace=False)) for _ in range(40)]), 41000)
    with pytest.raises(hip.LdpcError) as e:                     # 164 000 B of f32 LLRs
        hip.Decoder(big.code(hip), "min", "f32", 8, schedule="layered", path="fused")
    assert e.value.code == -5 and "LDS" in str(e.value)
    j = load("jpl.1024.4.5")                                    # a QC code keeps its on-chip QC kernel
    dq = hip.Decoder(j.hip_code(hip), "min", "f32", 8, schedule="layered", path="fused")
    assert dq.path == "fused" and "fused_layered" in dq.kernel_name and KERNEL not in dq.kernel_name, dq.kernel_name
    monkeypatch.setenv("LDPC_LAYERED_CSR", "0")                 # the switch takes both instances
    G = spec._named("1920.1280.3.303")
    with pytest.raises(hip.LdpcError) as e:
        hip.Decoder(G.code(hip), "min", "f32", 8, schedule="layered", path="fused")
    assert e.value.code == -5
    with pytest.raises(hip.LdpcError) as e:
        hip.Decoder(G.code(hip), "min", "f16", 8, schedule="layered")
    assert e.value.code == -5


CASES = [("moon.7.13", (1.0, 3.0)), ("1920.1280.3.303", (1.5, 2.5)), ("1920.1280.A", (2.0, 3.0)), ("random", (2.0, 4.0))]


def _case(hip, name, order):
    G = spec.random_irregular() if name == "random" else spec._named(name)
    lp = None
    if order == "helper":
        G, lp = G.permuted(hip)
    return G, lp


@pytest.mark.parametrize("name,dbs", CASES)
@pytest.mark.parametrize("order", ["file", "helper"])
def test_bit_exact_against_flood(hip, name, dbs, order):
    """flood.hip layered_kernel<float, min-sum>: the same code object layout and layers, state in HBM"""
    G, lp = _case(hip, name, order)
    llr = spec.exact_inputs(G, dbs)
    dec = _f32(hip, G.code(hip, lp), len(llr))
    ref = hip.Decoder(G.code(hip, lp), "min", "f32", len(llr), schedule="layered", path="flood")
    assert ref.path == "flood" and KERNEL not in ref.kernel_name
    for mi in (0, 1, 25):
        _same(dec.decode_batch(llr.astype(np.float64), mi, want_lam=True), ref.decode_batch(llr.astype(np.float64), mi, want_lam=True),
              (name, order, mi))


@pytest.mark.parametrize("name,dbs", CASES)
@pytest.mark.parametrize("order", ["file", "helper"])
def test_bit_exact_against_emulation(hip, monkeypatch, name, dbs, order):
    G, lp = _case(hip, name, order)
    llr = spec.exact_inputs(G, dbs)
    dec = _f32(hip, G.code(hip, lp), len(llr))
    taken = False
    for mi in (0, 1, 25):
        vetoed = _check_emulation(monkeypatch, dec, G, llr, mi, (name, order, mi))[3]
        taken |= bool(vetoed.any())
    if name == "1920.1280.A":
        assert taken, "no frame of the 1920.1280.A input took the non-finite veto"
    if name in ("moon.7.13", "1920.1280.3.303"):
        assert not taken, name


@pytest.mark.parametrize("name,dbs", spec.ORACLE_CASES)
def test_against_the_double_oracle(hip, name, dbs):
    """one row per layer, 25 sweeps: flags, sweep counts and bits of all 16 frames per code (largest |LLR| 27.5 and 30.5: float and
    Double take the same decisions on these inputs -- tests/test_layered_f32_emulation.py)"""
    G = spec._named(name)
    llr = spec.oracle_inputs(G, dbs)
    dec = _f32(hip, G.code(hip), len(llr))
    b, i, c = dec.decode_batch(llr.astype(np.float64), spec.ORACLE_SWEEPS)
    ob, oi, oc = oracle.decode_layered_batch(oracle.Graph(G.rp, G.ci, G.N), np.arange(G.M + 1, dtype=np.int32), "min", spec.ORACLE_SWEEPS,
                                             llr.astype(np.float64))
    assert np.array_equal(c.astype(bool), oc.astype(bool)), name
    assert np.array_equal(i, oi), (name, i, oi)
    assert np.array_equal(b, ob), name


def test_inputs_outputs_and_many_frames(hip, monkeypatch):
    """more frames than resident workgroups (one per CU at 160 KB of LDS), N not a multiple of 8; f64, f32 and f16 LLRs, packed
    bits, LLRs in page-locked host memory"""
    G, lp = spec.random_irregular().permuted(hip)
    F = 300
    llr = np.concatenate([G.frames(F // 2, 2.0, 200), G.frames(F - F // 2, 3.5, 201)])
    dec = _f32(hip, G.code(hip, lp), F)
    bits, its, conv, _ = _check_emulation(monkeypatch, dec, G, llr, 25, "f64")
    for x in (llr, llr.astype(np.float16)):
        b, i, c = dec.decode_batch(x, 25)
        ref = spec.emulate(monkeypatch, G, x.astype(np.float32), 25)[:3] if x.dtype == np.float16 else (bits, its, conv)
        _same((b, i, c), ref, str(x.dtype))
    p, i, c = dec.decode_batch_packed(llr, 25)
    assert np.array_equal(p, np.packbits(bits, axis=1, bitorder="little")) and np.array_equal(i, its) and np.array_equal(c.astype(bool), conv)
    pin_in, pin_out = hip.PinnedArray(llr.shape, np.float32), hip.PinnedArray(llr.shape, np.uint8)
    pin_in.array[:] = llr
    b, i, c = dec.decode_batch(pin_in.array, 25, out_bits=pin_out.array)
    _same((b, i, c), (bits, its, conv), "page-locked")
    assert np.array_equal(pin_out.array, bits)


def _wide_case(hip, name):
    """-> G, layer_ptr, f32 LLRs, sweeps.  N % 8 == 0 and 16-byte aligned frames: f32 / f16 LLRs without the LLR output take the kernel's
    wide path (eight cells per lane and request, two 16-byte LDS stores, eight bits per store)"""
    if name == "dvbs2-short":                                   # T = 1024, N = 16 200; frames 0 and 1 run out of sweeps
        rp, ci = dvbs2_short.csr()
        G, lp = Graph(rp, ci, dvbs2_short.N, dvbs2_short.K).permuted(hip)
        return G, lp, np.concatenate([G.frames(2, db, 400 + i) for i, db in enumerate((1.0, 1.5, 2.0))]), 20
    G = spec._named(name)                                       # file order; some frames take the veto
    return G, None, spec.exact_inputs(G, (2.0, 3.0)), 25


@pytest.mark.parametrize("name", ["1920.1280.A", "dvbs2-short"])
def test_wide_path(hip, monkeypatch, name):
    """f32 and f16 host arrays, packed bits and page-locked arrays, none with the LLR output, on codes with N % 8 == 0: against the
    emulation with the veto and against path="flood"; a vetoed frame and a frame out of sweeps reload the channel's decisions wide"""
    G, lp, llr, mi = _wide_case(hip, name)
    assert G.N % 8 == 0 and llr.dtype == np.float32
    dec = _f32(hip, G.code(hip, lp), len(llr))
    flood = hip.Decoder(G.code(hip, lp), "min", "f32", len(llr), schedule="layered", path="flood")
    assert flood.path == "flood"
    for x in (llr, llr.astype(np.float16)):
        bits, its, conv, _, vetoed = spec.emulate(monkeypatch, G, x.astype(np.float32), mi)
        if name == "1920.1280.A":
            assert vetoed.any(), "no frame of the 1920.1280.A input took the non-finite veto"
        assert (~conv).any() and conv.any()
        got = dec.decode_batch(x, mi)
        _same(got, (bits, its, conv), (name, str(x.dtype), "emulation"))
        _same(got, flood.decode_batch(x, mi), (name, str(x.dtype), "flood"))
        p, i, c = dec.decode_batch_packed(x, mi)
        assert np.array_equal(p, np.packbits(bits, axis=1, bitorder="little")), (name, str(x.dtype), "packed bits")
        _same((i, c), (its, conv), (name, str(x.dtype), "packed"))
    bits, its, conv, _, _ = spec.emulate(monkeypatch, G, llr, mi)
    pin_in, pin_out = hip.PinnedArray(llr.shape, np.float32), hip.PinnedArray(llr.shape, np.uint8)
    pin_in.array[:] = llr
    b, i, c = dec.decode_batch(pin_in.array, mi, out_bits=pin_out.array)
    _same((b, i, c), (bits, its, conv), (name, "page-locked"))
    assert np.array_equal(pin_out.array, bits)


def test_merging_is_result_neutral(hip, monkeypatch):
    base = spec._named("1920.1280.A")
    G, lp = base.permuted(hip)
    llr = np.concatenate([G.frames(6, 2.0, 300), G.frames(6, 3.0, 301)])
    one = _f32(hip, G.code(hip), 12)                  # one row per layer: merged into the same steps
    lay = _f32(hip, G.code(hip, lp), 12)
    _check_emulation(monkeypatch, one, G, llr, 30, "one row per layer")
    _check_emulation(monkeypatch, lay, G, llr, 30, "helper layers")
    capped, lpc = base.permuted(hip, max_rows=64)     # smaller layers, another order: still the emulation
    _check_emulation(monkeypatch, _f32(hip, capped.code(hip, lpc), 12), capped, llr, 30, "max_rows=64")


def test_dvbs2_short_structure(hip, monkeypatch):
    rp, ci = dvbs2_short.csr()
    N, M, Q = dvbs2_short.N, dvbs2_short.M, dvbs2_short.Q
    assert (N, dvbs2_short.K, M, Q, dvbs2_short.PERIOD) == (16200, 7200, 9000, 25, 360) and len(rp) == M + 1
    assert sum(dvbs2_short.GROUP_WEIGHTS) == 100 and all(np.bincount(np.concatenate(dvbs2_short.address_tables()) % Q, minlength=Q) == 4)
    # the quasi-cyclic route cannot take it: blocks with two circulants (ldpc_code_create_qc holds one rotation per block), and
    # such a block row is no column-disjoint layer
    doubles = {k: v for k, v in dvbs2_short.qc_blocks().items() if len(v) > 1}
    assert len({g for _, g in doubles}) >= 3
    for (r, g) in list(doubles)[:3]:
        rows = r + Q * np.arange(M // Q)
        cols = np.concatenate([ci[rp[m]:rp[m + 1]] for m in rows])
        assert len(np.unique(cols)) < len(cols), (r, g)
    assert np.array_equal(ci[rp[0]:rp[1]][-1:], [dvbs2_short.K])               # check 0 sees parity bit 0 only: no wrap
    assert np.sum(ci[rp[0]:rp[1]] >= dvbs2_short.K) == 1
    G, lp = Graph(rp, ci, N, dvbs2_short.K).permuted(hip)
    llr = np.concatenate([G.frames(2, db, 400 + i) for i, db in enumerate((1.0, 1.5, 2.0))])
    dec = _f32(hip, G.code(hip, lp), len(llr))
    _check_emulation(monkeypatch, dec, G, llr, 20, "dvbs2-short")
    flood = hip.Decoder(G.code(hip, lp), "min", "f32", len(llr), schedule="layered", path="flood")
    assert flood.path == "flood"
    _same(dec.decode_batch(llr.astype(np.float64), 20, want_lam=True), flood.decode_batch(llr.astype(np.float64), 20, want_lam=True), "dvbs2-short/flood")
