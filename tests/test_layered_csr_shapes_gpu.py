"""GPU: all eighteen instances of the on-chip layered min-sum kernel for any H (csrc/layered_csr.hip layered_csr_kernel<8|20|32, cell> and
<..., Ruled<cell>>, cell fp16, f32, int8) on the synthetic matrices of tests/layered_shapes.py -- every row weight 2..27, waves of heavy rows
only, many steps of mixed weights, steps of several slabs, a last slab with an idle wave, declared layers that merge into one step, rows
without edges -- against ONE reference, tests/layered_rule_spec.py decode (at (3/4, 0) the plain kernels' specification), bit for bit:
np.array_equal everywhere, no tolerance.  The reference depends on the row order only, so the layer and thread variants share it.

The frames are the ten of tests/test_layered_i8_gpu.py _llr: four noisy ones at each of two Eb/N0 (seeds 100 and 101), an all-zero frame, the
noiseless codeword.  What every (case, cell) has to give ON THE REFERENCE: among the eight noisy frames one that converges after more than
one sweep and one that runs out of the 25 sweeps (a frame out of sweeps returns the channel's decisions: alone it would show nothing of the
arithmetic).  Eb/N0: "w20" (5, 7) and "w27" (3, 5); "w8" (2.5, 5) -- at (3, 5) all eight noisy frames of the fp16 and f32 cells converge.
The int8 cell with the rule (1, 0.5) converges on no noisy frame of "w8" at any Eb/N0 or seed tried (1.5 .. 8 dB; at scale 1 its message
magnitudes grow to the cap): that instance is decoded with the rule (1/2, 0) as well, which meets the condition."""
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import layered_rule_spec as spec
from tests import layered_shapes as S
from tests.test_layered_i8_gpu import _llr

pytestmark = pytest.mark.gpu

NAMES = list(S.CASES)
CELLS = ["f16", "f32", "i8"]
DBS = {"w8": (2.5, 5.0), "w20": (5.0, 7.0), "w27": (3.0, 5.0)}
PLAIN, RULED = (0.75, 0.0), (1.0, 0.5)
ALSO = {("w8", "i8"): (0.5, 0.0)}          # a second rule where (1, 0.5) converges on no noisy frame
SWEEPS = 25
ENV = "LDPC_LAYERED_CSR_THREADS"


@functools.lru_cache(maxsize=None)
def _frames(name):
    llr = _llr(S.case(name), DBS[name])
    llr.setflags(write=False)
    return llr


def _frozen(ref):
    out = (ref[0], ref[1], np.asarray(ref[2], bool), np.asarray(ref[3], np.float64))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref(name, cell, alpha, beta, max_iters):
    """bits, sweeps, converged, final_lam (float64) of the ten frames; shared, never written"""
    return _frozen(spec.decode(cell, S.case(name), _frames(name), max_iters, alpha, beta, 4.0))


def _exercised(ref):
    """the condition on the reference: of the eight noisy frames one converges after more than one sweep, one runs out"""
    sweeps, conv = ref[1][:8], ref[2][:8]
    return bool((conv & (sweeps > 1)).any() and (~conv).any())


def _kernel_name(name, cell, ruled):
    t = {"f16": "_Float16", "f32": "float", "i8": "signed char"}[cell]
    if ruled:
        return f"ldpc::layered_csr_kernel<{S.DCLASS[name]}, ldpc::Ruled<{t}>>"
    return f"ldpc::layered_csr_kernel<{S.DCLASS[name]}>" if cell == "f16" else f"ldpc::layered_csr_kernel<{S.DCLASS[name]}, {t}>"


def _decoder(hip, g, layer_ptr, cell, rule, F):
    kw = {} if rule == PLAIN else dict(cn_scale=rule[0], cn_offset=rule[1])
    path = "fused" if cell == "f32" and rule == PLAIN else "auto"          # (auto keeps a plain f32 context on flood.hip)
    dec = hip.Decoder(g.code(hip, layer_ptr), "min", cell, F, schedule="layered", path=path, **kw)
    assert dec.path == "fused"
    return dec


def _same(got, ref, what, n=4):
    assert np.array_equal(got[1], ref[1]), (what, "sweeps", got[1], ref[1])
    assert np.array_equal(np.asarray(got[2], bool), ref[2]), (what, "flags")
    assert np.array_equal(got[0], ref[0]), (what, "bits")
    if n == 4:
        assert np.array_equal(got[3], ref[3]), (what, "final_lam")


def test_the_parametrisations_name_eighteen_instances():
    names = {_kernel_name(n, c, r) for n in NAMES for c in CELLS for r in (False, True)}
    assert len(names) == 18 and all(k.startswith("ldpc::layered_csr_kernel<") for k in names)


@pytest.mark.parametrize("rule", [PLAIN, RULED], ids=["plain", "ruled"])
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", NAMES)
def test_every_instance_bit_exact(hip, monkeypatch, name, cell, rule):
    monkeypatch.delenv(ENV, raising=False)
    g, llr = S.case(name), _frames(name)
    for r in [rule] + ([ALSO[name, cell]] if rule == RULED and (name, cell) in ALSO else []):
        what = (name, cell, r)
        ref = _ref(name, cell, r[0], r[1], SWEEPS)
        if r == RULED and (name, cell) in ALSO:
            assert not ref[2][:8].any(), what                  # (what the module's docstring says of it)
        else:
            assert _exercised(ref), (what, ref[1], ref[2])
        dec = _decoder(hip, g, g.layer_ptr, cell, r, len(llr))
        assert dec.kernel_name == _kernel_name(name, cell, r != PLAIN), dec.kernel_name
        assert dec.kernel_geometry == (S.default_threads(g, g.layer_ptr), 1) and dec.kernel_geometry[0] == {"w8": 256, "w20": 256, "w27": 192}[name]
        for mi in (0, 1, SWEEPS):
            _same(dec.decode_batch(llr.astype(np.float64), mi, want_lam=True), _ref(name, cell, r[0], r[1], mi), what + (mi,))
        # f32 LLRs, no LLR output: the 8-wide prologue and epilogue ("w8", "w27": N a multiple of 8), the element-wise one ("w20")
        assert (g.N % 8 == 0) == (name != "w20")
        _same(dec.decode_batch(llr, SWEEPS), ref, what + ("f32",), n=3)
        p, i, c = dec.decode_batch_packed(llr, SWEEPS)
        assert np.array_equal(p, np.packbits(ref[0], axis=1, bitorder="little")), what + ("packed",)
        assert np.array_equal(i, ref[1]) and np.array_equal(c.astype(bool), ref[2]), what + ("packed",)
        dec.close()


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", NAMES)
def test_layers_and_threads_do_not_change_results(hip, monkeypatch, name, cell):
    g, llr = S.case(name), _frames(name)
    ref = _ref(name, cell, PLAIN[0], PLAIN[1], SWEEPS)
    declared, own = g.layer_ptr, np.arange(g.M + 1)
    steps = S.steps_of(g, declared)
    # what each variant is there for
    assert max(int(np.sum((declared[:-1] >= s[0]) & (declared[:-1] <= s[-1]))) for s in steps) >= 2          # declared: layers that merge
    assert [int(s[0]) for s in S.steps_of(g, own)] != [int(s[0]) for s in steps]                              # own: other step boundaries
    assert sum(S.slabs(s, 64)[0] > 1 for s in steps) >= 5                                                      # 64: steps of several slabs
    assert any(S.slabs(s, 128)[1] <= 64 for s in steps if len(s) > 1)                                         # 128: an idle second wave
    seen = set()
    for what, lp, force, threads in (("declared", declared, None, S.default_threads(g, declared)), ("own", None, None, S.default_threads(g, own)),
                                     ("64", declared, "64", 64), ("128", declared, "128", 128)):
        if force is None:
            monkeypatch.delenv(ENV, raising=False)
        else:
            monkeypatch.setenv(ENV, force)
        dec = _decoder(hip, g, lp, cell, PLAIN, len(llr))
        assert dec.kernel_name == _kernel_name(name, cell, False) and dec.kernel_geometry == (threads, 1), (what, dec.kernel_name, dec.kernel_geometry)
        seen.add(dec.kernel_geometry[0])
        _same(dec.decode_batch(llr.astype(np.float64), SWEEPS, want_lam=True), ref, (name, cell, what))
        dec.close()
    assert len(seen) >= 3, seen


@pytest.mark.parametrize("cell", ["f16", "i8"])
@pytest.mark.parametrize("name", ["w27", "w20"])
def test_helper_order(hip, monkeypatch, name, cell):
    """the rows in the order ldpc_csr_layer_order proposes, its layers declared: the reference on THAT matrix (the one reference not shared)"""
    monkeypatch.delenv(ENV, raising=False)
    g, llr = S.case(name), _frames(name)
    p = g.permuted(hip)
    assert p.M == g.M and np.array_equal(np.sort(p.weights), np.sort(g.weights)) and not np.array_equal(p.col_idx, g.col_idx)
    ref = _frozen(spec.decode(cell, p, llr, SWEEPS, PLAIN[0], PLAIN[1], 4.0))
    assert ref[2][:8].any() and (ref[1][:8] > 1).any()
    dec = _decoder(hip, p, p.layer_ptr, cell, PLAIN, len(llr))
    assert dec.kernel_name == _kernel_name(name, cell, False) and dec.kernel_geometry == (S.default_threads(p, p.layer_ptr), 1)
    _same(dec.decode_batch(llr.astype(np.float64), SWEEPS, want_lam=True), ref, (name, cell, "helper order"))
    dec.close()


@pytest.mark.parametrize("name", NAMES)
def test_f32_on_chip_equals_flood_and_flood_equals_oracle(hip, monkeypatch, name):
    """flood.hip layered_kernel on an irregular matrix with declared layers: its f32 instance is the f32 on-chip instance bit for bit, its f64
    instance the Double oracle's layered schedule (all ten frames: the oracle takes milliseconds)"""
    monkeypatch.delenv(ENV, raising=False)
    g, llr = S.case(name), _frames(name)
    l64 = llr.astype(np.float64)
    chip = _decoder(hip, g, g.layer_ptr, "f32", PLAIN, len(llr))
    flood = hip.Decoder(g.code(hip, g.layer_ptr), "min", "f32", len(llr), schedule="layered", path="flood")
    assert flood.path == "flood" and "layered_csr_kernel" not in flood.kernel_name
    a, b = chip.decode_batch(l64, SWEEPS, want_lam=True), flood.decode_batch(l64, SWEEPS, want_lam=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
    _same(a, _ref(name, "f32", PLAIN[0], PLAIN[1], SWEEPS), (name, "on-chip"))
    d64 = hip.Decoder(g.code(hip, g.layer_ptr), "min", "f64", len(llr), schedule="layered", path="flood")
    assert d64.path == "flood"
    bits, its, conv = d64.decode_batch(l64, SWEEPS)
    og = oracle.Graph(g.row_ptr, g.col_idx, g.N)
    o = [oracle.decode_layered(og, g.layer_ptr, "min", SWEEPS, l64[f]) for f in range(len(llr))]
    oconv, oits = np.array([x["converged"] for x in o]), np.array([x["iters"] for x in o])
    # a frame that converges after some sweeps, one that runs out, the all-zero frame and the noiseless one (both codewords before sweep 1)
    assert (oconv[:8] & (oits[:8] > 0)).any() and (~oconv[:8]).any() and oconv[8] and oconv[9] and oits[8] == 0 and oits[9] == 0
    assert np.array_equal(conv.astype(bool), oconv), (name, conv, oconv)
    assert np.array_equal(bits, np.stack([x["bits"] for x in o])), name
    assert np.array_equal(its[oconv], oits[oconv]), (name, its, oits)
    for d in (chip, flood, d64):
        d.close()


def test_more_frames_than_workgroups(hip, monkeypatch):
    """1200 frames on one fp16 context of that capacity, "w27": the class-32 instance holds 177 registers per lane, so two waves per SIMD
    and two workgroups of three waves per CU are resident -- 512 on 256 CUs; the other frames are taken from the counter"""
    monkeypatch.delenv(ENV, raising=False)
    name, F = "w27", 1200
    g, ten = S.case(name), _frames(name)
    ref = _ref(name, "f16", PLAIN[0], PLAIN[1], SWEEPS)
    idx = np.random.default_rng(1200).permutation(np.tile(np.arange(len(ten)), F // len(ten)))
    llr = np.ascontiguousarray(ten[idx])
    dec = _decoder(hip, g, g.layer_ptr, "f16", PLAIN, F)
    assert dec.kernel_name == "ldpc::layered_csr_kernel<32>" and dec.kernel_geometry == (192, 1)
    want = tuple(r[idx] for r in ref)
    _same(dec.decode_batch(llr, SWEEPS), want, "f32 LLRs", n=3)
    _same(dec.decode_batch(llr.astype(np.float64), SWEEPS, want_lam=True), want, "f64 LLRs")
    dec.close()
