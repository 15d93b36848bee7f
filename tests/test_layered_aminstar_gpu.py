"""GPU: the A-min* check-node rule (ldpc_ctx_config cn_rule = LDPC_CN_AMINSTAR) of the on-chip layered kernel for any H -- csrc/layered_csr.hip
layered_csr_kernel, layered_csr_soft_kernel and layered_csr_cont_kernel<8|20|32, MinStar<_Float16|float>> -- against its specification
tests/layered_aminstar_spec.py, bit for bit: np.array_equal everywhere, no tolerance.

Graphs: "w8", "w20", "w27" of tests/layered_shapes.py (every row weight 2..27, the three row classes, uniform and mixed waves, idle waves,
rows without edges, layers that merge) and codes/jpl.1024.4.5 as CSR (rows of weight 18, punctured columns: LLR 0, real ties).
Frames (26 per graph): twelve noisy ones at each of two Eb/N0 with the LLRs ROUNDED TO MULTIPLES OF 1/2, so that several edges of a row tie
in |t| and "the first arg-min" decides which edge gets Delta; an all-zero frame and the noiseless codeword, which stop before the first
sweep.  At most 12 sweeps.  What the specification has to give on every (graph, cell) is asserted: a frame that converges after more than
one sweep, one that runs out of sweeps, and a result that is not 3/4 min-sum's."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import layered_aminstar_spec as spec
from tests import layered_rule_spec as rule
from tests import layered_shapes as S
from tests import soft_output_spec as soft
from tests.helpers import CODES
from tests.test_layered_i8_gpu import _named

pytestmark = pytest.mark.gpu

SWEEPS = 12
NAMES = ["w8", "w20", "w27", "jpl.1024.4.5"]
CELLS = ["f16", "f32"]
DBS = {"w8": (2.5, 5.0), "w20": (5.0, 7.0), "w27": (3.0, 5.0), "jpl.1024.4.5": (2.5, 3.5)}
DCLASS = dict(S.DCLASS, **{"jpl.1024.4.5": 20})
TYPE = {"f16": "_Float16", "f32": "float"}
NOISY = 24


@functools.lru_cache(maxsize=None)
def _graph(name):
    return S.case(name) if name in S.CASES else _named(name)


@functools.lru_cache(maxsize=None)
def _frames(name):
    g = _graph(name)
    noisy = np.concatenate([g.frames(NOISY // 2, db, 300 + i) for i, db in enumerate(DBS[name])])
    noisy = (np.round(noisy * 2) / 2).astype(np.float32)
    llr = np.concatenate([noisy, np.zeros((1, g.N), np.float32), np.where(g.cw, 100.0, -100.0).astype(np.float32)[None]])
    llr.setflags(write=False)
    return llr


def _frozen(ref):
    for a in ref:
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _ref(name, cell, max_iters):
    """bits, sweeps, converged, P, C of the 26 frames; shared, never written"""
    return _frozen(spec.decode_soft(cell, _graph(name), _frames(name), max_iters))


def _final(ref):
    return np.where(ref[2][:, None], ref[3], ref[4]).astype(np.float64)


def _decoder(hip, name, cell, F, **kw):
    g = _graph(name)
    dec = hip.Decoder(g.code(hip, getattr(g, "layer_ptr", None)), "min", cell, F, schedule="layered", cn_rule="aminstar", **kw)
    assert dec.path == "fused" and dec.kernel_name == f"ldpc::layered_csr_kernel<{DCLASS[name]}, ldpc::MinStar<{TYPE[cell]}>>", dec.kernel_name
    return dec


def _bits_of(a):
    return a.view({2: np.uint16, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", NAMES)
def test_bit_exact_against_specification(hip, name, cell):
    g, llr = _graph(name), _frames(name)
    ref = _ref(name, cell, SWEEPS)
    sweeps, conv = ref[1][:NOISY], ref[2][:NOISY]
    assert (conv & (sweeps > 1)).any() and (~conv).any() and ref[2][NOISY:].all() and (ref[1][NOISY:] == 0).all(), (name, cell, ref[1], ref[2])
    # ties: in the first sweep some row of some frame has its least |LLR| on two edges
    rp = np.asarray(g.row_ptr)
    tied = False
    for m in np.flatnonzero(np.diff(rp) >= 3)[:200]:
        a = np.sort(np.abs(llr[:NOISY, g.col_idx[rp[m]:rp[m + 1]]]), axis=1)
        tied |= bool((a[:, 0] == a[:, 1]).any())
    assert tied, name
    # the specification's own result is not 3/4 min-sum's: a kernel that ignored cn_rule would fail below
    base = rule.decode_float(g, llr, SWEEPS, 0.75, 0.0, cell)
    assert not (np.array_equal(base[1], ref[1]) and np.array_equal(base[3], _final(ref).astype(np.float32))), (name, cell)
    dec = _decoder(hip, name, cell, len(llr))
    assert dec.cn_rule == "aminstar" and hip.lib().ldpc_ctx_cn_rule(dec._h) == 1 and (dec.cn_scale, dec.cn_offset) == (0.0, 0.0)
    for mi in (0, 1, SWEEPS):
        r = _ref(name, cell, mi)
        b, i, c, l = dec.decode_batch(llr.astype(np.float64), mi, want_lam=True)
        what = (name, cell, mi)
        assert np.array_equal(i, r[1]), (what, i, r[1])
        assert np.array_equal(c.astype(bool), r[2]), what
        assert np.array_equal(b, r[0]), what
        assert np.array_equal(l, _final(r)), what
    b, i, c = dec.decode_batch(llr, SWEEPS)                    # f32 LLRs, no LLR output: the 8-wide prologue where N is a multiple of 8
    assert np.array_equal(b, ref[0]) and np.array_equal(i, ref[1]) and np.array_equal(c.astype(bool), ref[2]), (name, cell, "f32")
    dec.close()


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", ["w8", "w20", "w27"])
def test_soft_output(hip, name, cell):
    llr = _frames(name).copy()                                  # (writable: the arrays travel through torch tensors)
    ref = _ref(name, cell, SWEEPS)
    bits, iters, conv, P, Cc = ref
    keep = np.isfinite(P).all(axis=1)                           # the soft output of a vetoed f32 frame is not compared
    assert keep.sum() >= len(llr) - 2
    dec = _decoder(hip, name, cell, len(llr))
    for kind in soft.KINDS:
        for fmt in soft.FORMATS:
            b, i, c, s = dec.decode_batch_soft(llr, SWEEPS, kind=kind, soft_fmt=fmt)
            what = (name, cell, kind, fmt)
            assert f"layered_csr_soft_kernel<{DCLASS[name]}, ldpc::MinStar<" in dec.kernel_name, dec.kernel_name
            assert np.array_equal(i, iters) and np.array_equal(c.astype(bool), conv) and np.array_equal(b, bits), what
            want = soft.soft(cell, P, Cc, kind, fmt)
            assert s.dtype == want.dtype and np.array_equal(_bits_of(s)[keep], _bits_of(want)[keep]), what
    dec.close()


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", ["w8", "w20", "w27"])
def test_continuation(hip, name, cell):
    g, llr = _graph(name), _frames(name).copy()
    dec = _decoder(hip, name, cell, len(llr))
    # from a reset slot the call is the soft call, bit for bit
    st = hip.DecodeState(dec, len(llr))
    a = dec.decode_batch_soft(llr, SWEEPS, kind="extrinsic", soft_fmt="f32")
    b = dec.decode_batch_continue(st, llr, SWEEPS, kind="extrinsic", soft_fmt="f32")
    assert f"layered_csr_cont_kernel<{DCLASS[name]}, ldpc::MinStar<" in dec.kernel_name, dec.kernel_name
    for x, y in zip(a, b):
        assert np.array_equal(_bits_of(x) if x.dtype == np.float32 else x, _bits_of(y) if y.dtype == np.float32 else y), (name, cell, "reset slot")
    # two calls of 3 sweeps: the continuation specification run with this row rule
    st.reset()
    state = spec.State(cell, g, len(llr))
    ran = False
    for call, kind in enumerate(("posterior", "extrinsic")):
        (rb, ri, rc, P, Cc), state = spec.call(cell, g, state, llr, 3)
        keep = np.isfinite(P).all(axis=1)
        b2, i2, c2, s2 = dec.decode_batch_continue(st, llr, 3, kind=kind, soft_fmt="f32")
        what = (name, cell, call, kind)
        assert np.array_equal(i2, ri) and np.array_equal(c2.astype(bool), rc) and np.array_equal(b2, rb), (what, i2, ri)
        assert np.array_equal(_bits_of(s2)[keep], _bits_of(soft.soft(cell, P, Cc, kind, "f32"))[keep]), what
        ran |= bool(call == 1 and (ri[:NOISY] > 0).any())
    assert ran                                                  # the second call really swept: its first sweep subtracted stored messages
    st.close()
    dec.close()


def _raw_context(hip, code, struct_size, cn_rule, cell="f16", max_batch=32):
    """ldpc_ctx_create_cfg with a structure of `struct_size` bytes -> Decoder (the handle is destroyed by the caller)"""
    from ecc_ldpc_amd import _lib
    cfg = _lib.CtxConfig(struct_size, -1, _lib._VARIANTS["min"], _lib._DTYPES[cell], max_batch, _lib._PATHS["fused"], _lib._SCHEDULES["layered"], 0, 0.0, 0.0, 0.0, cn_rule)
    h = hip.lib().ldpc_ctx_create_cfg(code._h, C.byref(cfg))
    assert h, hip.last_error()
    return hip.Decoder(code, _handle=h)


def test_the_default_is_unchanged(hip):
    """cn_rule = 0, and a structure that ends before the field (whatever the bytes there hold), are the context made without it"""
    from ecc_ldpc_amd import _lib
    name, cell = "w20", "f16"
    g, llr = _graph(name), _frames(name)
    assert _lib.CtxConfig.cn_rule.offset + 4 <= C.sizeof(_lib.CtxConfig)
    plain = hip.Decoder(g.code(hip, g.layer_ptr), "min", cell, len(llr), schedule="layered", path="fused")
    zero = hip.Decoder(g.code(hip, g.layer_ptr), "min", cell, len(llr), schedule="layered", path="fused", cn_rule="minsum")
    code = g.code(hip, g.layer_ptr)
    short = _raw_context(hip, code, _lib.CtxConfig.cn_rule.offset, 1, cell, len(llr))     # the field says A-min*, the size says "not there"
    want = plain.decode_batch(llr.astype(np.float64), SWEEPS, want_lam=True)
    base = rule.decode_float(g, llr, SWEEPS, 0.75, 0.0, cell)
    assert np.array_equal(want[0], base[0]) and np.array_equal(want[1], base[1]) and np.array_equal(want[3], base[3].astype(np.float64))
    for d in (zero, short):
        assert d.kernel_name == plain.kernel_name == f"ldpc::layered_csr_kernel<{DCLASS[name]}>" and d.cn_rule == "minsum"
        assert (d.cn_scale, d.cn_offset) == (0.75, 0.0) and hip.lib().ldpc_ctx_cn_rule(d._h) == 0
        got = d.decode_batch(llr.astype(np.float64), SWEEPS, want_lam=True)
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
    hip.lib().ldpc_ctx_destroy(short._h)
    short._h = None
    # a context of another family says LDPC_CN_MINSUM too
    assert hip.Decoder(g.code(hip), "tanh", "f32", 4).cn_rule == "minsum"


def test_selection_and_refusals(hip):
    amin = dict(cn_rule="aminstar")
    for name in ("w8", "jpl.1024.4.5"):
        g = _graph(name)
        for cell in CELLS:
            for path in ("auto", "fused"):
                d = _decoder(hip, name, cell, 8, path=path)
                assert d.cn_rule == "aminstar" and (d.cn_scale, d.cn_offset) == (0.0, 0.0)
                d.close()
    J = _named("jpl.1024.4.5", qc=True)                         # handed over quasi-cyclic: taken as its CSR form with its layers
    d = hip.Decoder(J.code(hip), "min", "f16", 8, schedule="layered", **amin)
    assert d.path == "fused" and d.kernel_name == "ldpc::layered_csr_kernel<20, ldpc::MinStar<_Float16>>"
    G = _graph("jpl.1024.4.5")
    unsupported = [dict(variant="min", dtype="i8", schedule="layered"), dict(variant="min", dtype="f32", schedule="flooding"), dict(variant="tanh", dtype="f32", schedule="layered"),
                   dict(variant="tanh-cm", dtype="f64", schedule="flooding", path="flood"), dict(variant="min", dtype="f64", schedule="flooding", sum_order="arraylet", path="flood"),
                   dict(variant="min", dtype="f64", schedule="layered"), dict(variant="min", dtype="f16pk", schedule="layered"),
                   dict(variant="min", dtype="f16", schedule="layered", path="flood"), dict(variant="min", dtype="f32", schedule="layered", path="flood"),
                   dict(variant="min", dtype="i8", schedule="flooding")]
    for kw in unsupported:
        with pytest.raises(hip.LdpcError) as e:
            hip.Decoder(G.code(hip), max_batch=8, **kw, **amin)
        assert e.value.code == -5 and "cn_rule" in str(e.value), (kw, str(e.value))
    for call in (lambda: d.decode_trace(np.zeros((2, G.N)), 3), lambda: d.debug_step(np.zeros((1, G.N)), np.zeros((1, G.N)), np.zeros((1, len(G.col_idx))))):
        with pytest.raises(hip.LdpcError) as e:
            call()
        assert e.value.code == -5 and "cn_rule" in str(e.value)
    # A-min* has no scale and no offset; an unknown rule is not a rule
    for kw in (dict(cn_scale=0.75), dict(cn_scale=1.0), dict(cn_offset=0.5), dict(cn_scale=0.875, cn_offset=0.25)):
        with pytest.raises(hip.LdpcError) as e:
            hip.Decoder(G.code(hip), "min", "f16", 8, schedule="layered", **kw, **amin)
        assert e.value.code == -1 and "cn_rule" in str(e.value), kw
    from ecc_ldpc_amd import _lib
    for bad in (2, -1, 77):
        cfg = _lib.CtxConfig(C.sizeof(_lib.CtxConfig), -1, _lib._VARIANTS["min"], _lib._DTYPES["f16"], 8, 0, _lib._SCHEDULES["layered"], 0, 0.0, 0.0, 0.0, bad)
        code = G.code(hip)
        assert not hip.lib().ldpc_ctx_create_cfg(code._h, C.byref(cfg)) and hip.lib().ldpc_last_error_code() == -1 and "cn_rule" in hip.last_error()
    # the code-name grammar: -amin after the dtype, without -s / -o
    for nm, t in (("ldpc/hip-minsum-layered-f16-amin/1920.1280.3.303/50/1/3", "_Float16"), ("ldpc/hip-minsum-layered-f32-amin/1920.1280.3.303/50/1/3", "float"),
                  ("ldpc/hip-minsum-layered-amin/1920.1280.3.303/50/1/3", "float")):
        ecc = hip.ECC(CODES, nm, max_batch=4)
        assert ecc.decoder.path == "fused" and "layered_csr_kernel<" in ecc.decoder.kernel_name and f"MinStar<{t}>" in ecc.decoder.kernel_name, ecc.decoder.kernel_name
        assert ecc.decoder.cn_rule == "aminstar" and ecc.name.startswith(nm[:nm.index("/19")])
        ecc.close()
    for bad in ("ldpc/hip-minsum-layered-f16-amin-s1/1920.1280.3.303/50/1/3", "ldpc/hip-minsum-layered-f16-s1-amin/1920.1280.3.303/50/1/3",
                "ldpc/hip-minsum-layered-f16-amin-o0.5/1920.1280.3.303/50/1/3", "ldpc/hip-minsum-f16-amin/1920.1280.3.303/50/1/3",
                "ldpc/hip-tanh-layered-amin/1920.1280.3.303/50/1/3", "ldpc/hip-minsum-layered-amin-f16/1920.1280.3.303/50/1/3"):
        with pytest.raises(hip.LdpcError) as e:
            hip.ECC(CODES, bad, max_batch=4)
        assert e.value.code == -8, bad
    with pytest.raises(hip.LdpcError) as e:                     # the dtype the rule does not exist for: the context's refusal
        hip.ECC(CODES, "ldpc/hip-minsum-layered-i8-amin/1920.1280.3.303/50/1/3", max_batch=4)
    assert e.value.code == -5 and "cn_rule" in str(e.value)


@pytest.mark.parametrize("name", ["w8", "w27"])
def test_non_finite_frames_fail_and_leave_their_neighbours_alone(hip, name):
    """rules 3 and 6 of include/ldpc_hip.h on f32 cells: a frame given a NaN or an infinity fails -- converged 0, the sweep limit as its
    count, bits = llr > 0, final_lam = the LLRs as given --, also one whose decisions already are a codeword; the finite frames of the same
    batch come back bit for bit the specification's"""
    g = _graph(name)
    base = _frames(name)
    pick = [0, 1, NOISY // 2, NOISY // 2 + 1, NOISY, NOISY + 1]         # noisy at both Eb/N0, the all-zero frame, the noiseless codeword
    rng = np.random.default_rng(6)
    rows, kinds = [], []
    for f in pick:
        rows.append(base[f]); kinds.append(None)
        for v in (np.nan, np.inf, -np.inf):
            x = base[f].copy()
            x[rng.choice(g.col_idx, 3)] = v                              # columns some row reads
            rows.append(x); kinds.append(v)
    llr = np.stack(rows).astype(np.float32)
    finite = np.array([k is None for k in kinds])
    ref = spec.decode_soft("f32", g, llr[finite], SWEEPS)
    assert ref[2].any() and (~ref[2]).any()
    dec = _decoder(hip, name, "f32", len(llr))
    b, i, c, l = dec.decode_batch(llr.astype(np.float64), SWEEPS, want_lam=True)
    assert np.array_equal(b[finite], ref[0]) and np.array_equal(i[finite], ref[1]) and np.array_equal(c[finite].astype(bool), ref[2])
    assert np.array_equal(l[finite], _final(ref))
    bad = ~finite
    assert not c[bad].any() and (i[bad] == SWEEPS).all()
    assert np.array_equal(b[bad], (llr[bad] > 0).astype(np.uint8))
    assert np.array_equal(l[bad], llr[bad].astype(np.float64), equal_nan=True)
    b2, i2, c2 = dec.decode_batch(llr, SWEEPS)                           # f32 in: the 8-wide prologue and epilogue
    assert np.array_equal(b2, b) and np.array_equal(i2, i) and np.array_equal(c2, c)
    dec.close()
