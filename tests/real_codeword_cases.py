"""The cases of tests/test_real_codewords_gpu.py, their frames and their references (TEST INFRASTRUCTURE, no GPU needed): one case per
kernel family and context, on the smallest codes that family's own test file uses.  tests/test_codewords.py asserts on the CPU what the
GPU module rests on; the GPU module decodes the same frames.

A case's frames (frames_of): `F` noisy frames of random REAL codewords (tests/codewords.py), half at each of its two Eb/N0, unpunctured;
then a noiseless codeword at +-8 and its flip (the all-zero word at -8).  The words that go with them (the last two rows: that
codeword, twice) turn every frame into its mirror image under codewords.flip.

A reference (reference_of) is what the family's own test file compares with:
    "oracle"        the Double oracle, flooding: whole trajectory (f64 contexts), or hard bits / flags / turn counts (f32 contexts)
    "oracle-layered" the same for the layered schedule
    "f16-flood", "pk16", "pk16-layered", "f16-layered"   the bit-exact emulations of oracle/emulate_f16.py
    ("spec", cell)  tests/layered_rule_spec.py decode with the case's rule: the specification of every layered min-sum kernel whose lam
                    cells are fp16, f32 or int8.  The f32 layered kernels (flood.hip layered_kernel, layered_qc_kernel, the on-chip
                    ones) are held equal to one another bit for bit by their own tests and the any-H one to this specification, so it
                    is the exact bar of them all; tests/test_codewords.py holds it to the Double oracle's bits and flags on these frames.
Every reference is returned as (bits, turns, converged, final_lam or None, trace or None), read-only and shared."""
from __future__ import annotations

import functools

import numpy as np

from oracle import emulate_f16 as em
from oracle import oracle
from tests import codewords as cwm
from tests import layered_rule_spec as spec
from tests import layered_shapes as S
from tests.helpers import load, synthetic

TURNS = 25
LOADED = ("jpl.1024.4.5", "jpl.4096.4.5", "1920.1280.3.303", "1920.1280.A")
DEGENERATE = {"latin-24x16-sz64": 1, "latin-18x9-sz40": 0}         # name -> dimension: the all-ones word only; the zero word only
RULED = (1.0, 0.5)


class Code:
    """one parity-check matrix with what the references, the frames and the library need"""

    def __init__(self, name):
        self.name = name
        if name in S.CASES:
            g = S.case(name)
            rp, ci, self.N, self.k, self.layer_ptr = g.row_ptr, g.col_idx, g.N, g.k, np.asarray(g.layer_ptr)
            self._make = lambda hip, qc: g.code(hip, g.layer_ptr)
        elif name == "dvbs2_short":     # in the row order ldpc_csr_layer_order proposes, its layers declared (host code: no GPU needed)
            import ecc_ldpc_amd as E
            from tests import dvbs2_short
            rp0, ci0 = dvbs2_short.csr()
            perm, lp = E.Code.csr_layer_order(rp0, ci0, dvbs2_short.N, 0)
            rp, ci = E.Code.permute_rows(rp0, ci0, perm)
            self.N, self.k, self.layer_ptr = dvbs2_short.N, dvbs2_short.K, np.asarray(lp)
            self._natural = oracle.Graph(rp0, ci0, self.N)         # (the triangular encoder wants the natural order; same code)

            def make(hip, qc, rp=rp, ci=ci, lp=lp):
                c = hip.Code.from_csr(rp, ci, dvbs2_short.N)
                c.set_layers(lp)
                return c
            self._make = make
        elif name in LOADED:
            c = load(name)
            rp, ci, self.N, self.k = c.graph.row_ptr, c.graph.col_idx, c.N, c.k
            self.layer_ptr = np.arange(0, c.M + 1, c.sz) if c.sz else np.arange(c.M + 1)
            self._make = lambda hip, qc: c.hip_code(hip, prefer_qc=qc)
        else:
            c = synthetic(name)
            rp, ci, self.N, self.k, self.layer_ptr = c.graph.row_ptr, c.graph.col_idx, c.N, c.k, c.layer_ptr
            self._make = lambda hip, qc: c.hip_code(hip)
        self.graph = oracle.Graph(rp, ci, self.N)
        self.M, self.E = self.graph.M, self.graph.E

    def hip_code(self, hip, qc=True):
        return self._make(hip, qc)

    def codewords(self, F, seed):
        return cwm.codewords(getattr(self, "_natural", self.graph), F, seed)


@functools.lru_cache(maxsize=None)
def code(name) -> Code:
    return Code(name)


class Case:
    def __init__(self, id, code, ref, dbs, kernel, variant="min", dtype="f32", path="auto", schedule="flooding", qc=True, env=None, rule=None,
                 F=8, seed=1, pair=None, step=None, sym="exact", native_i8=False, stuck=False):
        """kernel: substrings the context's kernel_name must hold (the first one: at its start when it begins with "ldpc");
        pair: (Decoder keywords that replace the case's, environment, kernel substrings, how many of bits / turns / flags / final_lam
        the family's own test holds equal); step: "flood" | "layered", one teacher-forced debug_step from oracle states;
        sym: "exact" | "loose" (f64 tanh: the reference's formula is not odd in floating point); stuck: no noisy frame converges on the
        reference at any Eb/N0 (the one such instance: see below)"""
        self.id, self.code, self.ref, self.dbs, self.kernel = id, code, ref, dbs, kernel if isinstance(kernel, tuple) else (kernel,)
        self.variant, self.dtype, self.path, self.schedule, self.qc = variant, dtype, path, schedule, qc
        self.env, self.rule, self.F, self.seed, self.pair, self.step, self.sym, self.native_i8 = env or {}, rule, F, seed, pair, step, sym, native_i8
        self.stuck = stuck

    def decoder_kw(self):
        kw = dict(variant=self.variant, dtype=self.dtype, path=self.path, schedule=self.schedule)
        if self.rule:
            kw.update(cn_scale=self.rule[0], cn_offset=self.rule[1])
        return kw

    @property
    def ref_key(self):
        """cases that share frames and a reference share its computation"""
        return (self.code, self.ref, self.variant, self.rule, self.dbs, self.F, self.seed)


def _cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    flood_pair = lambda kernel: (dict(path="flood"), {}, (kernel,), 3)
    # ---- run-time specialised split kernel (jit.cc JIT_SPLIT): f32 against the Double oracle, and equal to the flood path
    for name, dbs in (("small-2x4-sz32", (1.0, 3.0)), ("wifi-12x24-sz27", (1.5, 3.0)), ("irregular-20x30-sz64", (2.0, 4.0)), ("wide-4x40-sz256", (4.5, 6.0))):
        for v in ("min", "tanh"):
            add(f"jit_split-{v}-{name}", name, "oracle", dbs, "ldpc_jit_split_", variant=v, path="fused", pair=flood_pair("flood_qc_kernel"), step="flood")
    # ---- the other run-time specialised kinds, on the two smallest shapes of tests/test_jit_kinds_gpu.py
    for name, dbs in (("small-2x4-sz32", (3.0, 5.0)), ("wifi-12x24-sz27", (1.5, 3.0))):
        add(f"jit_pk16-{name}", name, "pk16", dbs, "ldpc_jit_pk16_minsum_sz", dtype="f16pk")
        add(f"jit_layered_pk16-{name}", name, "pk16-layered", dbs, "ldpc_jit_layered_pk16_minsum_sz", dtype="f16pk", schedule="layered")
        add(f"jit_layered-{name}", name, ("spec", "f32"), dbs, "ldpc_jit_layered_minsum_sz", schedule="layered",
            pair=(dict(path="flood"), {}, ("layered_qc_kernel",), 4))
    # ---- the two-wave table-driven kernel (fused_msg.hip)
    for v in ("min", "tanh"):
        add(f"fused_msg-dyn-{v}", "jpl.1024.4.5", "oracle", (3.0, 5.0), "fused_msg_kernel", variant=v, path="fused", env={"LDPC_FUSED_TABLE": "dyn"},
            pair=flood_pair("flood_qc_kernel"), step="flood")
    add("fused_msg-msg-min", "jpl.1024.4.5", "oracle", (3.0, 5.0), "fused_msg_kernel", path="fused", env={"LDPC_FUSED_KERNEL": "msg"}, pair=flood_pair("flood_qc_kernel"))
    # ---- the generic on-chip kernel (fused_csr.hip)
    for name, dbs in (("1920.1280.3.303", (1.0, 2.0)), ("jpl.1024.4.5", (3.0, 4.0))):
        for v in ("min", "tanh"):
            add(f"fused_csr-{v}-f32-{name}", name, "oracle", dbs, "fused_csr", variant=v, path="fused", qc=False, pair=flood_pair("flood_cn_kernel"), step="flood")
    add("fused_csr-min-f64-1920.1280.3.303", "1920.1280.3.303", "oracle", (1.0, 2.0), "fused_csr", dtype="f64", path="fused", qc=False)
    add("fused_csr-tanh-f64-1920.1280.3.303", "1920.1280.3.303", "oracle", (1.0, 2.0), "fused_csr", variant="tanh", dtype="f64", path="fused", qc=False, sym="loose")
    # ---- one workgroup per frame, state in HBM (layered_qc.hip): flood_qc_kernel and layered_qc_kernel
    for name, dbs, ldbs in (("ira-12x24-sz64", (1.5, 3.0), (1.0, 2.0)), ("small-2x4-sz32", (1.0, 3.0), (3.0, 6.0))):
        add(f"flood_qc-min-f32-{name}", name, "oracle", dbs, "flood_qc_kernel<float", path="flood", step="flood")
        add(f"flood_qc-tanh-f32-{name}", name, "oracle", (1.0, 3.0), "flood_qc_kernel<float", variant="tanh", path="flood", step="flood")
        add(f"flood_qc-min-f64-{name}", name, "oracle", dbs, "flood_qc_kernel<double", dtype="f64", path="flood")
        add(f"layered_qc-min-f32-{name}", name, ("spec", "f32"), ldbs, "layered_qc_kernel<float", path="flood", schedule="layered", step="layered")
        add(f"layered_qc-min-f64-{name}", name, "oracle-layered", ldbs, "layered_qc_kernel<double", dtype="f64", path="flood", schedule="layered")
        add(f"layered_qc-min-f16-{name}", name, "f16-layered", ldbs, ("layered_qc_kernel<float", "__half"), dtype="f16", path="flood", schedule="layered",
            env={"LDPC_LAYERED_LDS": "0"})
    # ---- the batch-major kernels for any H (flood.hip)
    m = "1920.1280.3.303"
    add("flood-min-f32", m, "oracle", (1.0, 2.5), "flood_cn_kernel", path="flood", step="flood")
    add("flood-tanh-f32", m, "oracle", (1.0, 2.5), "flood_cn_kernel", variant="tanh", path="flood", step="flood")
    add("flood-min-f64", m, "oracle", (1.0, 2.5), "flood_cn_kernel", dtype="f64", path="flood")
    add("flood-min-f16", m, "f16-flood", (1.0, 2.0), "flood_cn_kernel", dtype="f16", path="flood")
    add("flood-layered-f32-w8", "w8", ("spec", "f32"), (2.5, 5.0), "layered_kernel", path="flood", schedule="layered",
        pair=(dict(path="fused"), {}, ("ldpc::layered_csr_kernel<8, float>",), 4))
    add("flood-layered-f64-w8", "w8", "oracle-layered", (2.5, 5.0), "layered_kernel", dtype="f64", path="flood", schedule="layered")
    add("flood-heavy-columns-min-f32", "1920.1280.A", "oracle", (1.5, 2.5), "flood_cn_kernel", path="flood", F=4)
    # ---- layered min-sum, fp16 lam in LDS, QC codes (layered_lds.hip).  latin-18x9-sz40 has rank N: its only codeword is the zero word
    # (its rows have weight 3, so the all-ones word is none); latin-24x16-sz64 is the shape with the all-ones word
    for name, dbs in (("latin-18x9-sz40", (-8.0, 3.0)), ("latin-24x16-sz64", (-1.0, 3.0))):
        add(f"layered_lds-{name}", name, "f16-layered", dbs, "layered_lds_kernel", dtype="f16", path="flood", schedule="layered")
    # (7200 rows: the emulation's row-by-row loop takes 10 s, the specification groups rows; tests/test_layered_rule_spec.py holds the two equal)
    add("layered_lds-dvbs2short-20x45-sz360", "dvbs2short-20x45-sz360", ("spec", "f16"), (1.0, 2.0), "layered_lds_kernel", dtype="f16", path="flood", schedule="layered", F=4)
    # ---- layered min-sum for any H, lam on-chip (layered_csr.hip): all eighteen instances
    dbs_of = {"w8": (2.5, 5.0), "w20": (5.0, 7.0), "w27": (3.0, 5.0)}
    ctype = {"f16": "_Float16", "f32": "float", "i8": "signed char"}
    for name in S.CASES:
        d = S.DCLASS[name]
        for cell in ("f16", "f32", "i8"):
            plain = f"ldpc::layered_csr_kernel<{d}>" if cell == "f16" else f"ldpc::layered_csr_kernel<{d}, {ctype[cell]}>"
            # int8 lam cells are often exactly 0, and hard(0) = 0 serves the all-zero word: with seed 1 frame 1 of "w20" stops one sweep
            # apart from its mirror image on the SPECIFICATION (as does frame 5 of "w8" under the rule (1/2, 0) below): seed 2 there
            add(f"layered_csr-{cell}-plain-{name}", name, ("spec", cell), dbs_of[name], plain, dtype=cell, path="fused", schedule="layered", native_i8=cell == "i8",
                seed=2 if (name, cell) == ("w20", "i8") else 1)
            add(f"layered_csr-{cell}-ruled-{name}", name, ("spec", cell), dbs_of[name], f"ldpc::layered_csr_kernel<{d}, ldpc::Ruled<{ctype[cell]}>>", dtype=cell, path="fused",
                schedule="layered", rule=RULED, native_i8=cell == "i8", stuck=(name, cell) == ("w8", "i8"))
    # the int8 cell with the rule (1, 0.5) converges on no noisy frame of "w8" (tests/test_layered_csr_shapes_gpu.py): the rule (1/2, 0) as well
    add("layered_csr-i8-ruled-half-w8", "w8", ("spec", "i8"), dbs_of["w8"], "ldpc::layered_csr_kernel<8, ldpc::Ruled<signed char>>", dtype="i8", path="fused", schedule="layered",
        rule=(0.5, 0.0), native_i8=True, seed=2)
    add("layered_csr-f16-plain-dvbs2_short", "dvbs2_short", ("spec", "f16"), (1.5, 2.5), "ldpc::layered_csr_kernel<", dtype="f16", schedule="layered", F=4)
    # ---- the built-in kernels of the shipped AR4JA codes, here WITHOUT puncturing (their own tests puncture)
    for name, dbs, ldbs in (("jpl.1024.4.5", (3.0, 5.0), (2.5, 3.5)), ("jpl.4096.4.5", (2.5, 3.5), (2.5, 3.5))):
        add(f"builtin_split-{name}", name, "oracle", dbs, "fused_split_kernel", pair=flood_pair("flood_qc_kernel"), step="flood")
        add(f"builtin_pk16-{name}", name, "pk16", dbs, "fused_pk16_kernel", dtype="f16pk")
        add(f"builtin_layered-{name}", name, ("spec", "f32"), ldbs, "fused_layered_kernel", schedule="layered", pair=(dict(path="flood"), {}, ("layered_qc_kernel",), 4))
    assert len({c.id for c in out}) == len(out)
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


# ------------------------------------------------------------------------------------------------------------------ frames
@functools.lru_cache(maxsize=None)
def _frames(name, dbs, F, seed):
    c = code(name)
    if DEGENERATE.get(name) == 0:
        cws = np.zeros((F + 1, c.N), np.uint8)
    elif DEGENERATE.get(name) == 1:                 # the two words of the code, in turn
        cws = np.zeros((F + 1, c.N), np.uint8)
        cws[0::2] = 1
        assert not (np.add.reduceat(cws[0][c.graph.col_idx], c.graph.row_ptr[:-1]) & 1).any()
    else:
        cws = c.codewords(F + 1, 1000 + seed)
    h = F // 2
    llr = np.concatenate([cwm.noisy(cws[:h], dbs[0], c.k, c.N, 2000 + seed), cwm.noisy(cws[h:F], dbs[1], c.k, c.N, 3000 + seed),
                          cwm.noiseless(cws[F]).astype(np.float64)])
    cws = np.concatenate([cws[:F], cws[F:], cws[F:]])
    assert llr.shape == cws.shape == (F + 2, c.N) and np.array_equal(llr[F + 1], cwm.flip(llr[F], cws[F]))
    llr.setflags(write=False); cws.setflags(write=False)
    return llr, cws


def frames_of(case):
    """-> (llr [F + 2][N] float64 holding float32 values, words [F + 2][N] uint8)"""
    return _frames(case.code, case.dbs, case.F, case.seed)


# -------------------------------------------------------------------------------------------------------------- references
def _frozen(bits, its, conv, lam=None, trace=None):
    out = [np.asarray(bits, np.uint8), np.asarray(its, np.int32), np.asarray(conv).astype(bool), None if lam is None else np.asarray(lam, np.float64), trace]
    for a in out[:4]:
        if a is not None:
            a.setflags(write=False)
    return tuple(out)


def _oracle(c, variant, llr, layered):
    o = [oracle.decode_layered(c.graph, c.layer_ptr, variant, TURNS, l, trace=True) if layered else oracle.decode(c.graph, variant, TURNS, l, trace=True) for l in llr]
    return _frozen(np.stack([x["bits"] for x in o]), [x["iters"] for x in o], [x["converged"] for x in o], np.stack([x["lam"] for x in o]), o)


def compute_reference(case, llr):
    """the case's reference on ANY frames of its code (tests/test_codewords.py decodes the mirror images with it)"""
    c, ref = code(case.code), case.ref
    l32 = np.asarray(llr, np.float32)
    if ref == "oracle" or ref == "oracle-layered":
        return _oracle(c, case.variant, np.asarray(llr, np.float64), ref == "oracle-layered")
    if ref == "f16-flood":
        b, i, v, t = em.decode_minsum_f16_flood(c.graph, l32, TURNS)
        lam = em.r16(l32).astype(np.float64)                  # a frame out of turns: the channel LLRs as stored
        for f in np.flatnonzero(v):
            lam[f] = t[i[f]][f].astype(np.float64)
        return _frozen(b, i, v, lam, t)
    if ref in ("pk16", "pk16-layered"):
        b, i, v, t = (em.decode_minsum_pk16 if ref == "pk16" else em.decode_minsum_pk16_layered)(c.graph, l32, TURNS)
        lam = -em.neg_llr16(l32).astype(np.float64)          # a frame out of turns: the channel LLRs as stored
        for f in np.flatnonzero(v):
            lam[f] = t[i[f]][f].astype(np.float64)
        return _frozen(b, i, v, lam, t)
    if ref == "f16-layered":
        return _frozen(*em.decode_minsum_f16_layered(c.graph, l32, TURNS))
    kind, cell = ref
    assert kind == "spec"
    alpha, beta = case.rule or (0.75, 0.0)
    return _frozen(*spec.decode(cell, c.graph, l32, TURNS, alpha, beta, 4.0))


_refs = {}


def reference_of(case):
    if case.ref_key not in _refs:
        _refs[case.ref_key] = compute_reference(case, frames_of(case)[0])
    return _refs[case.ref_key]


def exercised(case, ref):
    """of the noisy frames one converges after more than one turn and one runs out of turns"""
    its, conv = ref[1][:case.F], ref[2][:case.F]
    if case.stuck:
        return not conv.any()
    return bool((conv & (its > 1)).any() and (~conv).any())


def mirrored(ref, cws):
    """what the symmetry says the reference of the mirror images is, given the reference of the frames: (bits -- they hold wherever
    final_lam != 0 --, turns, flags, final_lam)"""
    lam = None if ref[3] is None else cwm.flip(ref[3], cws)
    return ref[0] ^ cws, ref[1], ref[2], lam
