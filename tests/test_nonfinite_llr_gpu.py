"""NaN and infinite channel LLRs through every decoder family, held to the six rules include/ldpc_hip.h states next to the decode
entry points ("Non-finite channel LLRs"):

  1  converting conversions (fp16 storage and LDPC_F16 rounding +-65504, LDPC_F16PK +-16384, LDPC_I8 +-127): +inf -> +max, -inf -> -max,
     NaN -> +0; afterwards the frame is an ordinary finite frame -- held to oracle/emulate_f16.py and tests/layered_i8_spec.py, exactly;
  2  f32 and f64 state takes the values as they are;
  3  f32 min-sum: a frame with any non-finite channel LLR fails -- converged 0, iters = max_iters, bits = llr > 0, final lam = the
     channel LLRs -- also when the channel's hard decisions already are a codeword;
  4  tanh and f64 contexts: no parity with the oracle on such input, but
  5  self-consistency: converged => H bits = 0 (on the host, from the CSR) and bits = hard(final lam); not converged => iters =
     max_iters and bits = hard(the channel LLRs as taken in);
  6  isolation: the finite frames of a batch come back bit for bit the same -- bits, iters, flags, final lam -- whatever sits beside them.

Rule 6 is judged against the same call with every poisoned frame replaced by the finite frame it was made from, and that clean call's
finite frames are held to the bar of the kernel's own test file (the Double oracle: hard bits and flags exact; the fp16 / int8
emulations: everything exact), so that isolation is not judged by the code under test alone.

Poisoned frames, each made from a finite frame the oracle decodes (CPU premise test below): one NaN in a transmitted column; the same
with the sign bit set (0xFFC00000); all NaN (both signs); +inf on three columns whose sign is right; +inf and -inf on two columns of one
check, both wrong-signed; a noiseless codeword at +-8 with one right-signed +inf (syndrome zero before the first turn: f32
min-sum still fails it, the converting formats return it converged at 0).

Placement, asserted per context from Decoder.kernel_geometry: the frame -> lane map of the on-chip QC kernels is csrc/fused_frame.h
Where -- frame = (workgroup * CPW + lane % CPW) * FPL + h, CPW = 64 / sz slots interleaved lane by lane for a power-of-two sz below 64,
else 1 (sz 27: one frame per workgroup, nothing shared), FPL = 2 halves of a packed-fp16 word -- so frames 2j and 2j + 1 share a lane
(pk16) and the frames of one workgroup share every wave; csrc/flood.hip keeps frame b in lane b % 64 of slab b / 64; the persistent
kernels (layered_lds, layered_csr, fused_csr_batched) start on frame blockIdx.x and take the next id from a counter.  Batches of 13 on
chip and 70 batch-major, a poisoned frame first and one last.  For the persistent kernels a second test uses more frames than workgroups
can be resident (32 waves per CU bound the grid) with EVERY frame below that bound poisoned: whichever workgroup takes the first
finite frame has just finished a poisoned one.
"""
import functools

import numpy as np
import pytest

from oracle import channel
from oracle import emulate_f16 as em
from oracle import oracle
from tests import layered_i8_spec as i8spec
from tests import layered_rule_spec as rulespec
from tests.helpers import load, synthetic

TURNS = 20
RULE = dict(cn_scale=0.8125, cn_offset=0.125)
NAN_POS, NAN_NEG = np.array([0x7FC00000, 0xFFC00000], np.uint32).view(np.float32)
# what an fp16 buffer holds for them: +inf, -inf, NaN, NaN with the sign bit, a signalling NaN
H_PINF, H_NINF, H_NAN, H_NNAN, H_SNAN = np.array([0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01], np.uint16).view(np.float16)
POISONS = ("nan", "nan_neg", "all_nan", "inf_right", "inf_mixed", "codeword_inf")
AT13 = (0, 2, 5, 7, 10, 12)                          # poisoned frames of a batch of 13: first, last, an odd batch
AT70 = (0, 2, 5, 7, 10, 12, 31, 63, 64, 69)          # ... of 70: both slabs of 64 hold poisoned and finite frames


# ---------------------------------------------------------------------------------------------------------------- codes and frames
def _null_vector(H, seed):
    """a random codeword of H over GF(2) (the synthetic codes ship no generator; the all-zero word has no right-signed +inf)"""
    A = H.astype(np.uint8).copy()
    M, N = A.shape
    piv, r = [], 0
    for c in range(N):
        nz = np.flatnonzero(A[r:, c])
        if not len(nz):
            continue
        p = r + nz[0]
        A[[r, p]] = A[[p, r]]
        others = np.flatnonzero(A[:, c])
        A[others[others != r]] ^= A[r]
        piv.append(c)
        r += 1
        if r == M:
            break
    free = np.setdiff1d(np.arange(N), piv)
    x = np.zeros(N, np.uint8)
    x[free] = np.random.default_rng(seed).integers(0, 2, len(free))
    x[piv] = (A[:len(piv)][:, free].astype(np.int64) @ x[free]) & 1
    assert not ((H.astype(np.int64) @ x) & 1).any() and x.any()
    return x


class Case:
    """a code with what the frames, the references and the library need; db = (an Eb/N0 the oracle decodes at, one it also fails at)"""

    def __init__(self, name):
        self.name = name
        if name.startswith("rand"):           # a small random graph: column weight 3, rows of weight about 6; rand205: N % 8 != 0
            N = int(name[4:])
            M = N // 2
            rng = np.random.default_rng(N)
            H = np.zeros((M, N), np.uint8)
            for _ in range(3):
                perm = rng.permutation(N)
                for m, cols in enumerate(np.array_split(perm, M)):
                    H[m, cols] = 1
            self.H, self.sz, self.k, self.n_tx, self.db = H, 0, N - M, N, (5.0, 1.5)
            self.cw = lambda seed: _null_vector(H, seed)
            self.offsets = None
        elif name in ("moon.7.13", "jpl.1024.4.5"):
            c = load(name)
            self.H, self.sz, self.k, self.n_tx, self.offsets = c.H, c.sz, c.k, c.n_tx, c.offsets
            self.cw = lambda seed: c.encode(np.random.default_rng(seed).integers(0, 2, c.k).astype(np.uint8))
            self.db = (6.0, 0.0) if name == "moon.7.13" else (8.0, 2.5)
        else:
            c = synthetic(name)
            self.H, self.sz, self.k, self.n_tx, self.offsets = c.H, c.sz, c.k, c.n_tx, c.offsets
            self.cw = lambda seed: _null_vector(c.H, seed)
            self.db = (7.0, 2.0) if name == "small-2x4-sz32" else (4.0, 1.5)
        self.M, self.N = self.H.shape
        self.graph = oracle.Graph.from_dense(self.H)
        self.rows = [self.graph.col_idx[self.graph.row_ptr[m]:self.graph.row_ptr[m + 1]] for m in range(self.M)]
        self.layer_ptr = np.arange(self.M + 1, dtype=np.int32)      # rows in ascending order: what every layered kernel's order amounts to

    def code(self, hip, qc=True):
        if self.offsets is not None and qc:
            return hip.Code.from_qc(self.sz, self.offsets)
        return hip.Code.from_csr(self.graph.row_ptr, self.graph.col_idx, self.N)

    def syndrome_zero(self, bits):
        b = np.asarray(bits).astype(bool)
        return np.array([not any(np.logical_xor.reduce(f[cols]) for cols in self.rows) for f in b])

    def frames(self, F, db, seed):
        """-> codewords [F, N] u8, LLRs [F, N] float32"""
        cws = np.stack([self.cw(seed + 17 * f) for f in range(F)])
        return cws, channel.frames(cws, db, self.k, self.n_tx, self.N, seed).astype(np.float32)

    def poison(self, kind, cw, x):
        """the poisoned version of the finite frame x (codeword cw)"""
        x = x.copy()
        tx = np.flatnonzero(x != 0)                      # transmitted columns (a punctured column holds +0)
        ones = np.flatnonzero((cw == 1) & (x != 0))
        assert len(ones) >= 3
        if kind == "nan":
            x[tx[len(tx) // 3]] = NAN_POS
        elif kind == "nan_neg":
            x[tx[len(tx) // 2]] = NAN_NEG
        elif kind == "all_nan":
            x[0::2], x[1::2] = NAN_POS, NAN_NEG
        elif kind == "inf_right":
            x[ones[[0, len(ones) // 2, -1]]] = np.inf
        elif kind == "inf_mixed":                        # two columns of one check: +inf on a 0 bit and -inf on a 1 bit, both wrong-signed
            m = next(m for m, cols in enumerate(self.rows) if len(set(cw[cols])) == 2)
            x[next(c for c in self.rows[m] if cw[c] == 0)] = np.inf
            x[next(c for c in self.rows[m] if cw[c] == 1)] = -np.inf
        elif kind == "codeword_inf":
            x[:] = np.where(cw == 1, 8.0, -8.0)
            x[ones[1]] = np.inf
        return x

    @functools.lru_cache(maxsize=None)
    def batch(self, F):
        """-> (poisoned [F, N] f32, clean [F, N] f32, finite frame ids, {poisoned frame id: kind}): finite frames half at each Eb/N0;
        a poisoned frame and the clean frame in its place come from one frame at the Eb/N0 the oracle decodes at"""
        at = AT13 if F == 13 else AT70
        cws_hi, hi = self.frames(F, self.db[0], 1000 + F)
        _, lo = self.frames(F, self.db[1], 2000 + F)
        clean = np.where((np.arange(F) % 2 == 0)[:, None], hi, lo)
        kinds = {f: POISONS[i % len(POISONS)] for i, f in enumerate(at)}
        clean[list(at)] = hi[list(at)]
        bad = clean.copy()
        for f, kind in kinds.items():
            bad[f] = self.poison(kind, cws_hi[f], hi[f])
        finite = np.array([f for f in range(F) if f not in kinds])
        assert F % 2 == 1 or F == 70
        assert 0 in kinds and F - 1 in kinds and np.isfinite(clean).all() and np.isfinite(bad[finite]).all()
        assert not np.isfinite(bad[list(at)]).all(axis=1).any()
        return bad, clean, finite, kinds


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ---------------------------------------------------------------------------------------------------------------- contexts
# id -> (code, qc form, Decoder arguments, environment, what kernel_name must hold, numerics, batch)
#   numerics: "f32min"  rules 3, 5, 6; clean frames: the flooding ("F") or layered ("L") Double oracle, hard bits and flags exact
#             "parity"  rules 5, 6 (f64, tanh); clean frames: that oracle, hard bits and flags exact
#             "f16" "f16L" "pk16" "pk16L" "i8" "ruled16"  rule 1: the emulation, everything exact, poisoned frames included
#             "r16"     LDPC_F16 on an on-chip f32 kernel: equal to the same kernel in f32 (the context `twin`) fed emulate_f16.r16(llr)
#             "ruled32" rules 3, 5, 6; clean frames: tests/layered_rule_spec.py, everything exact
def _contexts():
    out = {}

    def add(cid, code, args, kernel, numerics, F=13, env=None, qc=True, ref="F", twin=None):
        out[cid] = dict(code=code, args=args, kernel=kernel, numerics=numerics, F=F, env=env or {}, qc=qc, ref=ref, twin=twin)

    # Not here: flood_qc_kernel, and the two on-chip kernels that are not under the rules yet (item 0a): the
    # flooding packed-fp16 kernel (a NaN is the LLR -16384 in its load) and the on-chip layered f32 kernel (LDPC_F16 rounding makes a
    # NaN -65504; a frame whose channel decisions are a codeword stops before sweep 1 with its infinity)
    j = "jpl.1024.4.5"
    add("jpl1024-split", j, dict(variant="min", dtype="f32", path="fused"), ("fused_split_kernel",), "f32min")
    add("jpl1024-msg", j, dict(variant="min", dtype="f32", path="fused"), ("fused_msg_kernel",), "f32min", env={"LDPC_FUSED_KERNEL": "msg"})
    add("jpl1024-split-f16", j, dict(variant="min", dtype="f16", path="fused"), ("fused_split_kernel",), "r16", twin="jpl1024-split")
    add("jpl1024-msg-f16", j, dict(variant="min", dtype="f16", path="fused"), ("fused_msg_kernel",), "r16", env={"LDPC_FUSED_KERNEL": "msg"}, twin="jpl1024-msg")
    add("jpl1024-layered-pk16", j, dict(variant="min", dtype="f16pk", schedule="layered"), ("fused_layered_pk16_kernel",), "pk16L")
    for s in ("small-2x4-sz32", "wifi-12x24-sz27"):
        sz = s[-2:]
        add(f"{s}-jit-split", s, dict(variant="min", dtype="f32"), (f"ldpc_jit_split_minsum_sz{sz}_",), "f32min")
        add(f"{s}-jit-layered-pk16", s, dict(variant="min", dtype="f16pk", schedule="layered"), (f"ldpc_jit_layered_pk16_minsum_sz{sz}_",), "pk16L")
        add(f"{s}-layered-qc-f32", s, dict(variant="min", dtype="f32", schedule="layered", path="flood"), ("layered_qc_kernel", "float"), "f32min", ref="L")
        add(f"{s}-layered-qc-f64", s, dict(variant="min", dtype="f64", schedule="layered"), ("layered_qc_kernel", "double"), "parity", ref="L")
        add(f"{s}-layered-qc-half", s, dict(variant="min", dtype="f16", schedule="layered", path="flood"), ("layered_qc_kernel", "__half"), "f16L",
            env={"LDPC_LAYERED_LDS": "0"})
        add(f"{s}-layered-lds", s, dict(variant="min", dtype="f16", schedule="layered", path="flood"), ("layered_lds_kernel",), "f16L")
    for g in ("moon.7.13", "rand205"):
        add(f"{g}-fused-csr", g, dict(variant="min", dtype="f32", path="fused"), ("fused_csr",), "f32min", qc=False)
        add(f"{g}-fused-csr-f16", g, dict(variant="min", dtype="f16", path="fused"), ("fused_csr",), "r16", qc=False, twin=f"{g}-fused-csr")
        add(f"{g}-fused-csr-tanh", g, dict(variant="tanh", dtype="f32", path="fused"), ("fused_csr",), "parity", qc=False, ref="Ft")
        add(f"{g}-flood-f32", g, dict(variant="min", dtype="f32", path="flood"), ("flood_cn_kernel",), "f32min", F=70, qc=False)
        add(f"{g}-flood-f16", g, dict(variant="min", dtype="f16", path="flood"), ("flood_cn_kernel",), "f16", F=70, qc=False)
        add(f"{g}-flood-f64", g, dict(variant="min", dtype="f64", path="flood"), ("flood_cn_kernel",), "parity", F=70, qc=False)
        add(f"{g}-flood-tanh", g, dict(variant="tanh", dtype="f32", path="flood"), ("flood_cn_kernel",), "parity", F=70, qc=False, ref="Ft")
        add(f"{g}-flood-layered", g, dict(variant="min", dtype="f32", schedule="layered", path="flood"), ("layered_kernel",), "f32min", F=70, qc=False, ref="L")
        add(f"{g}-layered-csr-f16", g, dict(variant="min", dtype="f16", schedule="layered"), ("layered_csr_kernel",), "f16L", qc=False)
        add(f"{g}-layered-csr-f32", g, dict(variant="min", dtype="f32", schedule="layered", path="fused"), ("layered_csr_kernel", "float"), "f32min", qc=False, ref="L")
        add(f"{g}-layered-csr-i8", g, dict(variant="min", dtype="i8", schedule="layered"), ("layered_csr_kernel", "signed char"), "i8", qc=False)
        add(f"{g}-layered-csr-ruled-f32", g, dict(variant="min", dtype="f32", schedule="layered", path="fused", **RULE),
            ("layered_csr_kernel", "Ruled<", "float"), "ruled32", qc=False)
        add(f"{g}-layered-csr-ruled-f16", g, dict(variant="min", dtype="f16", schedule="layered", **RULE), ("layered_csr_kernel", "Ruled<"), "ruled16", qc=False)
    w = "rand208"     # N a multiple of 8: layered_csr takes a frame in by 16-byte loads when its buffer is aligned (test_input_paths)
    add(f"{w}-layered-csr-f16", w, dict(variant="min", dtype="f16", schedule="layered"), ("layered_csr_kernel",), "f16L", qc=False)
    add(f"{w}-layered-csr-f32", w, dict(variant="min", dtype="f32", schedule="layered", path="fused"), ("layered_csr_kernel", "float"), "f32min", qc=False, ref="L")
    add(f"{w}-layered-csr-i8", w, dict(variant="min", dtype="i8", schedule="layered"), ("layered_csr_kernel", "signed char"), "i8", qc=False)
    return out


CONTEXTS = _contexts()
CONVERTING = ("f16", "f16L", "pk16", "pk16L", "i8", "ruled16")
PERSISTENT = [cid for cid in CONTEXTS if cid.startswith(("small-2x4-sz32-layered-lds", "moon.7.13-layered-csr", "rand205-fused-csr"))
              and "tanh" not in cid and not cid.endswith("fused-csr-f16")]


def _decoder(hip, monkeypatch, cid, batch=None):
    cx = CONTEXTS[cid]
    for k, v in cx["env"].items():
        monkeypatch.setenv(k, v)
    c = case(cx["code"])
    dec = hip.Decoder(c.code(hip, cx["qc"]), max_batch=batch or cx["F"], **cx["args"])
    for k in cx["env"]:
        monkeypatch.delenv(k)
    assert all(part in dec.kernel_name for part in cx["kernel"]), (cid, dec.kernel_name)
    if cx["kernel"] == ("flood_cn_kernel",):
        assert dec.path == "flood" and "qc" not in dec.kernel_name
    return c, dec


def _final_of_trace(its, conv, trace, channel_lam):
    """the emulations of the flooding schedule return a trace: the LLRs a frame stops with are its row at the turn it stopped"""
    lam = np.array(channel_lam, np.float32)
    for f in np.flatnonzero(conv):
        lam[f] = trace[its[f]][f]
    return lam


def _reference(cx, c, llr):
    """-> bits, iters, converged, final lam (float64, or None where the bar is hard bits and flags)"""
    llr = np.asarray(llr, np.float32)
    n = cx["numerics"]
    with np.errstate(all="ignore"):
        if n == "f16":
            b, i, cv, tr = em.decode_minsum_f16_flood(c.graph, llr, TURNS)
            return b, i, cv, _final_of_trace(i, cv, tr, em.r16(llr)).astype(np.float64)
        if n == "pk16":
            b, i, cv, tr = em.decode_minsum_pk16(c.graph, llr, TURNS)
            return b, i, cv, _final_of_trace(i, cv, tr, -em.neg_llr16(llr).astype(np.float32)).astype(np.float64)
        if n == "pk16L":
            b, i, cv, tr = em.decode_minsum_pk16_layered(c.graph, llr, TURNS)
            return b, i, cv, _final_of_trace(i, cv, tr, -em.neg_llr16(llr).astype(np.float32)).astype(np.float64)
        if n == "f16L":
            b, i, cv, lam = em.decode_minsum_f16_layered(c.graph, llr, TURNS)
            return b, i, cv, lam.astype(np.float64)
        if n == "i8":
            return i8spec.decode_minsum_i8_layered(c.graph, i8spec.quantize(llr, 4.0), TURNS, qscale=4.0)
        if n in ("ruled16", "ruled32"):
            b, i, cv, lam = rulespec.decode_float(c.graph, llr, TURNS, RULE["cn_scale"], RULE["cn_offset"], "f16" if n == "ruled16" else "f32")
            return b, i, cv, lam.astype(np.float64)
    x = llr.astype(np.float64)
    if cx["ref"] == "L":
        b, i, cv = oracle.decode_layered_batch(c.graph, c.layer_ptr, "min", TURNS, x, nthreads=8)
    else:
        b, i, cv = oracle.decode_batch(c.graph, "tanh" if cx["ref"] == "Ft" else "min", TURNS, x, nthreads=8)
    return b, i, cv.astype(bool), None


def _taken_in(cx, llr):
    """hard decisions of the channel LLRs as the context takes them in (a NaN is not > 0 in any format; int8 rounds small values to 0)"""
    if cx["numerics"] == "i8":
        return (i8spec.quantize(llr, 4.0) > 0).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        return (np.asarray(llr) > 0).astype(np.uint8)


def _same(a, b, frames=slice(None), what=""):
    for x, y, name in zip(a, b, ("bits", "iters", "converged", "final lam")):
        if y is None:
            continue
        assert np.array_equal(np.asarray(x)[frames].astype(np.float64), np.asarray(y)[frames].astype(np.float64), equal_nan=True), (what, name)


def _self_consistent(cx, c, llr, out, what):
    """rule 5"""
    bits, its, conv = out[0], out[1], out[2].astype(bool)
    assert c.syndrome_zero(bits[conv]).all(), (what, "a converged frame is not a codeword")
    assert (its[~conv] == TURNS).all(), (what, "a failed frame reports fewer turns than the limit")
    assert np.array_equal(bits[~conv], _taken_in(cx, llr)[~conv]), (what, "a failed frame does not return the channel's decisions")
    if len(out) > 3:
        with np.errstate(invalid="ignore"):
            assert np.array_equal(bits[conv], (out[3][conv] > 0).astype(np.uint8)), (what, "bits are not hard(final lam)")


def _placement(cid, dec, F, kinds, finite):
    """a finite frame shares a lane / a wave / a workgroup / a slab with a poisoned one, by the kernel's own geometry"""
    cx = CONTEXTS[cid]
    bad = np.array(sorted(kinds))
    shares = lambda unit: bool(np.intersect1d(bad // unit, finite // unit).size)
    threads, fpw = dec.kernel_geometry
    onchip_qc = cx["qc"] and any(k in dec.kernel_name for k in ("fused_", "ldpc_jit_"))
    if cx["numerics"] in ("pk16", "pk16L"):
        assert fpw % 2 == 0 and shares(2), (cid, "two frames of one lane (the halves of a packed word)")
    if onchip_qc:
        sz = case(cx["code"]).sz
        cpw = 64 // sz if sz < 64 and sz & (sz - 1) == 0 else 1
        assert fpw == cpw * (2 if "pk16" in cx["numerics"] else 1), (cid, dec.kernel_name, fpw)
        if fpw > 1:
            assert shares(fpw), (cid, "the frames of a workgroup interleave lane by lane: one wave")
    if cx["F"] == 70:
        assert dec.path == "flood" and shares(64) and bool(np.intersect1d(bad[bad >= 64] // 64, finite[finite >= 64] // 64).size), (cid, "a slab of 64 frames")


# ---------------------------------------------------------------------------------------------------------------- CPU: the premises
@pytest.mark.parametrize("name", sorted({cx["code"] for cx in CONTEXTS.values()}))
def test_premises_hold_on_the_oracle(name):
    """the Double oracle decodes every frame a poisoned frame is made from, and both decodes and fails some of the finite frames, in
    both schedules; the poisoned frames are what the docstring says"""
    c = case(name)
    for F in sorted({cx["F"] for cx in CONTEXTS.values() if cx["code"] == name}):
        bad, clean, finite, kinds = c.batch(F)
        x = clean.astype(np.float64)
        for conv in (oracle.decode_batch(c.graph, "min", TURNS, x, nthreads=8)[2].astype(bool),
                     oracle.decode_layered_batch(c.graph, c.layer_ptr, "min", TURNS, x, nthreads=8)[2].astype(bool)):
            assert conv[sorted(kinds)].all(), (name, F, "a poisoned frame's origin does not decode")
            assert conv[finite].any() and not conv[finite].all(), (name, F, int(conv[finite].sum()), len(finite))
        assert set(kinds.values()) == set(POISONS)
        for f, kind in kinds.items():
            nan, inf = np.isnan(bad[f]), np.isinf(bad[f])
            assert (nan.sum(), inf.sum()) == {"nan": (1, 0), "nan_neg": (1, 0), "all_nan": (c.N, 0), "inf_right": (0, 3), "inf_mixed": (0, 2),
                                              "codeword_inf": (0, 1)}[kind], (name, f, kind)
            if kind in ("nan", "nan_neg"):
                assert bool(np.signbit(bad[f][nan])[0]) == (kind == "nan_neg") and clean[f][nan][0] != 0
            if kind == "all_nan":
                assert np.signbit(bad[f]).any() and not np.signbit(bad[f]).all()
            if kind == "codeword_inf":
                with np.errstate(invalid="ignore"):
                    assert c.syndrome_zero((bad[f] > 0)[None])[0] and (np.abs(bad[f][~inf]) == 8).all() and (bad[f][inf] > 0).all()
            if kind == "inf_mixed":
                cols = np.flatnonzero(inf)
                assert any(set(cols) <= set(r) for r in c.rows) and sorted(bad[f][cols]) == [-np.inf, np.inf]
    assert (name != "rand205" or c.N % 8 != 0) and (name != "rand208" or c.N % 8 == 0)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CONTEXTS))
def test_rules_on_poisoned_batches(hip, monkeypatch, cid):
    cx = CONTEXTS[cid]
    c, dec = _decoder(hip, monkeypatch, cid)
    F = cx["F"]
    bad, clean, finite, kinds = c.batch(F)
    poisoned = np.array(sorted(kinds))
    with np.errstate(all="ignore"):
        got = dec.decode_batch(bad.astype(np.float64), TURNS, want_lam=True)
        _placement(cid, dec, F, kinds, finite)                   # (the geometry is that of the launch just made)
        ref = dec.decode_batch(clean.astype(np.float64), TURNS, want_lam=True)
        got32 = dec.decode_batch(bad, TURNS)                     # the float32 entry point: the same answers
    print(f"{cid}: {dec.kernel_name}: poisoned frames converged {got[2][poisoned].tolist()} iters {got[1][poisoned].tolist()}; "
          f"finite frames converged {int(got[2][finite].sum())}/{len(finite)}")
    _same(got32, got[:3], what=(cid, "f32 input against f64 input"))
    # rule 6: the finite frames, bit for bit, against the call without poisoned frames -- and that call against its reference
    _same(got, ref, finite, (cid, "rule 6"))
    want = _reference(cx, c, clean)
    n = cx["numerics"]
    if n == "r16":
        _, d32 = _decoder(hip, monkeypatch, cx["twin"])
        with np.errstate(all="ignore"):
            _same(ref, d32.decode_batch(em.r16(clean).astype(np.float64), TURNS, want_lam=True), what=(cid, "clean frames: f32 fed r16"))
            _same(got, d32.decode_batch(em.r16(bad).astype(np.float64), TURNS, want_lam=True), what=(cid, "rule 1: f32 fed r16"))
        d32.close()
    elif want[3] is None:
        _same(ref, (want[0], None, want[2], None), what=(cid, "clean frames against the Double oracle"))
    else:
        _same(ref, want, what=(cid, "clean frames against the specification"))
    assert ref[2][finite].any() and not ref[2][finite].all()     # the premise, as the device sees it
    # rule 5, everywhere
    _self_consistent(cx, c, bad, got, cid)
    _self_consistent(cx, c, clean, ref, cid)
    # rule 3 / rule 1 on the poisoned frames
    if n in ("f32min", "ruled32"):
        conv = got[2].astype(bool)
        assert np.isfinite(got[3][conv]).all(), (cid, "a converged frame with an LLR that is not finite")
        assert not conv[poisoned].any() and (got[1][poisoned] == TURNS).all(), (cid, got[2][poisoned], got[1][poisoned])
        with np.errstate(invalid="ignore"):
            assert np.array_equal(got[0][poisoned], (bad[poisoned] > 0).astype(np.uint8)), cid
        assert np.array_equal(got[3][poisoned], bad[poisoned].astype(np.float64), equal_nan=True), (cid, "final lam of a failed frame")
    elif n in CONVERTING:
        _same(got, _reference(cx, c, bad), what=(cid, "rule 1: the poisoned batch against the specification"))
        assert np.isfinite(got[3]).all()
    if n in CONVERTING or n == "r16":
        f = next(f for f, k in kinds.items() if k == "codeword_inf")
        assert got[2][f] and got[1][f] == 0, (cid, "a codeword with a saturated +inf converges before the first turn")
        f = next(f for f, k in kinds.items() if k == "all_nan")
        assert got[2][f] and got[1][f] == 0 and not got[0][f].any(), (cid, "all NaN = all erased: the zero word")
    dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CONTEXTS))
def test_input_paths(hip, monkeypatch, cid):
    """the same rules whatever the buffer: fp16 bit patterns 0x7C00 0xFC00 0x7E00 0xFE00 0x7C01 in host and device fp16 buffers, device
    buffers 16-byte aligned and one element past it (the 16-byte and the element-wise loads), 1e300 in a double on an f32 context"""
    import torch
    cx = CONTEXTS[cid]
    n = cx["numerics"]
    F = 13
    c, dec = _decoder(hip, monkeypatch, cid, batch=F)
    bad, clean, finite, kinds = c.batch(F)
    poisoned = np.array(sorted(kinds))
    h = bad.astype(np.float16)
    hv = h.view(np.uint16)
    hv[np.isnan(bad) & ~np.signbit(bad)] = 0x7E00
    hv[np.isnan(bad) & np.signbit(bad)] = 0xFE00
    f = next(f for f, k in kinds.items() if k == "all_nan")
    hv[f, 1::3] = 0x7C01                                          # signalling NaNs among the quiet ones
    assert {0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01} <= set(hv[poisoned].ravel().tolist())
    hc = clean.astype(np.float16)
    with np.errstate(all="ignore"):
        got = dec.decode_batch(h, TURNS)                          # ldpc_decode_batch_f16
        ref = dec.decode_batch(hc, TURNS)
        _same(got, ref, finite, (cid, "rule 6, fp16 input"))
        if n in CONVERTING:
            _same(got, _reference(cx, c, h.astype(np.float32))[:3], what=(cid, "rule 1, fp16 input"))
        elif n in ("f32min", "ruled32"):
            assert not got[2][poisoned].any() and (got[1][poisoned] == TURNS).all(), (cid, "rule 3, fp16 input")
            assert np.array_equal(got[0][poisoned], (h[poisoned] > 0).astype(np.uint8))
        _self_consistent(cx, c, h.astype(np.float32), got, (cid, "fp16 input"))
    # device buffers: element 0 of a fresh allocation is 16-byte aligned, element 1 is not.  Which loads a run takes is the kernel's own
    # `wide` condition and cannot be observed from here; the runs below meet it (shift 0) and break it (shift 1) by construction:
    #   csrc/layered_csr.hip  wide = N % 8 == 0 && llr_fmt != LLR_F64 && !final_lam && (llr + frame offset) % 16 == 0 && (bits + frame
    #                         offset) % 8 == 0 (int8 input: 8-byte alignment)         -> the rand208 contexts, N = 208, f16 / f32 buffers
    #   csrc/layered_lds.hip  the same condition on its frame                          -> small-2x4-sz32 (N = 128), wifi-12x24-sz27 (N = 648)
    # (a change of either condition has to be followed here)
    dev = torch.device("cuda", 0)
    for name, host in (("f16", h), ("f32", bad)):
        want = dec.decode_batch(host, TURNS)
        for shift in (0, 1):
            buf = torch.zeros(F * c.N + 8, dtype=torch.float16 if name == "f16" else torch.float32, device=dev)
            assert buf.data_ptr() % 16 == 0
            view = buf[shift:shift + F * c.N]
            view.copy_(torch.from_numpy(host.reshape(-1).view(np.int16 if name == "f16" else np.int32)).to(dev).view(view.dtype))
            assert view.data_ptr() % 16 == shift * host.itemsize
            bits = torch.full((F + 1, c.N), 9, dtype=torch.uint8, device=dev)
            its = torch.full((F + 1,), -1, dtype=torch.int32, device=dev)
            conv = torch.full((F + 1,), 9, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            dec.decode_batch_dev(view.data_ptr(), bits.data_ptr(), F, TURNS, its.data_ptr(), conv.data_ptr(), None, llr_f16=name == "f16")
            dec.synchronize()
            torch.cuda.synchronize()
            out = (bits.cpu().numpy(), its.cpu().numpy(), conv.cpu().numpy())
            assert (out[0][F] == 9).all() and out[1][F] == -1 and out[2][F] == 9, (cid, name, shift, "a row past the batch was written")
            _same([o[:F] for o in out], want, what=(cid, name, "device buffer, element offset", shift))
    if n in ("f32min", "ruled32", "parity") and cx["args"]["dtype"] == "f32":
        # a double beyond the float range is an infinity once the context holds it: the frame fails (rule 3) / stays consistent (rule 5)
        d = clean.astype(np.float64)
        col = int(np.flatnonzero(clean[1] > 0)[0])
        d[1, col], d[3, col] = 1e300, -1e300
        with np.errstate(all="ignore"):
            out = dec.decode_batch(d, TURNS, want_lam=True)
            base = dec.decode_batch(clean.astype(np.float64), TURNS, want_lam=True)
        rest = np.array([i for i in range(F) if i not in (1, 3)])
        _same(out, base, rest, (cid, "rule 6, doubles beyond the float range"))
        if n != "parity":
            assert not out[2][[1, 3]].any() and (out[1][[1, 3]] == TURNS).all() and out[0][1, col] == 1 and out[0][3, col] == 0, cid
            assert out[3][1, col] > 3.4e38 and out[3][3, col] < -3.4e38
        with np.errstate(over="ignore"):
            _self_consistent(cx, c, d.astype(np.float32), out, (cid, "1e300"))
    dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", PERSISTENT)
def test_a_workgroup_takes_a_finite_frame_after_a_poisoned_one(hip, monkeypatch, cid):
    """the persistent kernels: grid = min(batch, workgroups that can be resident), and a workgroup of at least one wave cannot be
    resident more than 32 times per compute unit (8 waves per SIMD, 4 SIMDs).  Every frame id below that bound is poisoned, the frames
    after it are finite: the grid's own frames are all poisoned, so whichever workgroup takes the first finite frame from the counter
    has just finished a poisoned one.  Rule 6 for the finite frames, rules 1 / 3 and 5 for all."""
    import torch
    cx = CONTEXTS[cid]
    bound = 32 * torch.cuda.get_device_properties(0).multi_processor_count
    F = bound + 13
    c, dec = _decoder(hip, monkeypatch, cid, batch=F)
    assert "fused_csr" not in cid or "fused_csr_batched_kernel" in dec.kernel_name, (cid, dec.kernel_name)   # (the persistent one)
    bad13, clean13, finite13, kinds13 = c.batch(13)
    src = np.array(sorted(kinds13))
    idx = src[np.arange(bound) % len(src)]
    bad = np.concatenate([bad13[idx], clean13[finite13], bad13[src]])            # poisoned x bound, 7 finite, the 6 kinds again
    clean = np.concatenate([clean13[idx], clean13[finite13], clean13[src]])
    assert len(bad) == F and F % 2 == 1
    finite = np.arange(bound, bound + len(finite13))
    assert not np.isfinite(bad[:bound]).all(axis=1).any() and np.isfinite(bad[finite]).all() and not np.isfinite(bad[-1]).all()
    with np.errstate(all="ignore"):
        got = dec.decode_batch(bad.astype(np.float64), TURNS, want_lam=True)
        ref = dec.decode_batch(clean.astype(np.float64), TURNS, want_lam=True)
    _same(got, ref, finite, (cid, "rule 6"))
    small = dec.decode_batch(clean13.astype(np.float64), TURNS, want_lam=True)   # (held to its reference in test_rules_on_poisoned_batches)
    _same([o[finite] for o in ref], [o[finite13] for o in small], what=(cid, "the finite frames as in the batch of 13"))
    # every copy of a poisoned frame gives what the first one gives, and that is what the rules say
    first = {k: int(np.flatnonzero(idx == k)[0]) for k in src}
    for k in src:
        same = np.flatnonzero(idx == k)
        for o in got:
            assert np.array_equal(o[same], np.broadcast_to(o[first[k]], o[same].shape), equal_nan=True), (cid, kinds13[k])
    head = np.array([first[k] for k in src])
    sub = [o[head] for o in got]
    _self_consistent(cx, c, bad[head], sub, cid)
    if cx["numerics"] in ("f32min", "ruled32"):
        assert not sub[2].any() and (sub[1] == TURNS).all() and np.array_equal(sub[3], bad[head].astype(np.float64), equal_nan=True), cid
    else:
        _same(sub, _reference(cx, c, bad[head]), what=(cid, "rule 1"))
    dec.close()


@pytest.mark.gpu
def test_a_nan_gain_in_the_chain_decodes_as_an_erasure(hip):
    """the N = 203, n_tx = 187 source shape of tests/test_fading_gpu.py (29 checks of 7 positions, a random table): ldpc_demap_dev_il_csi
    with a NaN gain writes NaN LLRs for that symbol into an fp16 buffer; fp16-storage contexts decode the buffer as they decode it with
    those LLRs set to 0, and as the emulation does"""
    import torch
    from tests import modulation_spec as ms
    B, m, N, n_tx = 3, 4, 203, 187
    dev = torch.device("cuda", 0)
    rp, ci = np.arange(0, N + 1, 7, dtype=np.int32), np.arange(N, dtype=np.int32)
    code = hip.Code.from_csr(rp, ci, N)
    pts = ms.builtin(ms.QAM16)
    mod = hip.Modulation(pts)
    pos = np.random.default_rng(600 + m).permutation(n_tx).astype(np.int32)
    il = hip.Interleaver(pos, N)
    ns = ms.symbols_per_frame(n_tx, m)
    rng = np.random.default_rng(203)
    sym = (pts[rng.integers(0, len(pts), B * ns)] + rng.normal(0.0, 0.2, (B * ns, 2))).astype(np.float32).reshape(B, ns, 2)
    gain = rng.uniform(0.5, 2.0, (B, ns)).astype(np.float32)
    gain[1, 5] = np.nan
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    llr, sym_t, gain_t = torch.full((B + 1, N), 777.0, dtype=torch.float16, device=dev), put(sym), put(gain)
    torch.cuda.synchronize()
    hip.demap_il_csi(mod, il, B, sym_t.data_ptr(), gain_t.data_ptr(), 0.05, llr.data_ptr(), "f16", 0.0, None)
    torch.cuda.synchronize()
    host = llr.cpu().numpy()
    assert (host[B] == 777.0).all()
    host = host[:B]
    hit = pos[5 * m:6 * m]
    assert np.isnan(host[1, hit]).all() and np.isnan(host).sum() == m
    zeroed = host.copy()
    zeroed[1, hit] = 0
    g = oracle.Graph(rp, ci, N)
    for kw, kernel, emu in ((dict(path="flood"), "flood_cn_kernel", em.decode_minsum_f16_flood),
                            (dict(schedule="layered"), "layered_csr_kernel", em.decode_minsum_f16_layered)):
        dec = hip.Decoder(code, "min", "f16", B, **kw)
        assert kernel in dec.kernel_name, dec.kernel_name
        outs = []
        for buf in (host, zeroed):
            t = put(buf)
            bits = torch.full((B + 1, N), 9, dtype=torch.uint8, device=dev)
            its = torch.full((B + 1,), -1, dtype=torch.int32, device=dev)
            conv = torch.full((B + 1,), 9, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            dec.decode_batch_dev(t.data_ptr(), bits.data_ptr(), B, TURNS, its.data_ptr(), conv.data_ptr(), None, llr_f16=True)
            dec.synchronize()
            torch.cuda.synchronize()
            out = (bits.cpu().numpy(), its.cpu().numpy(), conv.cpu().numpy())
            assert (out[0][B] == 9).all() and out[1][B] == -1 and out[2][B] == 9
            outs.append([o[:B] for o in out])
        _same(outs[0], outs[1], what=(kernel, "NaN LLRs against zeros"))
        _same(outs[0], emu(g, host.astype(np.float32), TURNS)[:3], what=(kernel, "against the emulation"))
        dec.close()
    il.close(); mod.close(); code.close()
