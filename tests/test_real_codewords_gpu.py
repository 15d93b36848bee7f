"""GPU: every kernel family decodes REAL codewords, and every min-sum (and f32 tanh) context is symmetric under them.

Before this module the decode tests of most families saw the all-zero codeword only (tests/helpers.py SyntheticQC.frames and
LoadedCode.frames for the codes without a generator, tests/layered_shapes.py, tests/test_layered_csr_gpu.py, ...).  With that word and
hard(x) = x > 0 a converged frame's output is all zeros -- right for any bit written to the wrong place, any bit order of a packed
result, any stop rule that reads the wrong columns -- and nearly every lam - ne is negative, so sign and parity code runs on half of its
inputs.  Here: one case per family and context (tests/real_codeword_cases.py), 8 noisy frames of random codewords at two Eb/N0 (4 on the
two long codes) plus a noiseless codeword at +-8 and its mirror image, 25 turns.  tests/test_codewords.py asserts on the CPU what this rests on.

Each case asserts
  * the kernel it ran (kernel_name) and that its reference has both kinds of frame: one converging after several turns, one running out;
  * the bar its family's own test file holds, unchanged: bit for bit against the emulation or specification where one exists (fp16
    storage, packed fp16, the layered min-sum kernels in fp16, f32 and int8 cells, with and without a rule; int8 also from native int8
    input); the Double oracle's whole trajectory and final_lam for the f64 contexts (min: bit for bit; tanh: as tests/test_flood_gpu.py, to
    the last places of the device's libm); for f32 against the Double oracle hard bits and flags exact, turn counts within
    helpers.iters_agree, and one teacher-forced debug_step from the oracle's states of THESE frames within helpers.lam_tolerance (min: 1e-5
    relative, no allowance) where the family has the step; the f32 pairs their own tests hold equal (on-chip = flood path, on-chip
    layered = HBM layered, any-H layered = flood.hip layered) equal here too;
  * ldpc_decode_batch_dev_packed on the same frames = the byte result packed LSB first (tests/test_launch_limits_gpu.py pack_rows), the row
    past the batch untouched;
  * the symmetry: the mirror images (LLRs negated where the codeword is 1) stop at the same turn with the same flag, return final_lam negated
    at those positions bit for bit and the bits XOR the codeword wherever final_lam != 0.  Negation commutes with every IEEE rounding and
    min and |.| do not see it; the f32 tanh rules compute on |t| and read the sign off the sign bit.  An f64 tanh context follows the
    reference's formula, which is not odd in floating point: bits, flags and turn counts equal, final_lam within helpers.lam_tolerance.

Measured on MI355X: DESIGN.md section 2."""
import numpy as np
import pytest

from oracle import oracle
from tests import codewords as cwm
from tests import layered_rule_spec as spec
from tests import real_codeword_cases as R
from tests.helpers import iters_agree, lam_tolerance

pytestmark = pytest.mark.gpu

T = R.TURNS
# the switches that choose a rung of the ladder: a case sets the ones it names, none of the others is inherited from the environment
SWITCHES = ("LDPC_FUSED_KERNEL", "LDPC_FUSED_TABLE", "LDPC_JIT", "LDPC_LAYERED_LDS", "LDPC_LAYERED_CSR_THREADS", "LDPC_LAYERED_QC", "LDPC_FLOOD_QC",
            "LDPC_LAYERED_FUSED", "LDPC_LAYERED_RECORDS", "LDPC_LAYERED_CSR", "LDPC_CSR_BATCHED")


def _ran(dec, want, what):
    name = dec.kernel_name
    for w in want:
        assert name.startswith(w) if w.startswith("ldpc_jit") else w in name, (what, name, want)


def _same(got, ref, what, n):
    assert np.array_equal(got[1], ref[1]), (what, "turns", got[1], ref[1])
    assert np.array_equal(np.asarray(got[2], bool), np.asarray(ref[2], bool)), (what, "flags")
    assert np.array_equal(got[0], ref[0]), (what, "bits", np.flatnonzero((got[0] != ref[0]).any(axis=1)))
    if n == 4:
        assert np.array_equal(got[3], ref[3]), (what, "final_lam", np.flatnonzero((got[3] != ref[3]).any(axis=1)))


def _tanh_f64_tolerance(o):
    """tests/test_flood_gpu.py test_tanh_f64_trajectory: relative, while the oracle's own conditioning allows a tight bound"""
    ne_max = np.abs(o["trace_ne"]).max() if o["iters"] else 0.0
    return 1e-11 * (1 + np.exp(min(ne_max, 36)) * 2.0 ** -30)


def _against_the_reference(dec, case, c, llr, ref, got):
    what = case.id
    if case.ref in ("oracle", "oracle-layered") and case.dtype == "f64":
        bits, its, conv, trace = dec.decode_trace(llr, T)
        _same((bits, its, conv), ref, what, 3)
        _same(got, ref, what, 4 if case.variant == "min" else 3)
        for f, o in enumerate(ref[4]):
            if case.variant == "min":
                assert np.array_equal(trace[f, : o["iters"] + 1], o["trace_lam"]), (what, f)
            else:
                tol = _tanh_f64_tolerance(o)
                for x, want in ((trace[f, : o["iters"] + 1], o["trace_lam"]), (got[3][f], ref[3][f])):
                    err = np.abs(x - want) / np.maximum(1, np.abs(want))
                    assert err.max() <= tol, (what, f, err.max(), tol)
    elif case.ref == "oracle":                                  # f32 against the Double oracle
        assert np.array_equal(got[0], ref[0]), (what, np.flatnonzero((got[0] != ref[0]).any(axis=1)))
        assert np.array_equal(got[2].astype(bool), ref[2]), what
        assert iters_agree(got[1], ref[1]), (what, got[1], ref[1])
    elif case.ref in ("f16-flood", "pk16", "pk16-layered"):     # the emulations with a trajectory
        bits, its, conv, trace = dec.decode_trace(llr, T)
        _same((bits, its, conv), ref, what, 3)
        _same(got, ref, what, 3 if case.ref == "f16-flood" else 4)
        for n, lam in enumerate(ref[4]):
            live = np.ones(len(llr), bool) if case.ref == "f16-flood" else n <= (ref[1] if case.ref == "pk16" else np.where(ref[2], ref[1], T))
            assert np.isfinite(lam[live]).all()
            assert np.array_equal(trace[live, n, :], lam[live].astype(np.float64)), (what, n)
    else:                                                       # f16-layered, (spec, cell): bits, sweeps, flags, final_lam
        _same(got, ref, what, 4)
    # the throughput entry point: f32 LLRs in, no LLRs out
    l32 = llr.astype(np.float32)
    _same(dec.decode_batch(l32, T), got, (what, "f32 in"), 3)
    if case.native_i8:
        assert dec.qscale == 4.0
        _same(dec.decode_batch(spec.quantize(l32, 4.0).astype(np.int8), T), got, (what, "int8 in"), 3)


def _packed(hip, dec, case, llr, got):
    """ldpc_decode_batch_dev_packed: bit i of a frame is bit i % 8 of byte i // 8 (include/ldpc_hip.h)"""
    import torch
    from tests.test_launch_limits_gpu import Dev, pack_rows
    d = Dev()
    F, N = llr.shape
    PB = (N + 7) // 8
    x = torch.from_numpy(llr.astype(np.float32)).to(d.dev)
    out, its, conv = d.full(F, PB, 0xA5, d.u8), d.full(F, 1, -1, d.i32), d.full(F, 1, 9, d.u8)
    d.sync()
    dec.decode_batch_dev_packed(x.data_ptr(), out.data_ptr(), F, T, its.data_ptr(), conv.data_ptr(), None)
    dec.synchronize()
    d.sync()
    want = pack_rows(d, torch.from_numpy(np.ascontiguousarray(got[0])).to(d.dev), PB)
    assert torch.equal(out[:F], want), (case.id, "packed bits are not the bytes packed")
    assert bool((out[F] == 0xA5).all()) and int(its[F, 0]) == -1 and int(conv[F, 0]) == 9, (case.id, "the row past the batch was written")
    assert np.array_equal(its[:F, 0].cpu().numpy(), got[1]) and np.array_equal(conv[:F, 0].cpu().numpy().astype(bool), got[2].astype(bool)), case.id
    assert np.array_equal(out[:F].cpu().numpy(), np.packbits(got[0], axis=1, bitorder="little"))          # (and the helper is numpy's little order)


def _symmetry(dec, case, c, llr, cws, ref, got):
    mir = dec.decode_batch(cwm.flip(llr, cws), T, want_lam=True)
    what = (case.id, "mirror images")
    assert np.array_equal(mir[1], got[1]), (what, "turns", mir[1], got[1])
    assert np.array_equal(mir[2], got[2]), (what, "flags")
    if case.sym == "loose":
        assert np.array_equal(mir[0], got[0] ^ cws), what
        for f, o in enumerate(ref[4]):
            ne = o["trace_ne"][-1] if o["iters"] else np.zeros(c.E)
            tol, _ = lam_tolerance(c.graph, ne, ref[3][f])
            assert (np.abs(mir[3][f] - cwm.flip(got[3][f], cws[f])) <= tol).all(), (what, f)
        return
    assert np.array_equal(mir[3], cwm.flip(got[3], cws)), (what, "final_lam", np.flatnonzero((mir[3] != cwm.flip(got[3], cws)).any(axis=1)))
    decided = got[3] != 0
    assert np.array_equal(mir[0][decided], (got[0] ^ cws)[decided]), (what, "bits")
    assert decided.mean() > 0.9


def _teacher_forced(dec, case, c, llr, ref, cap):
    """one debug_step from oracle states of these frames: the last turn of every frame that has one, then first turns, up to the batch"""
    states = []
    if case.step == "flood":
        traces = ref[4]
        for pick in (-1, 0):
            for f, o in enumerate(traces):
                if o["iters"] > (0 if pick == -1 else 1):
                    n = o["iters"] - 1 if pick == -1 else 0
                    states.append((llr[f], o["trace_lam"][n], o["trace_ne"][n - 1] if n else np.zeros(c.E), o["trace_ne"][n], o["trace_lam"][n + 1]))
    else:
        for f in range(case.F):
            lam, msg = llr[f].copy(), np.zeros(c.E)
            for n in range(3):
                m2, l2, _, _ = oracle.layered_step(c.graph, case.variant, lam, msg)
                states.append((llr[f], lam, msg, m2, l2))
                lam, msg = l2, m2
    states = states[:cap]
    assert len(states) >= 4
    ne2, lam2, _ = dec.debug_step(np.stack([s[0] for s in states]), np.stack([s[1] for s in states]), np.stack([s[2] for s in states]))
    worst = 0.0
    for i, s in enumerate(states):
        tol_lam, tol_ne = lam_tolerance(c.graph, s[3], s[4])
        if case.variant == "min":                                # no transcendental: no oracle-conditioning allowance
            tol_lam, tol_ne = 1e-5 * np.maximum(1, np.abs(s[4])), 1e-5 * np.maximum(1, np.abs(s[3]))
        assert (np.abs(ne2[i] - s[3]) <= tol_ne).all(), (case.id, i, np.abs(ne2[i] - s[3]).max())
        assert (np.abs(lam2[i] - s[4]) <= tol_lam).all(), (case.id, i, np.abs(lam2[i] - s[4]).max())
        worst = max(worst, (np.abs(lam2[i] - s[4]) / np.maximum(1, np.abs(s[4]))).max())
    return worst, len(states)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_real_codewords(hip, monkeypatch, case):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    c = R.code(case.code)
    llr, cws = R.frames_of(case)
    ref = R.reference_of(case)
    assert R.exercised(case, ref), (case.id, ref[1], ref[2])
    F = len(llr)
    kw = case.decoder_kw()
    dec = hip.Decoder(c.hip_code(hip, case.qc), max_batch=F, **kw)
    got = dec.decode_batch(llr, T, want_lam=True)
    _ran(dec, case.kernel, case.id)
    assert dec.schedule == case.schedule and (case.path == "auto" or dec.path == case.path), (case.id, dec.path, dec.schedule)
    if case.rule:
        assert (dec.cn_scale, dec.cn_offset) == case.rule
    _against_the_reference(dec, case, c, llr, ref, got)
    assert np.array_equal(got[0][case.F], cws[case.F]) and not got[0][case.F + 1].any()            # the noiseless word and its mirror image
    if R.DEGENERATE.get(case.code) != 0 and not case.stuck:     # converged frames whose bits hold ones: what the zero word cannot show
        assert got[0][:case.F][got[2][:case.F].astype(bool)].any() and got[0][case.F].any()
    _packed(hip, dec, case, llr, got)
    _symmetry(dec, case, c, llr, cws, ref, got)
    note = ""
    if case.pair:
        over, env, kernel, n = case.pair
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        other = hip.Decoder(c.hip_code(hip, case.qc), max_batch=F, **{**kw, **over})
        out = other.decode_batch(llr, T, want_lam=True)
        _ran(other, kernel, (case.id, "pair"))
        assert other.kernel_name != dec.kernel_name
        _same(out, got, (case.id, "pair", other.kernel_name), n)
        other.close()
    if case.step:
        worst, count = _teacher_forced(dec, case, c, llr, ref, F)
        note = f", worst teacher-forced relative LLR error {worst:.2e} over {count} states"
    print(f"{case.id}: {dec.kernel_name} {int(got[2][:case.F].sum())}/{case.F} noisy frames converged, turns {got[1].tolist()}{note}")
    dec.close()
