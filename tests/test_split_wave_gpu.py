"""The wave-specialised split kernel (csrc/fused_split_body.h SPLIT_WAVE_SPEC / SPLIT_FLAGS_LDS / SPLIT_NEG_LAM: one program per wave,
rotation wrap as an immediate, syndrome words as LDS accesses, optionally lam stored negated with a sign-bit syndrome) on the headline
context -- jpl.4096.4.5, f32 min-sum -- held to the bars tests/test_fused_gpu.py holds this kernel to against the CPU oracle
(hard bits and flags exact, iteration counts by helpers.iters_agree, a teacher-forced turn within 1e-5 * max(1, |x|)), and EQUAL to the
kernel families the change does not touch -- flood_qc_kernel from HBM and the two-wave fused_msg kernel, which do the same float
arithmetic in the same order -- in bits, iteration counts, flags, final lam, the per-turn trace and teacher-forced steps.

The frames are chosen to hit what such a change can break:
  (a) channel LLRs that are exactly +0.0 and -0.0: the punctured columns as -0.0, zeros of both signs sprinkled over a frame, a frame of
      all +0.0 and one of all -0.0  (a zero must count as "not > 0" whatever its sign, also when lam is stored as 0 - lam);
  (b) frames on a half-integer grid, where every sum of the first turns is exact and in turns 2..4 some columns' lam cancels to
      exactly zero although messages that are not zero arrive there (the CPU test below proves that premise on the oracle's trace);
  (c) a batch of 61 frames: a multiple of nothing the host or the kernel chunks by;
  (d) teacher-forced steps whose given lam holds zeros of both signs;
  (e) LLRs large enough to leave the float range in the first update (non-finite veto: such a frame fails, it never "converges"),
      and infinite channel LLRs (inf - inf = NaN in the first turn).
"""
import numpy as np
import pytest

from oracle import oracle
from tests.helpers import load, iters_agree

NAME = "jpl.4096.4.5"
TURNS = 50


def _random(c):
    return np.concatenate([c.frames(6, db, 6200 + i)[1] for i, db in enumerate((2.0, 3.0, 3.6))]).astype(np.float32).astype(np.float64)


def _zeros(c):
    """(a) -> 8 frames"""
    cws, llr = c.frames(6, 3.2, seed=6300)
    llr = llr.astype(np.float32).astype(np.float64)
    punct = llr[0] == 0
    assert punct.sum() == c.N - c.n_tx and not np.signbit(llr[0][punct]).any()    # the channel leaves +0.0 in the punctured columns
    rng = np.random.default_rng(6301)
    llr[0][punct] = -0.0
    llr[1][punct] = -0.0
    for f in (1, 2, 3):     # zeros of both signs in transmitted columns
        at = rng.choice(c.n_tx, 300, replace=False)
        llr[f][at[:150]] = 0.0
        llr[f][at[150:]] = -0.0
    return np.concatenate([llr, np.zeros((1, c.N)), np.full((1, c.N), -0.0)])


def _grid(c):
    """(b) -> 12 frames on a half-integer grid, |LLR| <= 8 (small negative values round to -0.0)"""
    _, llr = c.frames(12, 3.0, seed=6100)
    return np.clip(np.round(llr * 2) / 2, -8, 8)


def _huge(c):
    """(e) -> 4 frames: a codeword at +-3e38 with 1 / 40 small wrong-signed entries (first update: 3e38 + 0.75 * 3e38 * ... = inf);
    a noisy frame with some channel LLRs at +-inf; a noisy frame at +-1e38 scale"""
    cws, llr = c.frames(4, 3.0, seed=6400)
    llr = llr.astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(6401)
    out = []
    for f, nbad in ((0, 1), (1, 40)):
        x = (2.0 * cws[f] - 1.0) * 3e38
        x[c.n_tx:] = 0.0
        bad = rng.choice(c.n_tx, nbad, replace=False)
        x[bad] = -np.sign(x[bad]) * 0.5
        out.append(x)
    x = llr[2].copy()
    at = rng.choice(c.n_tx, 6, replace=False)
    x[at[:3]] = np.inf
    x[at[3:]] = -np.inf
    out.append(x)
    out.append(np.clip(llr[3] * 1e37, -3e38, 3e38))
    return np.stack(out).astype(np.float32).astype(np.float64)


def _finite_batch(c):
    """(a) + (b) + random frames: 8 + 12 + 18 = 38 frames"""
    return np.concatenate([_zeros(c), _grid(c), _random(c)])


def test_premises_hold_on_the_oracle():
    """(CPU) the frames are what the docstring says: -0.0 and +0.0 among the channel LLRs; on the grid frames a column with a nonzero
    receiving nonzero messages has lam == 0 exactly in some turn >= 1; every frame of (a) and (b) is exactly representable in f32."""
    c = load(NAME)
    z, g = _zeros(c), _grid(c)
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z) and np.array_equal(g.astype(np.float32).astype(np.float64), g)
    for x in (z, g):
        zero = x == 0
        assert (zero & np.signbit(x)).any() and (zero & ~np.signbit(x)).any()
    cancelled = 0
    for f in range(4):
        o = oracle.decode(c.graph, "min", TURNS, g[f], trace=True)
        for n in range(1, min(5, o["iters"] + 1)):
            arriving = np.zeros(c.N)
            np.add.at(arriving, c.graph.col_idx, (o["trace_ne"][n - 1] != 0).astype(float))
            cancelled += int(((o["trace_lam"][n] == 0) & (arriving > 0)).sum())
    assert cancelled >= 20, cancelled
    o = oracle.decode(c.graph, "min", TURNS, z[6])     # all zeros: hard(0) = 0 everywhere, a codeword: converged before any turn
    assert o["converged"] and o["iters"] == 0 and not o["bits"].any()


def _split(hip, code, batch):
    dec = hip.Decoder(code, "min", "f32", batch, path="fused")
    assert "fused_split_kernel" in dec.kernel_name, dec.kernel_name
    return dec


@pytest.mark.gpu
def test_bits_iters_flags_against_oracle_flood_and_two_wave_kernel(hip, monkeypatch):
    c = load(NAME)
    llr = np.concatenate([_finite_batch(c), _random(c)[::-1], _grid(c)[:5]])     # 38 + 18 + 5 = 61 frames (c)
    assert len(llr) == 61
    code = c.hip_code(hip)
    l32 = llr.astype(np.float32)
    a = _split(hip, code, len(llr)).decode_batch(l32, TURNS)
    ob, oi, oc = oracle.decode_batch(c.graph, "min", TURNS, llr, nthreads=8)
    print(f"split vs oracle: {int((a[1] != oi).sum())} of {len(llr)} iteration counts differ; converged {int(a[2].sum())}; turns {sorted(set(a[1].tolist()))}")
    assert np.array_equal(a[0], ob) and np.array_equal(a[2], oc)
    assert iters_agree(a[1], oi)
    b = hip.Decoder(code, "min", "f32", len(llr), path="flood").decode_batch(l32, TURNS)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    monkeypatch.setenv("LDPC_FUSED_KERNEL", "msg")
    m = hip.Decoder(code, "min", "f32", len(llr), path="fused")
    assert "fused_split_kernel" not in m.kernel_name, m.kernel_name
    m = m.decode_batch(l32, TURNS)
    monkeypatch.delenv("LDPC_FUSED_KERNEL")
    assert all(np.array_equal(x, y) for x, y in zip(a, m))
    # a short first chunk and one frame at a time: the same answers
    d = _split(hip, code, 7)
    for f in (0, 6, 7, 20, 60):
        b1, it1, cv1 = d.decode_one(llr[f], TURNS)
        assert np.array_equal(b1, a[0][f]) and it1 == a[1][f] and bool(cv1) == bool(a[2][f]), f
    few = d.decode_batch(l32[3:10], 3)              # frames cut off after 3 turns: hard(channel LLR), not converged
    fl = hip.Decoder(code, "min", "f32", 7, path="flood").decode_batch(l32[3:10], 3)
    assert all(np.array_equal(x, y) for x, y in zip(few, fl))


@pytest.mark.gpu
def test_final_lam_and_trace_equal_the_flood_kernel(hip):
    c = load(NAME)
    llr = np.concatenate([_zeros(c), _grid(c)[:6], _random(c)[::4]])     # 8 + 6 + 5 = 19 frames
    code = c.hip_code(hip)
    s, fl = _split(hip, code, len(llr)), hip.Decoder(code, "min", "f32", len(llr), path="flood")
    a = s.decode_batch(llr, TURNS, want_lam=True)
    b = fl.decode_batch(llr, TURNS, want_lam=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    ta = s.decode_trace(llr, 20)
    tb = fl.decode_trace(llr, 20)
    assert all(np.array_equal(x, y) for x, y in zip(ta, tb))
    # against the oracle: on the grid frames every value of turns 0..3 is a multiple of 0.5 * (3/4)^3 = 27/128 below 2^9 -- 16 bits,
    # so the float sums are as exact as the Double ones
    for f in range(8, 14):
        o = oracle.decode(c.graph, "min", 20, llr[f], trace=True)
        n = min(3, o["iters"])
        assert np.array_equal(ta[3][f, : n + 1], o["trace_lam"][: n + 1]), f
    # a converged frame's final lam is its trace at the turn it stopped
    for f in np.flatnonzero(ta[2]):
        if a[2][f] and a[1][f] <= 20:
            assert np.array_equal(a[3][f], ta[3][f, a[1][f]]), f


@pytest.mark.gpu
def test_teacher_forced_steps_with_zeros_in_the_given_lam(hip):
    """(d) states from the oracle's own trajectories of the zero-laden and the grid frames; the lam given to the kernel holds +0.0
    and -0.0 (asserted).  Bar against the oracle as in tests/test_fused_gpu.py: 1e-5 * max(1, |x|) on the new messages and the new lam,
    syndrome flag exact; and equal to the flood kernel's step."""
    c = load(NAME)
    frames = np.concatenate([_zeros(c)[:4], _grid(c)[:4]])
    states = []
    for x in frames:
        o = oracle.decode(c.graph, "min", TURNS, x, trace=True)
        ne = np.zeros(c.E)
        for n in range(min(o["iters"], 4)):
            states.append((x, o["trace_lam"][n], ne, o["trace_ne"][n], o["trace_lam"][n + 1]))
            ne = o["trace_ne"][n]
    lam_in = np.stack([s[1] for s in states])
    assert ((lam_in == 0) & np.signbit(lam_in)).any() and ((lam_in == 0) & ~np.signbit(lam_in)).any()
    # two hand-made states: lam all zero of either sign with zero messages -> syndrome satisfied (hard(0) = 0), lam' = channel LLR
    for z in (0.0, -0.0):
        states.append((frames[0], np.full(c.N, z), np.zeros(c.E), None, None))
    code = c.hip_code(hip)
    s, fl = _split(hip, code, 64), hip.Decoder(code, "min", "f32", 64, path="flood")
    args = [np.stack([st[i] for st in states]) for i in range(3)]
    ne2, lam2, syn = s.debug_step(*args)
    ne2f, lam2f, synf = fl.debug_step(*args)
    assert np.array_equal(ne2, ne2f) and np.array_equal(lam2, lam2f) and np.array_equal(syn, synf)
    assert not syn[:-2].any() and syn[-2:].all()
    assert not ne2[-2:].any() and np.array_equal(lam2[-2:], np.stack([frames[0]] * 2).astype(np.float32).astype(np.float64))
    worst = 0.0
    for i, st in enumerate(states[:-2]):
        assert (np.abs(ne2[i] - st[3]) <= 1e-5 * np.maximum(1, np.abs(st[3]))).all(), i
        err = np.abs(lam2[i] - st[4]) / np.maximum(1, np.abs(st[4]))
        worst = max(worst, err.max())
        assert err.max() <= 1e-5, (i, err.max())
    print(f"split, zero-laden states: worst teacher-forced relative LLR error {worst:.3e} over {len(states) - 2} turns")


@pytest.mark.gpu
def test_llrs_beyond_the_float_range_fail_and_equal_the_flood_kernel(hip):
    """(e) ldpc_math.h kVetoesNonFinite: a frame whose LLRs are not finite when its syndrome reads zero comes back failed -- the
    channel's hard decisions, iters = max, flag clear -- never converged; the frames around it are not disturbed."""
    c = load(NAME)
    huge, rnd = _huge(c), _random(c)[6:12]
    llr = np.concatenate([rnd[:3], huge, rnd[3:]])
    l32 = llr.astype(np.float32)
    code = c.hip_code(hip)
    with np.errstate(all="ignore"):
        a = _split(hip, code, len(llr)).decode_batch(l32, TURNS)
        b = hip.Decoder(code, "min", "f32", len(llr), path="flood").decode_batch(l32, TURNS)
        lam = _split(hip, code, len(llr)).decode_batch(llr, TURNS, want_lam=True)[3]
    print("huge frames: iters", a[1][3:7].tolist(), "converged", a[2][3:7].tolist())
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    conv = a[2].astype(bool)
    assert np.isfinite(lam[conv]).all()         # THE bar: whatever comes back converged has finite LLRs
    f = 5                                       # infinite channel LLRs stay non-finite in every turn: this frame can only fail
    assert not a[2][f] and a[1][f] == TURNS and np.array_equal(a[0][f], (l32[f] > 0).astype(np.uint8))
    ob, oi, oc = oracle.decode_batch(c.graph, "min", TURNS, rnd, nthreads=6)
    keep = [0, 1, 2, 7, 8, 9]
    assert np.array_equal(a[0][keep], ob) and np.array_equal(a[2][keep], oc) and iters_agree(a[1][keep], oi)
