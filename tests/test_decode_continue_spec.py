"""CPU: tests/decode_continue_spec.py -- from a reset state it IS tests/soft_output_spec.py decode; the chain of three calls the device
test runs (tests/decode_continue_cases.py) meets the conditions that make it a test; a call's new state is what its definition gives and
leaves the other slots alone; the integers of an int8 state stay in their ranges."""
import numpy as np
import pytest

from tests import decode_continue_cases as D
from tests import decode_continue_spec as cspec
from tests import layered_rule_spec as rule_spec
from tests import layered_shapes as S
from tests import soft_output_cases as K
from tests import soft_output_spec as sspec

CASES = [(n, c, r) for n in K.NAMES for c in K.CELLS for r in (False, True)]
IDS = [f"{n}-{c}-{'ruled' if r else 'plain'}" for n, c, r in CASES]


def _same(a, b):
    return a.dtype == b.dtype and np.array_equal(D.bits_of(a), D.bits_of(b))


@pytest.mark.parametrize("name,cell,ruled", CASES, ids=IDS)
def test_from_a_reset_state_it_is_the_soft_decode(name, cell, ruled):
    rule = K.rule_of(name, cell, ruled)
    g, llr = S.case(name), K.frames(name)
    assert not (np.signbit(llr) & (llr == 0)).any()                       # no -0.0 among the LLRs: the one exception of the header
    (bits, sweeps, conv, P, C), st = cspec.call(cell, g, cspec.State(cell, g, len(llr)), llr, K.SWEEPS, rule[0], rule[1], K.QSCALE)
    rb, rs, rc, rP, rC = K.ref(name, cell, rule, K.SWEEPS)
    assert np.array_equal(bits, rb) and np.array_equal(sweeps, rs) and np.array_equal(conv, rc), (name, cell, rule)
    assert _same(P, rP) and _same(C, rC)
    assert _same(st.S, sspec.value(cell, rP, rC, "extrinsic"))            # E, and the state's S is E
    for kind in sspec.KINDS:
        for fmt in sspec.FORMATS:
            assert _same(sspec.soft(cell, P, C, kind, fmt, 0.0, K.QSCALE), sspec.soft(cell, rP, rC, kind, fmt, 0.0, K.QSCALE))


@pytest.mark.parametrize("name,cell,ruled", CASES, ids=IDS)
def test_the_chain_is_a_test(name, cell, ruled):
    rule = K.rule_of(name, cell, ruled)
    (r1, r2, _), _ = D.chain(name, cell, rule)
    (_, s1, c1, _, _), (_, s2, c2, P2, _) = r1, r2
    noisy = slice(0, 8)
    if not ruled:
        # out of sweeps after call 1, converged in call 2 after at least one sweep
        assert (~c1[noisy] & c2[noisy] & (s2[noisy] >= 1)).any(), (name, cell, s1, c1, s2, c2)
        if name in ("w20", "w27"):
            # converged in call 1, stops in call 2 before its first sweep
            assert (c1[noisy] & c2[noisy] & (s2[noisy] == 0)).any(), (name, cell, s1, c1, s2, c2)
    assert (s2[noisy] >= 1).any()
    _, rs, _, rP, _ = D.restarted(name, cell, rule)
    assert ((s2 != rs) | (D.bits_of(P2) != D.bits_of(rP)).any(axis=1)).any(), (name, cell, rule, "a decoder that forgets gives the same")


@pytest.mark.parametrize("name,cell,ruled", CASES, ids=IDS)
def test_the_new_state_and_the_other_slots(name, cell, ruled):
    """call 3 on slots 10 .. 19 of a state of 30: its state is what a fresh evaluation from the same input state gives, S = P - C', a frame
    that ran no sweep keeps its messages, and the slots outside keep theirs"""
    rule = K.rule_of(name, cell, ruled)
    g = S.case(name)
    res, states = D.chain(name, cell, rule)
    llr3, mi3 = D.chain_llrs(name)[2]
    big = cspec.State(cell, g, 30)
    rng = np.random.default_rng(3)
    big.msg[:] = rng.integers(-3, 4, big.msg.shape)                         # something to keep in the other slots
    big.S[:] = rng.integers(-3, 4, big.S.shape)
    big.msg[10:20], big.S[10:20] = states[1].msg, states[1].S
    before = big.copy()
    r3, after = cspec.call(cell, g, big, llr3, mi3, rule[0], rule[1], K.QSCALE, first=10)
    assert _same(big.msg, before.msg) and _same(big.S, before.S)            # the input state is not written
    for got, want in zip(r3, res[2]):
        assert _same(np.asarray(got), np.asarray(want))
    assert _same(after.msg[10:20], states[2].msg) and _same(after.S[10:20], states[2].S)
    assert _same(after.S[10:20], sspec.value(cell, r3[3], r3[4], "extrinsic"))
    for a, b in ((0, 10), (20, 30)):
        assert _same(after.msg[a:b], before.msg[a:b]) and _same(after.S[a:b], before.S[a:b])
    idle = np.flatnonzero(sspec._syndrome_ok(rule_spec._rows(g)[0], cspec.start(cell, r3[4], before.S[10:20])))    # ran no sweep
    assert len(idle) and _same(after.msg[10 + idle], before.msg[10 + idle])
    r3b, again = cspec.call(cell, g, before, llr3, mi3, rule[0], rule[1], K.QSCALE, first=10)
    assert _same(again.msg, after.msg) and _same(again.S, after.S) and all(_same(np.asarray(x), np.asarray(y)) for x, y in zip(r3, r3b))


@pytest.mark.parametrize("name", K.NAMES)
def test_int8_ranges(name):
    for ruled in (False, True):
        rule = K.rule_of(name, "i8", ruled)
        res, states = D.chain(name, "i8", rule)
        prev = cspec.State("i8", S.case(name), 10)
        for (llr, _), (_, _, _, P, C), st in zip(D.chain_llrs(name), res, states):
            lam0 = cspec.start("i8", C, prev.S)
            assert lam0.dtype == np.int32 and np.abs(lam0).max() <= 127 and np.abs(P).max() <= 127
            assert st.S.dtype == np.int32 and np.abs(st.S).max() <= 254
            prev = st
        assert max(np.abs(s.S).max() for s in states) > 127                # the range beyond a cell is used


def test_continuing_instances_exist_and_use_no_scratch():
    """the eighteen layered_csr_cont_kernel instances of the build: no scratch, no spilled VGPR, the heavy-row class at 512 threads"""
    import os
    import re

    from ecc_ldpc_amd import build as B
    path = os.path.join(os.path.dirname(B.__file__), "build", "layered_csr-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), f"no device assembly at {path}: build first (python ecc_ldpc_amd/build.py)"
    text = open(path).read()
    for cell in ("DF16_", "f", "a"):
        for dclass in (8, 20, 32):
            for arg in (cell + "E", "NS_5RuledI%sEEE" % cell):
                m = re.search(r"\.max_flat_workgroup_size:\s+(\d+)\n\s+\.name:\s+_ZN4ldpc23layered_csr_cont_kernelILi%dE%sE\S*\n((?:\s+\.[a-z_]+:.*\n)+)" % (dclass, arg), text)
                assert m, f"layered_csr_cont_kernel<{dclass}, {arg}>: no code-object metadata"
                f = {k: int(v) for k, v in re.findall(r"\.([a-z_]+):\s+(\d+)", m.group(2))}
                assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (dclass, arg, f)
                assert int(m.group(1)) == (512 if dclass == 32 else 1024), (dclass, arg, m.group(1))


def test_max_iters_zero_keeps_the_messages():
    name, cell = "w8", "f16"
    g = S.case(name)
    _, states = D.chain(name, cell, K.PLAIN)
    r, st = cspec.call(cell, g, states[0], D.chain_llrs(name)[1][0], 0)
    assert _same(st.msg, states[0].msg) and (r[1] == 0).all() and _same(r[3], cspec.start(cell, r[4], states[0].S))
    assert _same(st.S, sspec.value(cell, r[3], r[4], "extrinsic"))
