"""CPU: pins the specification tests/test_layered_csr_f32_gpu.py holds the f32-lam instances of csrc/layered_csr.hip to
(tests/layered_f32_spec.py: oracle/emulate_f16.py decode_minsum_f16_layered with a float32 cast in place of its fp16 rounding, and the
non-finite veto on top).  It must be the layered schedule of the Double oracle where float and Double agree, and it must really
leave the float range on the input the GPU test uses for the veto."""
import numpy as np
import pytest

from oracle import emulate_f16 as em
from oracle import oracle
from tests import layered_f32_spec as spec


@pytest.mark.parametrize("name,dbs", spec.ORACLE_CASES)
def test_patched_emulation_is_the_double_oracle(monkeypatch, name, dbs):
    """one row per layer, 25 sweeps, 16 frames per code: flags, sweeps and bits equal (largest |LLR| on these inputs: 27.5 and 30.5)"""
    G = spec._named(name)
    llr = spec.oracle_inputs(G, dbs)
    bits, its, conv, lam, vetoed = spec.emulate(monkeypatch, G, llr, spec.ORACLE_SWEEPS)
    assert not vetoed.any() and np.isfinite(lam).all()
    g = oracle.Graph(G.rp, G.ci, G.N)
    ob, oi, oc = oracle.decode_layered_batch(g, np.arange(G.M + 1, dtype=np.int32), "min", spec.ORACLE_SWEEPS, llr.astype(np.float64))
    assert np.array_equal(conv, oc.astype(bool))
    assert np.array_equal(its, oi)
    assert np.array_equal(bits, ob)


def test_patch_is_undone_and_is_a_cast(monkeypatch):
    x = np.array([1e5, -1e5, 0.1, np.inf], np.float32)
    assert np.array_equal(em.r16(x)[:2], [65504.0, -65504.0])
    with monkeypatch.context() as m:
        m.setattr(em, "r16", spec.f32_cast)
        assert np.array_equal(em.r16(x), x)
    assert np.array_equal(em.r16(x)[:2], [65504.0, -65504.0])


def test_heavy_columns_leave_the_float_range(monkeypatch):
    """codes/1920.1280.A (column weight 18): frames that do not converge multiply their LLRs every sweep; in float they reach inf,
    then NaN, whose hard decisions are an all-zero "codeword" -- the emulation "converges" there, and the veto fails the frame"""
    G = spec._named("1920.1280.A")
    llr = spec.exact_inputs(G, (2.0, 3.0))
    monkeypatch.setattr(em, "r16", spec.f32_cast)
    with np.errstate(over="ignore", invalid="ignore"):
        rbits, rits, rconv, rlam = em.decode_minsum_f16_layered(spec._emu_graph(G), llr, 25)
    nonfinite = ~np.isfinite(rlam).all(axis=1)
    assert (rconv & nonfinite).any()
    bits, its, conv, lam, vetoed = spec.emulate(monkeypatch, G, llr, 25)
    assert np.array_equal(vetoed, rconv & nonfinite) and vetoed.any()
    assert not conv[vetoed].any() and (its[vetoed] == 25).all()
    assert np.array_equal(lam[vetoed], llr[vetoed]) and np.array_equal(bits[vetoed], (llr[vetoed] > 0).astype(np.uint8))
    assert conv[0] and its[0] == 0 and conv[1] and its[1] == 0     # the two planted frames stop before sweep 1
