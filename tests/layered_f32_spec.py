"""The specification of the f32-lam instances of csrc/layered_csr.hip, shared by tests/test_layered_f32_emulation.py (CPU) and
tests/test_layered_csr_f32_gpu.py: oracle/emulate_f16.py decode_minsum_f16_layered with its rounding r16 replaced by a plain float32
cast (the same IEEE operations in the same order, nothing rounded to fp16, nothing saturated), and the non-finite veto of
csrc/ldpc_math.h kVetoesNonFinite on top: a frame whose LLRs left the float range is failed, never "converged".

Graphs and frames are those of tests/test_layered_csr_gpu.py (the all-zero codeword + noise)."""
import numpy as np

from oracle import emulate_f16 as em
# the graphs and frames ARE those of the fp16 test: taken from its module, which is left as it is (importing it touches no GPU -- its
# tests get the library through the `hip` fixture -- so the CPU test may use this module too)
from tests.test_layered_csr_gpu import Graph, _emu_graph, _named   # noqa: F401  (re-exported)


def f32_cast(x):
    """what stands in for emulate_f16.r16: a lam cell holds the float as it is"""
    return np.asarray(x, np.float32)


def random_irregular(M=300, N=40001, seed=11):
    """rows of weight 2..14, mixed inside every layer; N not a multiple of 8, 160 004 B of f32 LLRs (160 048 B of LDS with the
    control words): one workgroup per CU"""
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(N, int(rng.integers(2, 15)), replace=False)) for _ in range(M)]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return Graph(rp, np.concatenate(rows).astype(np.int32), N, N - M)


def emulate(monkeypatch, G, llr, max_iters):
    """-> bits, sweeps, converged, lam [F, N] float32, vetoed [F]: the patched emulation with the veto applied.  monkeypatch undoes
    the replacement of r16 when the calling test ends."""
    monkeypatch.setattr(em, "r16", f32_cast)
    llr = np.asarray(llr, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        bits, its, conv, lam = em.decode_minsum_f16_layered(_emu_graph(G), llr, max_iters)
    vetoed = conv & ~np.isfinite(lam).all(axis=1)
    bits, its, conv, lam = bits.copy(), its.copy(), conv.copy(), lam.copy()
    conv[vetoed] = False
    its[vetoed] = max_iters
    lam[vetoed] = llr[vetoed]
    bits[vetoed] = (llr[vetoed] > 0).astype(np.uint8)
    return bits, its, conv, lam, vetoed


def exact_inputs(G, dbs, F=8):
    """the frames of the bit-exactness tests: F / 2 per Eb/N0 point with seeds 100 and 101, frame 0 all-zero LLRs (the syndrome is
    zero before sweep 1), frame 1 the noiseless all-zero codeword"""
    llr = np.concatenate([G.frames(F // 2, db, 100 + i) for i, db in enumerate(dbs)])
    llr[0] = 0.0
    llr[1] = -6.0
    return llr


def oracle_inputs(G, dbs):
    """the 16 frames per code compared with the Double oracle: 8 per Eb/N0 point, seeds 100 and 101"""
    return np.concatenate([G.frames(8, db, 100 + i) for i, db in enumerate(dbs)])


ORACLE_CASES = [("moon.7.13", (1.0, 3.0)), ("1920.1280.3.303", (1.5, 2.5))]
ORACLE_SWEEPS = 25
