"""(CPU) the headline kernel -- fused_split_kernel<float, min-sum, PlanAR4JA45, 128, TabJpl4096>, what bench.py's `value` measures --
is built spill-free at 4 waves per SIMD: no scratch, no spilled VGPR (csrc/fused_split.hip SPLIT_ORIG_LDS moves part of the round-0
LLR copies to LDS for that).  Read from the code-object metadata of the build's device assembly, the same check build.py makes."""
import os

from ecc_ldpc_amd import build as B

OBJDIR = os.path.join(os.path.dirname(B.__file__), "build")


def test_headline_kernel_spills_nothing():
    res = B.headline_resources(OBJDIR)
    assert res is not None, f"no device assembly in {OBJDIR}: build first (python ecc_ldpc_amd/build.py)"
    assert res["private_segment_fixed_size"] == 0, res
    assert res["vgpr_spill_count"] == 0, res
    assert res["vgpr_count"] <= 128, res   # 4 waves per SIMD: 512 VGPRs / 4
