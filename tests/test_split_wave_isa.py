"""(CPU) static instruction count of the headline kernel -- fused_split_kernel<float, min-sum, PlanAR4JA45, 128, TabJpl4096> -- from
ecc_ldpc_amd/build/isa_stats.json (tools/isa_histogram.py over the build's own device assembly).

The kernel runs one straight-line program per WAVE of a frame (csrc/fused_split_body.h SPLIT_WAVE_SPEC): NP x 2 = 4 turn loops where
the parent commit had NP = 2.  Each must need fewer VALU issue clocks per hot turn than the parent's programs did, and none may touch
scratch memory.

hot-turn valu_cost_weighted_clk (VALU instructions), same tool, same flags:
  parent commit (one program per pair):   2 881.4 (955)   2 883.4 (957)
  this tree (pair 0 wave 0 / 1, pair 1 wave 0 / 1):   2 603.4 (895)   2 627.4 (907)   2 621.4 (904)   2 625.4 (906)
  (the wave's own rotations in phase A only, SPLIT_WAVE_PHASES = 1; in both phases: 2 473.4 (831) 2 521.4 (855) 2 511.4 (849) 2 513.4 (850))
  of the parent's 233 / 236 address instructions (v_and_b32 + v_add_u32 + v_mov_b32) 177 / 189 / 186 / 188 are left, and the
  158 / 159 v_cmp of the syndrome are 80 / 80 / 81 / 81 (lam stored negated: one v_xor per edge, one test per row).
"""
import json
import os

from ecc_ldpc_amd import build as B

STATS = os.path.join(os.path.dirname(B.__file__), "build", "isa_stats.json")
HEADLINE = "ldpc::fused_split_kernel<float, 1, ldpc::PlanAR4JA45, 128, ldpc::TabJpl4096>"
PARENT_CLK = (2881.4, 2883.4)     # the parent commit's two programs
NP, WAVES_PER_PAIR = 2, 2


def _headline():
    assert os.path.exists(STATS), f"{STATS}: build first (python ecc_ldpc_amd/build.py)"
    hits = [k for k in json.load(open(STATS)) if HEADLINE in k["kernel"] and k["source"].startswith("fused_split-")]
    assert len(hits) == 1, [k["kernel"] for k in hits]
    return hits[0]


def test_one_turn_loop_per_wave():
    loops = _headline()["loops"]
    assert len(loops) == NP * WAVES_PER_PAIR, [lp["header"] for lp in loops]
    assert not any(lp["inner_loops"] for lp in loops)


def test_every_program_needs_fewer_valu_clocks_than_the_parents():
    for lp in _headline()["loops"]:
        clk = lp["hot_turn"]["valu_cost_weighted_clk"]
        print(lp["header"], lp["instructions"], "instructions;", "hot turn:", lp["hot_turn"]["units"], clk, "clk")
        assert clk < min(PARENT_CLK), (lp["header"], clk)


def test_no_scratch_instruction_in_any_turn_loop():
    for lp in _headline()["loops"]:
        for part in ("hot_turn", "every_turn", "whole_loop"):
            assert lp[part]["units"].get("spill", 0) == 0, (lp["header"], part, lp[part]["units"])
            assert not any(m.startswith("scratch_") for m in lp[part].get("mnemonics", {})), (lp["header"], part)
