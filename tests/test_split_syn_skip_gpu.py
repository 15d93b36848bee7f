"""The syndrome skip of the headline kernel (csrc/fused_split_body.h SPLIT_SYN_SKIP = K): in an ordinary turn a wave that has seen an
unsatisfied row among its group's first K block rows branches around the parity chains of the group's other rows.  A frame is four
waves: group P (0, 1) owns the block rows br with br % 2 == P, and wave WV (0, 1) of a group is rows 64 * WV .. 64 * WV + 63 of each of
them.  What can go wrong is a wave deciding from the wrong rows, so the frames below put the unsatisfied rows of the first turn where
the decision matters -- only BEHIND the test point of a wave, BEFORE it, nowhere -- and the kernel is held to EQUAL the flood path (other
kernels, no skip) in hard bits, iteration counts and flags; then whole trajectories from the device frame source in the waterfall."""
import os
import re

import numpy as np
import pytest

from tests.helpers import CODES, load

NAME = "jpl.4096.4.5"
SZ, NP = 128, 2
STRONG = 8.0
CSRC = os.path.join(os.path.dirname(CODES), "ecc_ldpc_amd", "csrc")


def _k():
    m = re.search(r"^#define SPLIT_SYN_SKIP (\d+)", open(os.path.join(CSRC, "fused_split.hip")).read(), re.M)
    assert m, "fused_split.hip sets SPLIT_SYN_SKIP for its instances"
    return int(m.group(1))


def _frames(c):
    """a strong all-zero codeword (hard bit = LLR > 0; punctured columns at 0): one sign flipped at position 5 and at position 64 + 5 of
    each of the 44 block columns (88 frames), the clean frame, 12 frames with two flips"""
    nbc = c.N // SZ
    assert nbc == 44
    clean = np.full(c.N, -STRONG, np.float32)
    clean[c.n_tx:] = 0.0
    out = []
    for bc in range(nbc):
        for pos in (5, 64 + 5):
            x = clean.copy()
            x[bc * SZ + pos] = -x[bc * SZ + pos]
            out.append(x)
    out.append(clean)
    rng = np.random.default_rng(4045)
    for _ in range(12):
        x = clean.copy()
        at = rng.choice(c.n_tx, 2, replace=False)
        x[at] = -x[at]
        out.append(x)
    return np.stack(out)


def _wave_rows(c, K):
    """per wave (P, WV): the check rows before and behind its test point"""
    nbr = c.M // SZ
    waves = {}
    for P in range(NP):
        own = [br for br in range(nbr) if br % NP == P]
        for WV in range(SZ // 64):
            rows = lambda brs: np.concatenate([np.arange(br * SZ + 64 * WV, br * SZ + 64 * WV + 64) for br in brs])
            waves[(P, WV)] = (rows(own[:K]), rows(own[K:]))
    return waves


def _syndrome(c, llr):
    return (c.H.astype(np.int64) @ (llr > 0).astype(np.int64).T % 2).T.astype(bool)      # [frame, check row]


def test_frames_reach_both_sides_of_every_waves_test_point():
    """(CPU) the condition on the inputs: for each of the four waves the set holds a frame whose only unsatisfied rows in that wave
    lie behind the test point (the wave must still find them), one with unsatisfied rows before it (the wave skips), and one
    without any (the clean frame)."""
    c = load(NAME)
    K = _k()
    assert 0 < K < (c.M // SZ) // NP
    syn = _syndrome(c, _frames(c))
    assert len(syn) == 101 and not syn[88].any()
    for wave, (before, behind) in _wave_rows(c, K).items():
        b, h = syn[:, before].any(axis=1), syn[:, behind].any(axis=1)
        print(wave, "frames with unsatisfied rows only behind the test:", int((~b & h).sum()), " before it:", int(b.sum()),
              " only before it:", int((b & ~h).sum()), " none:", int((~b & ~h).sum()))
        assert (~b & h).any() and b.any() and (~b & ~h).any(), wave


@pytest.mark.gpu
@pytest.mark.parametrize("max_iters", [0, 1, 2])
def test_single_and_double_flips_equal_the_flood_path(hip, max_iters):
    c = load(NAME)
    llr = _frames(c)
    code = c.hip_code(hip)
    dec = hip.Decoder(code, "min", "f32", len(llr))
    a = dec.decode_batch(llr, max_iters)
    assert "fused_split_kernel<float, 1" in dec.kernel_name, dec.kernel_name      # (the launch names its instance)
    b = hip.Decoder(code, "min", "f32", len(llr), path="flood").decode_batch(llr, max_iters)
    print(f"max_iters {max_iters}: converged {int(np.asarray(a[2]).sum())} of {len(llr)}; iteration counts {sorted(set(np.asarray(a[1]).tolist()))}")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    if max_iters == 0:
        assert np.array_equal(np.asarray(a[2]).astype(bool), ~_syndrome(c, llr).any(axis=1))


@pytest.mark.gpu
@pytest.mark.parametrize("ebn0", [2.8, 3.0])
def test_waterfall_trajectories_equal_the_flood_path(hip, ebn0):
    """512 frames from the device frame source, 50 turns: frames converge at different turns, so waves meet both arms turn after turn"""
    import torch
    B, TURNS = 512, 50
    ecc = hip.ECC(CODES, f"ldpc/hip-minsum/{NAME}/{TURNS}/4/5", max_batch=B)
    flood = hip.Decoder(ecc.code, "min", "f32", B, path="flood")
    dev = torch.device("cuda", 0)
    llr = torch.empty((B, ecc.code.N), dtype=torch.float32, device=dev)
    out = [[torch.empty((B, ecc.code.N), dtype=torch.uint8, device=dev), torch.empty((B,), dtype=torch.int32, device=dev),
            torch.empty((B,), dtype=torch.uint8, device=dev)] for _ in range(2)]
    torch.cuda.synchronize()
    ecc.sim.generate(0x5EED, 0, B, ebn0, llr.data_ptr(), None, None)
    torch.cuda.synchronize()
    for d, (bits, its, conv) in zip((ecc.decoder, flood), out):
        d.decode_batch_dev(llr.data_ptr(), bits.data_ptr(), B, TURNS, its.data_ptr(), conv.data_ptr(), None)
        torch.cuda.synchronize()
    assert "fused_split_kernel<float, 1" in ecc.decoder.kernel_name, ecc.decoder.kernel_name
    (ab, ai, ac), (fb, fi, fc) = [[t.cpu().numpy() for t in o] for o in out]
    print(f"{ebn0} dB: converged {int(fc.sum())} of {B}; distinct iteration counts {len(set(fi.tolist()))}")
    assert len(set(fi.tolist())) >= 4          # a condition on the inputs, met by the reference path alone
    assert np.array_equal(ab, fb) and np.array_equal(ai, fi) and np.array_equal(ac, fc)
    flood.close()
    ecc.close()
