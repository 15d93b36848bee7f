"""GPU: the iterative receiver (BICM-ID) -- ldpc_demap_dev_il_apriori, then ldpc_decode_batch_dev_soft with the extrinsic kind, whose output is
the next a-priori buffer -- on code 1920.1280.3.303 with f32 cells on the on-chip layered kernel for any H, 16QAM with shuffled (non-Gray)
labels, a random interleaver, 5 dB, 4 outer iterations of 10 sweeps, the decoder restarted each time, max-log.
The device's extrinsic values, bits and flags are those of the two specifications chained (tests/demap_apriori_spec.py,
tests/soft_output_spec.py), bit for bit, at every outer iteration.  On the restatement alone: at least 24 of the 32 frames are in error after
the first iteration and at most 4 after the fourth -- the loop does something."""
import functools

import numpy as np
import pytest

from tests import demap_apriori_spec as dspec
from tests import modulation_spec as ms
from tests import soft_output_spec as sspec
from tests.codewords import codewords
from tests.helpers import load

pytestmark = pytest.mark.gpu

NAME, K_BITS, N, F, DB, OUTER, SWEEPS = "1920.1280.3.303", 640, 1920, 32, 5.0, 4, 10


@functools.lru_cache(maxsize=None)
def setup():
    g = load(NAME).graph
    pts = np.ascontiguousarray(ms.builtin(ms.QAM16)[np.random.default_rng(5).permutation(16)], np.float32)
    pos = np.random.default_rng(9).permutation(N).astype(np.int32)
    cws = codewords(g, F, 7)
    nv = ms.noise_var(K_BITS, N, pts, DB)
    sent = pts[ms.labels(cws[:, pos], 4)].astype(np.float64)
    sym = (sent + np.random.default_rng(11).normal(0.0, np.sqrt(nv), sent.shape)).astype(np.float32)
    return g, pts, pos, cws, nv, sym


@functools.lru_cache(maxsize=None)
def restatement():
    """per outer iteration: (LLRs into the decoder, bits, sweeps, flags, extrinsic), the two specifications chained"""
    g, pts, pos, cws, nv, sym = setup()
    la = np.zeros((F, N), np.float32)
    out = []
    for _ in range(OUTER):
        llr = dspec.demap_il_apriori(pts, sym, None, pos, N, nv, la)
        bits, sweeps, conv, P, C = sspec.decode("f32", g, llr, SWEEPS)
        la = sspec.soft("f32", P, C, "extrinsic", "f32")
        out.append((llr, bits, sweeps, conv, la))
    return out


def test_the_loop_bit_for_bit(hip):
    import torch
    g, pts, pos, cws, nv, sym = setup()
    ref = restatement()
    errors = [int((bits != cws).any(axis=1).sum()) for _, bits, _, _, _ in ref]
    assert errors[0] >= 24 and errors[-1] <= 4, errors
    dev = torch.device("cuda", 0)
    mod, il = hip.Modulation(pts), hip.Interleaver(pos, N)
    dec = hip.Decoder(hip.Code.from_csr(g.row_ptr, g.col_idx, N), "min", "f32", F, schedule="layered", path="fused")
    assert dec.path == "fused" and dec.kernel_name == "ldpc::layered_csr_kernel<8, float>", dec.kernel_name
    d_sym = torch.from_numpy(sym).to(dev)
    d_la, d_ext = torch.zeros((F, N), device=dev), torch.zeros((F, N), device=dev)
    d_llr = torch.zeros((F, N), device=dev)
    d_bits = torch.zeros((F, N), dtype=torch.uint8, device=dev)
    d_iters, d_conv = torch.zeros(F, dtype=torch.int32, device=dev), torch.zeros(F, dtype=torch.uint8, device=dev)
    for it, (llr, bits, sweeps, conv, ext) in enumerate(ref):
        torch.cuda.synchronize()
        hip.demap_il_apriori(mod, il, F, d_sym.data_ptr(), None, nv, d_la.data_ptr(), d_llr.data_ptr(), "f32", 0.0, None)
        torch.cuda.synchronize()
        dec.decode_batch_dev_soft(d_llr.data_ptr(), d_bits.data_ptr(), d_ext.data_ptr(), F, SWEEPS, "extrinsic", "f32", 0.0, d_iters.data_ptr(), d_conv.data_ptr())
        dec.synchronize()
        assert dec.kernel_name == "ldpc::layered_csr_soft_kernel<8, float>", dec.kernel_name
        assert np.array_equal(d_llr.cpu().numpy().view(np.uint32), llr.view(np.uint32)), (it, "demapper")
        assert np.array_equal(d_ext.cpu().numpy().view(np.uint32), ext.view(np.uint32)), (it, "extrinsic")
        assert np.array_equal(d_bits.cpu().numpy(), bits) and np.array_equal(d_conv.cpu().numpy().astype(bool), conv), (it, "bits, flags")
        assert np.array_equal(d_iters.cpu().numpy(), sweeps), (it, "sweeps")
        d_la, d_ext = d_ext, d_la                           # the extrinsic output is the next a-priori buffer
    dec.close()
    il.close()
