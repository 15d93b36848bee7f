"""GPU: the iterative receiver of tests/test_bicm_id_gpu.py -- same code, labels, interleaver, point, 4 outer iterations of 10 sweeps -- with a
decoder that CONTINUES where that test restarts it: one decode state for the batch, reset once, ldpc_decode_batch_dev_continue at every outer
iteration.  The device's LLRs, extrinsic values, bits, sweeps and flags are those of the two specifications chained
(tests/demap_apriori_spec.py, tests/decode_continue_spec.py), bit for bit.  The frame-error counts per iteration are only asserted not to
increase; their values are recorded in profiles/r21_decode_continue.txt."""
import functools

import numpy as np
import pytest

from tests import decode_continue_spec as cspec
from tests import demap_apriori_spec as dspec
from tests import soft_output_spec as sspec
from tests.test_bicm_id_gpu import F, N, OUTER, SWEEPS, setup

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def restatement():
    """per outer iteration: (LLRs into the decoder, bits, sweeps, flags, extrinsic, hard(P)), the two specifications chained"""
    g, pts, pos, cws, nv, sym = setup()
    la = np.zeros((F, N), np.float32)
    st = cspec.State("f32", g, F)
    out = []
    for _ in range(OUTER):
        llr = dspec.demap_il_apriori(pts, sym, None, pos, N, nv, la)
        (bits, sweeps, conv, P, C), st = cspec.call("f32", g, st, llr, SWEEPS)
        la = sspec.soft("f32", P, C, "extrinsic", "f32")
        out.append((llr, bits, sweeps, conv, la, (P > 0).astype(np.uint8)))
    return out


def test_the_continuing_loop_bit_for_bit(hip):
    import torch
    g, pts, pos, cws, nv, sym = setup()
    ref = restatement()
    errors = [int((bits != cws).any(axis=1).sum()) for _, bits, *_ in ref]         # of d_bits, as tests/test_bicm_id_gpu.py counts them
    guesses = [int((guess != cws).any(axis=1).sum()) for *_, guess in ref]         # of the receiver's best guess, hard(P)
    print("frame errors per outer iteration, continuing decoder: d_bits", errors, "hard(P)", guesses)
    assert all(a >= b for a, b in zip(errors, errors[1:])), errors
    assert all(a >= b for a, b in zip(guesses, guesses[1:])), guesses
    dev = torch.device("cuda", 0)
    mod, il = hip.Modulation(pts), hip.Interleaver(pos, N)
    dec = hip.Decoder(hip.Code.from_csr(g.row_ptr, g.col_idx, N), "min", "f32", F, schedule="layered", path="fused")
    state = hip.DecodeState(dec, F)
    d_sym = torch.from_numpy(sym).to(dev)
    d_la, d_ext = torch.zeros((F, N), device=dev), torch.zeros((F, N), device=dev)
    d_llr = torch.zeros((F, N), device=dev)
    d_bits = torch.zeros((F, N), dtype=torch.uint8, device=dev)
    d_iters, d_conv = torch.zeros(F, dtype=torch.int32, device=dev), torch.zeros(F, dtype=torch.uint8, device=dev)
    state.reset()
    for it, (llr, bits, sweeps, conv, ext, _) in enumerate(ref):
        torch.cuda.synchronize()
        hip.demap_il_apriori(mod, il, F, d_sym.data_ptr(), None, nv, d_la.data_ptr(), d_llr.data_ptr(), "f32", 0.0, None)
        torch.cuda.synchronize()
        dec.decode_batch_dev_continue(state, d_llr.data_ptr(), d_bits.data_ptr(), F, SWEEPS, d_ext.data_ptr(), "extrinsic", "f32", 0.0, d_iters.data_ptr(), d_conv.data_ptr())
        dec.synchronize()
        assert dec.kernel_name == "ldpc::layered_csr_cont_kernel<8, float>", dec.kernel_name
        assert np.array_equal(d_llr.cpu().numpy().view(np.uint32), llr.view(np.uint32)), (it, "demapper")
        assert np.array_equal(d_ext.cpu().numpy().view(np.uint32), ext.view(np.uint32)), (it, "extrinsic")
        assert np.array_equal(d_bits.cpu().numpy(), bits) and np.array_equal(d_conv.cpu().numpy().astype(bool), conv), (it, "bits, flags")
        assert np.array_equal(d_iters.cpu().numpy(), sweeps), (it, "sweeps")
        d_la, d_ext = d_ext, d_la                           # the extrinsic output is the next a-priori buffer
    state.close()
    dec.close()
    il.close()
