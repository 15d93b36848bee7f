"""GPU: the frame source's encoder from H (csrc/sim_sparse.hip, ldpc_sim_create_sparse_on) against the numpy restatement of its rule
(tests/sparse_encoder_spec.py), against the dense device encoder of an equivalent generator, and against H itself.

The method of tests/test_encoder_gpu.py: at 40 dB no sample changes sign, so hard(llr[:, :n_tx]) of ldpc_sim_generate IS the codeword
the device encoded; ldpc_sim_encode_batch returns the codeword bytes without a channel.  Messages are oracle.frame_source.message_bits
of (seed, frame id), so the restatement encodes the very messages the device drew."""
import functools

import numpy as np
import pytest

from oracle import frame_source as fs
from tests import dvbs2_short
from tests import sparse_encoder_spec as spec
from tests.helpers import load

pytestmark = pytest.mark.gpu

SEED = 0x5EEDC0DE


def _codewords(sim, B, N, k, n_tx, first, seed=SEED, ebn0=40.0):
    """-> (messages [B][k], codewords from the noiseless LLRs [B][n_tx], codewords from encode_batch [B][n_tx])"""
    import torch
    dev = torch.device("cuda", 0)
    llr = torch.empty((B, N), dtype=torch.float32, device=dev)
    msg = torch.full((B, k), 9, dtype=torch.uint8, device=dev)
    cw = torch.full((B + 1, n_tx), 7, dtype=torch.uint8, device=dev)         # one row more: nothing is written for frames >= batch
    msg2 = torch.full((B, k), 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sim.generate(seed, first, B, ebn0, llr.data_ptr(), msg.data_ptr(), None)
    sim.encode_batch(seed, first, B, cw.data_ptr(), msg2.data_ptr(), None)
    torch.cuda.synchronize()
    l = llr.cpu().numpy()
    assert (l[:, n_tx:] == 0).all() and (np.abs(l[:, :n_tx]) > 1.0).all()      # noiseless: every sample far from zero
    assert np.array_equal(msg.cpu().numpy(), msg2.cpu().numpy())
    c = cw.cpu().numpy()
    assert (c[B] == 7).all()
    return msg.cpu().numpy(), (l[:, :n_tx] > 0).astype(np.uint8), c[:B]


def _expected(rp, ci, N, ids, seed=SEED):
    """the restatement's messages and codewords of these frames"""
    K = N - (len(rp) - 1)
    msg = fs.message_bits(seed, np.asarray(ids, dtype=np.uint64), K)
    return msg, spec.encode(rp, ci, N, spec.triangular_order(rp, ci, N), msg)


@functools.lru_cache(maxsize=None)
def _short_cases():
    """dvbs2_short in natural row order and in csr_layer_order order (with its layers), and the restatement's 65 codewords"""
    import ecc_ldpc_amd as E
    rp, ci = dvbs2_short.csr()
    perm, lp = E.Code.csr_layer_order(rp, ci, dvbs2_short.N)
    prp, pci = E.Code.permute_rows(rp, ci, perm)
    msg, cw = _expected(rp, ci, dvbs2_short.N, 7000 + np.arange(65))
    msg.setflags(write=False); cw.setflags(write=False)
    return (rp, ci), (prp, pci, lp), msg, cw


@pytest.mark.parametrize("B", [2049, 1])
def test_moon_equals_the_restatement_and_its_shipped_generator(hip, B):
    """2049 frames = 65 frame words: a second wave with one live lane holding one frame; frame ids past 2^32"""
    c = load("moon.7.13")
    code = hip.Code.from_csr(c.graph.row_ptr, c.graph.col_idx, c.N)
    first = 2 ** 32 + 5
    sim = hip.Sim(code, 7, 20, from_H=True, max_batch=B)
    assert sim.encoder == "sparse"
    msg, from_llr, from_enc = _codewords(sim, B, 20, 7, 20, first)
    wmsg, want = _expected(c.graph.row_ptr, c.graph.col_idx, 20, first + np.arange(B))
    assert np.array_equal(msg, wmsg)
    assert np.array_equal(from_llr, want) and np.array_equal(from_enc, want)
    dn = hip.Sim(code, 7, 20, G=c.G, max_batch=B)
    assert dn.encoder == "dense"
    msg2, from_llr2, from_enc2 = _codewords(dn, B, 20, 7, 20, first)
    assert np.array_equal(msg2, msg) and np.array_equal(from_llr2, from_llr) and np.array_equal(from_enc2, from_enc)
    sim.close(); dn.close(); code.close()


def test_toy_with_far_parity_edges_ragged_batch_and_punctured_tail(hip):
    """M 70, K 45, N 115: parity edges far back, rows without message bits, a row of weight 1, rows shuffled.  333 frames = 11 frame
    words, the last one of 13 frames; n_tx = N - 7 cuts into the last parity word"""
    rp, ci, N = spec.toy(70, 45)
    M, K, B, first = 70, 45, 333, 12345
    code = hip.Code.from_csr(rp, ci, N)
    wmsg, want = _expected(rp, ci, N, first + np.arange(B))
    assert not spec.syndrome(rp, ci, want).any()
    order = spec.triangular_order(rp, ci, N)
    G = spec.encode(rp, ci, N, order, np.eye(K, dtype=np.uint8))[:, K:]      # the generator this H implies, row by row
    for n_tx in (N - 7, N):
        sim = hip.Sim(code, K, n_tx, from_H=True, max_batch=B)
        assert sim.encoder == "sparse"
        msg, from_llr, from_enc = _codewords(sim, B, N, K, n_tx, first)
        assert np.array_equal(msg, wmsg)
        assert np.array_equal(from_llr, want[:, :n_tx]) and np.array_equal(from_enc, want[:, :n_tx])
        if n_tx == N:
            assert not spec.syndrome(rp, ci, from_enc).any()
        for i in (0, 1, B - 1):
            assert np.array_equal(sim.encode_host(msg[i], M), want[i, K:])
        dn = hip.Sim(code, K, n_tx, G=G, max_batch=B)
        msg2, from_llr2, from_enc2 = _codewords(dn, B, N, K, n_tx, first)
        assert np.array_equal(msg2, msg) and np.array_equal(from_llr2, from_llr) and np.array_equal(from_enc2, from_enc)
        sim.close(); dn.close()
    code.close()


def test_dvbs2_short_in_both_row_orders(hip):
    (rp, ci), (prp, pci, _), wmsg, want = _short_cases()
    N, K, B = dvbs2_short.N, dvbs2_short.K, 65
    got = []
    for r, c in ((rp, ci), (prp, pci)):
        code = hip.Code.from_csr(r, c, N)
        sim = hip.Sim(code, K, N, from_H=True, max_batch=B)
        msg, from_llr, from_enc = _codewords(sim, B, N, K, N, 7000)
        assert np.array_equal(msg, wmsg) and 0.45 < msg.mean() < 0.55
        assert np.array_equal(from_llr, want) and np.array_equal(from_enc, want)
        assert not spec.syndrome(r, c, from_enc).any()
        got.append(from_enc)
        sim.close(); code.close()
    assert np.array_equal(got[0], got[1])


def test_llr_values_fp16_output_and_punctured_tail(hip):
    """the toy at 2 dB against oracle.frame_source.llrs of the restatement's codewords; the bound of tests/test_frame_source_gpu.py"""
    import torch
    rp, ci, N = spec.toy(70, 45)
    K, n_tx, B, first, db = 45, N - 7, 33, 900, 2.0
    code = hip.Code.from_csr(rp, ci, N)
    sim = hip.Sim(code, K, n_tx, from_H=True, max_batch=64)
    dev = torch.device("cuda", 0)
    out = torch.full((B, N), 777.0, dtype=torch.float32, device=dev)
    out16 = torch.full((B, N), 777.0, dtype=torch.float16, device=dev)
    msg = torch.full((B, K), 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sim.generate(SEED, first, B, db, out.data_ptr(), msg.data_ptr(), None)
    sim.generate(SEED, first, B, db, out16.data_ptr(), None, None, llr_f16=True)
    torch.cuda.synchronize()
    got, got16 = out.cpu().numpy(), out16.cpu().numpy()
    ids = first + np.arange(B)
    wmsg, want = _expected(rp, ci, N, ids)
    assert np.array_equal(msg.cpu().numpy(), wmsg)
    ref, rad, sg, sc = fs.llrs(SEED, ids, want, K, n_tx, N, db)
    assert np.isfinite(got).all() and not got[:, n_tx:].view(np.uint32).any() and not got16[:, n_tx:].view(np.uint16).any()
    unit = 2.0 ** -24 * sc * (1.0 + sg * rad)
    mult = np.abs(got[:, :n_tx].astype(np.float64) - ref[:, :n_tx]) / unit
    print(f"toy 2 dB: worst LLR error {mult.max():.2f} x 2^-24 sc (1 + sg ra) over {mult.size} samples (bound 16)")
    assert mult.max() <= 16.0
    assert np.array_equal(got16.view(np.uint16), np.clip(got, -65504.0, 65504.0).astype(np.float16).view(np.uint16))
    sim.close(); code.close()


def _end_to_end(hip, rp, ci, N, lp, want, first):
    """generate -> decode -> tally at 40 dB through an fp16-lam and an int8 layered context: the decoder's own H accepts every frame
    before its first sweep, and its bits are the transmitted codeword"""
    import torch
    K, B = N - (len(rp) - 1), 64
    code = hip.Code.from_csr(rp, ci, N)
    if lp is not None:
        code.set_layers(lp)
    sim = hip.Sim(code, K, N, from_H=True, max_batch=B)
    dev = torch.device("cuda", 0)
    llr = torch.empty((B, N), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    sim.generate(SEED, first, B, 40.0, llr.data_ptr(), None, None)
    torch.cuda.synchronize()
    for cell in ("f16", "i8"):
        dec = hip.Decoder(code, "min", cell, B, schedule="layered")
        bits = torch.full((B, N), 9, dtype=torch.uint8, device=dev)
        its = torch.full((B,), -1, dtype=torch.int32, device=dev)
        conv = torch.full((B,), 9, dtype=torch.uint8, device=dev)
        tally = torch.zeros(4, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        dec.decode_batch_dev(llr.data_ptr(), bits.data_ptr(), B, 5, its.data_ptr(), conv.data_ptr(), None)
        dec.synchronize()
        torch.cuda.synchronize()
        sim.tally(B, bits.data_ptr(), its.data_ptr(), tally.data_ptr(), None)
        torch.cuda.synchronize()
        assert (conv.cpu().numpy() == 1).all() and (its.cpu().numpy() == 0).all(), cell
        assert np.array_equal(bits.cpu().numpy(), want), cell
        assert tally.cpu().numpy().tolist() == [B, 0, 0, 0], cell
        dec.close()
    sim.close(); code.close()


def test_end_to_end_dvbs2_short_in_helper_order(hip):
    _, (prp, pci, lp), _, want = _short_cases()
    _end_to_end(hip, prp, pci, dvbs2_short.N, lp, want[:64], 7000)


def test_end_to_end_toy(hip):
    rp, ci, N = spec.toy_decodable()
    _, want = _expected(rp, ci, N, 50 + np.arange(64))
    _end_to_end(hip, rp, ci, N, None, want, 50)


def test_refusals_and_no_side_effects(hip):
    import torch
    rp, ci = spec.ring(*dvbs2_short.csr(), dvbs2_short.N)
    code = hip.Code.from_csr(rp, ci, dvbs2_short.N)
    with pytest.raises(hip.LdpcError) as e:
        hip.Sim(code, dvbs2_short.K, dvbs2_short.N, from_H=True, max_batch=4)
    assert e.value.code == -5 and "rows 0 and 8999 end in column 16199" in str(e.value)
    code.close()
    m = load("1920.1280.3.303")
    code = m.hip_code(hip, prefer_qc=False)
    with pytest.raises(hip.LdpcError) as e:
        hip.Sim(code, m.N - m.M, m.N, from_H=True, max_batch=4)
    assert e.value.code == -5 and "end in column" in str(e.value)
    code.close()
    rp, ci, N = spec.toy(70, 45)
    code = hip.Code.from_csr(rp, ci, N)
    for n_tx in (44, N + 1):
        with pytest.raises(hip.LdpcError) as e:
            hip.Sim(code, 45, n_tx, from_H=True, max_batch=4)
        assert e.value.code == -1
    with pytest.raises(hip.LdpcError) as e:
        hip.Sim(code, 44, N, from_H=True, max_batch=4)                         # k is not the caller's to choose
    assert e.value.code == -1
    ok = hip.Sim(code, 45, N, from_H=True, max_batch=4)                        # a source from H next to a default one on the same code
    plain = hip.Sim(code, 45, N, max_batch=40)
    assert plain.encoder == "none" and ok.encoder == "sparse"
    dev = torch.device("cuda", 0)
    cw = torch.full((40, N), 7, dtype=torch.uint8, device=dev)
    msg = torch.full((40, 45), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    plain.encode_batch(SEED, 0, 40, cw.data_ptr(), msg.data_ptr(), None)
    torch.cuda.synchronize()
    assert not cw.cpu().numpy().any() and not msg.cpu().numpy().any()
    ok.close(); plain.close(); code.close()
