"""GPU: the frame source's encoder from any H (csrc/sim_systematic.hip, ldpc_sim_create_systematic_on) against the numpy restatement
of its rule (tests/systematic_encoder_spec.py), against the dense, quasi-cyclic and sparse device encoders where those exist, and
against H itself.

The method of tests/test_sparse_encoder_gpu.py: at 40 dB no sample changes sign, so hard(llr[:, :n_tx]) of ldpc_sim_generate IS the
codeword the device encoded; ldpc_sim_encode_batch returns the codeword bytes without a channel.  Messages are
oracle.frame_source.message_bits of (seed, frame id), so the restatement encodes the very messages the device drew."""
import functools

import numpy as np
import pytest

from oracle import frame_source as fs
from tests import dvbs2_natural, dvbs2_short
from tests import systematic_encoder_spec as spec
from tests.helpers import load

pytestmark = pytest.mark.gpu

SEED = 0x5EEDC0DE
BOUND = 16.0       # tests/test_frame_source_gpu.py: LLR error in units of 2^-24 sc (1 + sg ra)


def _codewords(sim, B, N, k, n_tx, first, seed=SEED, ebn0=40.0):
    """-> (messages [B][k], codewords from the noiseless LLRs [B][n_tx], codewords from encode_batch [B][n_tx]); one row more than
    the batch in every buffer: nothing is written for frames >= batch"""
    import torch
    dev = torch.device("cuda", 0)
    llr = torch.full((B + 1, N), 777.0, dtype=torch.float32, device=dev)
    msg = torch.full((B + 1, k), 9, dtype=torch.uint8, device=dev)
    cw = torch.full((B + 1, n_tx), 7, dtype=torch.uint8, device=dev)
    msg2 = torch.full((B + 1, k), 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sim.generate(seed, first, B, ebn0, llr.data_ptr(), msg.data_ptr(), None)
    sim.encode_batch(seed, first, B, cw.data_ptr(), msg2.data_ptr(), None)
    torch.cuda.synchronize()
    l, m, m2, c = llr.cpu().numpy(), msg.cpu().numpy(), msg2.cpu().numpy(), cw.cpu().numpy()
    assert (l[B] == 777.0).all() and (m[B] == 9).all() and (m2[B] == 9).all() and (c[B] == 7).all()
    assert (l[:B, n_tx:] == 0).all() and (np.abs(l[:B, :n_tx]) > 1.0).all()      # noiseless: every sample far from zero
    assert np.array_equal(m, m2)
    return m[:B], (l[:B, :n_tx] > 0).astype(np.uint8), c[:B]


@functools.lru_cache(maxsize=None)
def _form(name):
    H = spec.toy_40x90() if name == "40x90" else load(name).H
    mp, pp, P = spec.systematic_form(H)
    for a in (mp, pp, P):
        a.setflags(write=False)
    return H, mp, pp, P


def _expected(name, ids, seed=SEED):
    """the restatement's messages and codewords of these frames"""
    H, mp, pp, P = _form(name)
    msg = fs.message_bits(seed, np.asarray(ids, dtype=np.uint64), len(mp))
    return msg, spec.encode(H.shape[1], mp, pp, P, msg)


@functools.lru_cache(maxsize=None)
def _expected_1920():
    msg, cw = _expected("1920.1280.3.303", 300 + np.arange(96))
    msg.setflags(write=False); cw.setflags(write=False)
    return msg, cw


def _sim(hip, code, n_tx, B):
    sim = hip.Sim(code, None, n_tx, systematic=True, max_batch=B)
    assert sim.encoder == "systematic"
    return sim


@pytest.mark.parametrize("B", [2049, 1])
def test_moon_equals_the_restatement_the_dense_and_the_sparse_source(hip, B):
    """2049 frames = 33 workgroups, the last with one live lane; frame ids past 2^32"""
    c = load("moon.7.13")
    code = hip.Code.from_csr(c.graph.row_ptr, c.graph.col_idx, c.N)
    first = 2 ** 32 + 5
    sim = _sim(hip, code, 20, B)
    assert sim.k == 7
    mp, pp = sim.positions()
    assert np.array_equal(mp, np.arange(7)) and np.array_equal(pp, np.arange(7, 20))
    msg, from_llr, from_enc = _codewords(sim, B, 20, 7, 20, first)
    wmsg, want = _expected("moon.7.13", first + np.arange(B))
    assert np.array_equal(msg, wmsg)
    assert np.array_equal(from_llr, want) and np.array_equal(from_enc, want)
    for i in (0, B - 1):
        assert np.array_equal(sim.encode_host(msg[i], 13), want[i, 7:])
    for other, kind in ((hip.Sim(code, 7, 20, G=c.G, max_batch=B), "dense"), (hip.Sim(code, 7, 20, from_H=True, max_batch=B), "sparse")):
        assert other.encoder == kind
        omp, opp = other.positions()
        assert np.array_equal(omp, np.arange(7)) and np.array_equal(opp, np.arange(7, 20))
        msg2, from_llr2, from_enc2 = _codewords(other, B, 20, 7, 20, first)
        assert np.array_equal(msg2, msg) and np.array_equal(from_llr2, from_llr) and np.array_equal(from_enc2, from_enc)
        other.close()
    sim.close(); code.close()


def test_random_40x90_ragged_batch_and_punctured_tail(hip):
    """duplicated rows, a zero column, dependent tail columns: message and parity positions interleave.  N = 90 is no multiple of
    4 or 32; 333 frames = 6 workgroups, the last of 13 frames; n_tx = N - 7 cuts into the last codeword word"""
    H, mp, pp, P = _form("40x90")
    N, K, B, first = 90, len(mp), 333, 12345
    assert not np.array_equal(pp, np.arange(K, N))
    rp, ci = spec.csr(H)
    code = hip.Code.from_csr(rp, ci, N)
    wmsg, want = _expected("40x90", first + np.arange(B))
    for n_tx in (N - 7, N):
        sim = _sim(hip, code, n_tx, B)
        assert sim.k == K
        smp, spp = sim.positions()
        assert np.array_equal(smp, mp) and np.array_equal(spp, pp)
        msg, from_llr, from_enc = _codewords(sim, B, N, K, n_tx, first)
        assert np.array_equal(msg, wmsg)                                         # d_msg in msg_pos order
        assert np.array_equal(from_llr, want[:, :n_tx]) and np.array_equal(from_enc, want[:, :n_tx])
        if n_tx == N:
            assert not spec.syndrome(H, from_enc).any()
            assert np.array_equal(from_enc[:, mp], msg)
        for i in (0, 1, B - 1):
            assert np.array_equal(sim.encode_host(msg[i], len(pp)), want[i, pp])
        sim.close()
    code.close()


def test_1920_and_its_redundant_form_give_the_same_codewords(hip):
    import torch
    wmsg, want = _expected_1920()
    a, b = load("1920.1280.3.303"), load("1920.1280.A")
    N, K, B, first, db = 1920, 640, 96, 300, 2.0
    _, mp, pp, _ = _form("1920.1280.3.303")
    dev = torch.device("cuda", 0)
    got = []
    for m in (a, b):
        code = m.hip_code(hip, prefer_qc=False)
        sim = _sim(hip, code, N, B)
        assert sim.k == K
        smp, spp = sim.positions()
        assert np.array_equal(smp, mp) and np.array_equal(spp, pp) and spp[:8].tolist() == [447, 504, 558, 571, 590, 616, 622, 626]
        msg, from_llr, from_enc = _codewords(sim, B, N, K, N, first)
        assert np.array_equal(msg, wmsg) and np.array_equal(from_llr, want) and np.array_equal(from_enc, want)
        assert not spec.syndrome(a.H, from_enc).any() and not spec.syndrome(b.H, from_enc).any()
        assert np.array_equal(sim.encode_host(msg[3], 1280), want[3, pp])
        # 2 dB: the f32 LLRs against oracle.frame_source.llrs of those codewords, the fp16 ones the rounded f32 ones
        out = torch.full((B, N), 777.0, dtype=torch.float32, device=dev)
        out16 = torch.full((B, N), 777.0, dtype=torch.float16, device=dev)
        torch.cuda.synchronize()
        sim.generate(SEED, first, B, db, out.data_ptr(), None, None)
        sim.generate(SEED, first, B, db, out16.data_ptr(), None, None, llr_f16=True)
        torch.cuda.synchronize()
        l, l16 = out.cpu().numpy(), out16.cpu().numpy()
        ref, rad, sg, sc = fs.llrs(SEED, first + np.arange(B), want, K, N, N, db)
        unit = 2.0 ** -24 * sc * (1.0 + sg * rad)
        mult = np.abs(l.astype(np.float64) - ref) / unit
        print(f"{m.name} 2 dB: worst LLR error {mult.max():.2f} x 2^-24 sc (1 + sg ra) over {mult.size} samples (bound {BOUND:g})")
        assert np.isfinite(l).all() and mult.max() <= BOUND
        assert np.array_equal(l16.view(np.uint16), np.clip(l, -65504.0, 65504.0).astype(np.float16).view(np.uint16))
        got.append((from_enc, l))
        sim.close(); code.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32))


def test_jpl1024_equals_the_quasi_cyclic_source(hip):
    c = load("jpl.1024.4.5")
    B, first = 65, 41
    code = c.hip_code(hip)                                                        # quasi-cyclic: taken as its CSR form
    sim = _sim(hip, code, c.n_tx, B)
    assert sim.k == c.k
    mp, pp = sim.positions()
    assert np.array_equal(mp, np.arange(1024)) and np.array_equal(pp, np.arange(1024, 1408))
    msg, from_llr, from_enc = _codewords(sim, B, c.N, c.k, c.n_tx, first)
    sz, words = _qc_words(hip, "jpl.1024.4.5")
    qc = hip.Sim(code, c.k, c.n_tx, G_qc=(sz, words), max_batch=B)
    assert qc.encoder == "qc"
    msg2, from_llr2, from_enc2 = _codewords(qc, B, c.N, c.k, c.n_tx, first)
    assert np.array_equal(msg2, msg) and np.array_equal(from_llr2, from_llr) and np.array_equal(from_enc2, from_enc)
    wmsg, want = _expected("jpl.1024.4.5", first + np.arange(B))
    assert np.array_equal(msg, wmsg) and np.array_equal(from_enc, want[:, :c.n_tx])
    qc.close(); sim.close(); code.close()


def _qc_words(hip, name):
    """(sz, words [block_rows][block_cols][sz/32] uint32) of the shipped G.q, from the oracle-side parser's bits"""
    sz, bits = load(name).gq
    R, Cb, _ = bits.shape
    w = (bits.reshape(R, Cb, sz // 32, 32).astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(-1).astype(np.uint32)
    return sz, w


def test_dvbs2_short_equals_the_sparse_source(hip):
    rp, ci = dvbs2_short.csr()
    N, K, B, first = dvbs2_short.N, dvbs2_short.K, 65, 7000
    code = hip.Code.from_csr(rp, ci, N)
    sim = _sim(hip, code, N, B)
    assert sim.k == K
    mp, pp = sim.positions()
    assert np.array_equal(mp, np.arange(K)) and np.array_equal(pp, np.arange(K, N))
    sp = hip.Sim(code, K, N, from_H=True, max_batch=B)
    msg, from_llr, from_enc = _codewords(sim, B, N, K, N, first)
    msg2, from_llr2, from_enc2 = _codewords(sp, B, N, K, N, first)
    assert np.array_equal(msg2, msg) and np.array_equal(from_llr2, from_llr) and np.array_equal(from_enc2, from_enc)
    assert np.array_equal(msg, fs.message_bits(SEED, (first + np.arange(B)).astype(np.uint64), K))
    sp.close(); sim.close(); code.close()


def test_tally_counts_message_positions_only(hip):
    import torch
    wmsg, want = _expected_1920()
    _, mp, pp, _ = _form("1920.1280.3.303")
    N, B, first = 1920, 96, 300
    code = load("1920.1280.3.303").hip_code(hip, prefer_qc=False)
    sim = _sim(hip, code, N, B)
    dev = torch.device("cuda", 0)
    llr = torch.empty((B, N), dtype=torch.float32, device=dev)
    sim.generate(SEED, first, B, 40.0, llr.data_ptr(), None, None)
    torch.cuda.synchronize()

    def tally(bits, iters=None):
        t = torch.zeros(4, dtype=torch.int64, device=dev)
        d_bits = torch.from_numpy(bits).to(dev)
        d_it = torch.from_numpy(iters).to(dev) if iters is not None else None
        torch.cuda.synchronize()
        sim.tally(B, d_bits.data_ptr(), d_it.data_ptr() if d_it is not None else None, t.data_ptr(), None)
        torch.cuda.synchronize()
        return t.cpu().numpy().tolist()

    assert tally(want.copy()) == [B, 0, 0, 0]
    bits = want.copy()
    assert 447 in pp and 447 not in mp
    bits[[2, 50, 95], 447] ^= 1                                                  # a parity position among the first 640 columns
    assert tally(bits) == [B, 0, 0, 0]
    flips = {0: [mp[0], mp[447], mp[639]], 31: [mp[448]], 95: [mp[5], mp[6]]}      # mp[447] = 448: right behind that parity position
    assert mp[447] == 448 and mp[639] > 640
    for f, cols in flips.items():
        bits[f, cols] ^= 1
    iters = np.arange(B, dtype=np.int32)
    assert tally(bits, iters) == [B, 3, 6, int(iters.sum())]
    sim.close(); code.close()


def test_layered_decoders_accept_the_noiseless_frames(hip):
    """generate -> decode at 40 dB through the fp16-lam and the int8 layered context: H accepts every frame before the first sweep"""
    import torch
    _, want = _expected_1920()
    N, B, first = 1920, 96, 300
    code = load("1920.1280.3.303").hip_code(hip, prefer_qc=False)
    sim = _sim(hip, code, N, B)
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


def test_refusals(hip):
    H, mp, _, _ = _form("40x90")
    rp, ci = spec.csr(H)
    code = hip.Code.from_csr(rp, ci, 90)
    for n_tx in (len(mp) - 1, 91):
        with pytest.raises(hip.LdpcError) as e:
            hip.Sim(code, None, n_tx, systematic=True, max_batch=4)
        assert e.value.code == -1
    with pytest.raises(hip.LdpcError) as e:
        hip.Sim(code, len(mp), 90, systematic=True, max_batch=4)                  # k is not the caller's to choose
    assert e.value.code == -1
    code.close()
    code = hip.Code.from_csr(*dvbs2_natural.csr(), dvbs2_natural.N)
    with pytest.raises(hip.LdpcError) as e:
        hip.Sim(code, None, dvbs2_natural.N, systematic=True, max_batch=4)
    assert e.value.code == -5 and "2^28" in str(e.value)
    code.close()
