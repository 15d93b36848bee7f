"""GPU: the device frame source (csrc/sim.hip: sim_msg_kernel, sim_frame_kernel, sim_tally_kernel) against its CPU restatement
(oracle/frame_source.py), value by value.  The restatement's own statistics are tests/test_frame_source.py's business.

Message bytes are compared exactly.  LLRs: |device - restatement| <= 16 * 2^-24 * sc * (1 + sg * ra), ra = the restatement's
Box-Muller radius of that sample's pair.  Where the 16 comes from: the kernel forms z = ra * (cos, sin) with logf, sqrtf and
sincospif, documented at 1-2 ulp each and built with -fno-fast-math -ffp-contract=off (ecc_ldpc_amd/build.py), about 5 ulp on
z relative to ra; three more roundings follow in sc * (+-1 + sg * z); 16 leaves a factor of two to three over that.  Each case
prints the worst multiple of 2^-24 * sc * (1 + sg * ra) it saw (measured on MI355X: at most 3.16)."""
import numpy as np
import pytest

from oracle import frame_source as fs
from oracle import oracle
from tests.helpers import CODES, load

pytestmark = pytest.mark.gpu

BOUND = 16.0
JPL = "ldpc/hip-minsum/jpl.1024.4.5/50/4/5"
JPL_SEED, JPL_FIRST, JPL_B = 0x5EEDC0DE, 1000, 37
# Found by a search over the restatement: under seed 0 the noise word r0 of (frame 29 034, group 116) is 0xffffffde, which
# rounds to 2^32 as a float, so ua = 1, the radius of positions 464 and 465 is 0, and their LLRs are exactly +-sc.
ZERO_RADIUS = (0, 29034, 464)


def _generate(sim, seed, first, B, db, N, k, f16=False, offset=0):
    """-> (llr [B][N] as the device wrote it, msg [B][k]); offset: elements the output starts after a 16-byte aligned address.
    The buffer is longer than the output on both sides and must come back untouched there."""
    import torch
    dev = torch.device("cuda", 0)
    dt = torch.float16 if f16 else torch.float32
    pad = 8
    buf = torch.full((pad + B * N + pad,), 777.0, dtype=dt, device=dev)
    msg = torch.full((B, k), 9, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0 and (pad * buf.element_size()) % 16 == 0
    out = buf[pad + offset: pad + offset + B * N]
    assert out.data_ptr() == buf.data_ptr() + (pad + offset) * buf.element_size()
    torch.cuda.synchronize()
    sim.generate(seed, first, B, db, out.data_ptr(), msg.data_ptr(), None, llr_f16=f16)
    torch.cuda.synchronize()
    whole = buf.cpu().numpy()
    assert (whole[:pad + offset] == 777.0).all() and (whole[pad + offset + B * N:] == 777.0).all()
    return whole[pad + offset: pad + offset + B * N].reshape(B, N).copy(), msg.cpu().numpy()


def _check_llrs(case, got, ref, rad, sg, sc, n_tx):
    """got: float32 [B][N] from the device; ref, rad, sg, sc: oracle.frame_source.llrs"""
    assert got.dtype == np.float32 and got.shape == ref.shape and np.isfinite(got).all()
    assert not got[:, n_tx:].view(np.uint32).any()                                # punctured tail: exactly 0.0
    unit = 2.0 ** -24 * sc * (1.0 + sg * rad)
    mult = np.abs(got[:, :n_tx].astype(np.float64) - ref[:, :n_tx]) / unit
    print(f"{case}: worst LLR error {mult.max():.2f} x 2^-24 sc (1 + sg ra) over {mult.size} samples (bound {BOUND:g})")
    assert mult.max() <= BOUND, (case, float(mult.max()), np.unravel_index(mult.argmax(), mult.shape))
    zero = rad == 0.0
    assert np.array_equal(got[:, :n_tx][zero], (np.sign(ref[:, :n_tx][zero]) * sc).astype(np.float32))   # z = 0: exactly +-sc
    return int(zero.sum())


def _stub(hip, N):
    # a parity-check graph is needed only for N
    return hip.Code.from_csr(np.array([0, 2], np.int32), np.array([0, 1], np.int32), N)


@pytest.fixture(scope="module")
def jpl(hip):
    """the shipped code's frame source and the restatement's frames 1000 .. 1036 of it (messages, codewords); shared, read-only"""
    ecc = hip.ECC(CODES, JPL, max_batch=64)
    assert ecc.sim.encoder == "qc"
    assert (ecc.message_length, ecc.codeword_length, ecc.unpunctured_length) == (1024, 1280, 1408)
    c = load("jpl.1024.4.5")
    ids = JPL_FIRST + np.arange(JPL_B)
    msg = fs.message_bits(JPL_SEED, ids, 1024)
    cws = np.stack([np.concatenate([m, oracle.encode_qc(c.gq[0], c.gq[1], m)]) for m in msg])
    msg.setflags(write=False); cws.setflags(write=False)
    yield ecc, ids, msg, cws
    ecc.close()


@pytest.fixture(scope="module")
def ragged(hip):
    """dense random generator, k = 36, p = 13 (pp = 16), N = 49, n_tx = 46: a last message word of 4 bits, aligned 16-byte
    generator reads that run into the padding, n_tx and N no multiples of 4, hence the per-element-store instance"""
    rng = np.random.default_rng(3613)
    G = rng.integers(0, 2, size=(36, 13), dtype=np.uint8)
    code = _stub(hip, 49)
    sim = hip.Sim(code, 36, 46, G=G, max_batch=64)
    assert sim.encoder == "dense"
    yield sim, G
    sim.close(); code.close()


def _dense_case(case, sim, G, seed, ids, k, n_tx, N, db):
    """generate ids (consecutive) on a dense-generator source and compare with the restatement -> (llr, msg) of the device"""
    ids = np.asarray(ids, dtype=np.uint64)
    got, gmsg = _generate(sim, seed, int(ids[0]), len(ids), db, N, k)
    msg = fs.message_bits(seed, ids, k)
    assert np.array_equal(gmsg, msg)
    if G is None:
        cws = np.zeros((len(ids), n_tx), np.uint8)
    else:
        cws = np.stack([np.concatenate([m, oracle.encode_dense(G, m)]) for m in msg])
    ref, rad, sg, sc = fs.llrs(seed, ids, cws, k, n_tx, N, db)
    _check_llrs(case, got, ref, rad, sg, sc, n_tx)
    return got, gmsg


@pytest.mark.parametrize("db", [0.0, 2.0, 40.0])
def test_shipped_code_vector_store_path(jpl, db):
    ecc, ids, msg, cws = jpl
    got, gmsg = _generate(ecc.sim, JPL_SEED, JPL_FIRST, JPL_B, db, 1408, 1024)
    assert np.array_equal(gmsg, msg)
    ref, rad, sg, sc = fs.llrs(JPL_SEED, ids, cws, 1024, 1280, 1408, db)
    _check_llrs(f"jpl.1024 {db:g} dB", got, ref, rad, sg, sc, 1280)
    if db == 40.0:
        assert np.array_equal(got[:, :1280] > 0, cws[:, :1280] == 1)


def test_device_known_answer(jpl):
    """independent of the restatement: Random123's first known answer, philox4x32_10(counter 0, key 0) = 6627e8d5 ...;
    word 0 of (seed 0, frame 0)'s message is its output word 0"""
    _, gmsg = _generate(jpl[0].sim, 0, 0, 1, 3.0, 1408, 1024)
    assert gmsg[0, :32].tolist() == [(0x6627e8d5 >> i) & 1 for i in range(32)]


def test_zero_radius_sample_is_exactly_the_scale(jpl):
    seed, frame, pos = ZERO_RADIUS
    ids = np.array([frame])
    _, rad = fs.normals(seed, ids, 1280)
    assert rad[0, pos] == 0.0 and rad[0, pos + 1] == 0.0
    got, gmsg = _generate(jpl[0].sim, seed, frame, 1, 1.0, 1408, 1024)
    msg = fs.message_bits(seed, ids, 1024)
    assert np.array_equal(gmsg, msg)
    c = load("jpl.1024.4.5")
    cws = np.concatenate([msg[0], oracle.encode_qc(c.gq[0], c.gq[1], msg[0])])[None, :]
    ref, rad, sg, sc = fs.llrs(seed, ids, cws, 1024, 1280, 1408, 1.0)
    assert _check_llrs("jpl.1024 1 dB, a frame with a zero radius", got, ref, rad, sg, sc, 1280) == 2
    assert np.abs(got[0, pos:pos + 2]).tolist() == [sc, sc]


@pytest.mark.parametrize("db", [2.0, 7.5])
def test_per_element_store_path_and_ragged_sizes(ragged, db):
    sim, G = ragged
    _dense_case(f"k 36 p 13 N 49 n_tx 46, {db:g} dB", sim, G, 0xC0FFEE, 5 + np.arange(37), 36, 46, 49, db)


def test_moon_shape_per_column_path(hip):
    """k = 7, p = 13 (moon.7.13): k is no multiple of 4, so the group straddling k and every parity group take the
    per-column generator reads"""
    rng = np.random.default_rng(713)
    G = rng.integers(0, 2, size=(7, 13), dtype=np.uint8)
    code = _stub(hip, 20)
    sim = hip.Sim(code, 7, 20, G=G, max_batch=64)
    _dense_case("k 7 p 13 N 20 n_tx 20, 2 dB", sim, G, 0xC0FFEE, 5 + np.arange(37), 7, 20, 20, 2.0)
    sim.close()
    sim = hip.Sim(code, 7, 18, G=G, max_batch=64)                     # and with the last parity bits punctured
    _dense_case("k 7 p 13 N 20 n_tx 18, 2 dB", sim, G, 0xC0FFEE, 5 + np.arange(37), 7, 18, 20, 2.0)
    sim.close(); code.close()


def test_both_store_instances_write_the_same_values(jpl):
    """N % 4 == 0: a 16-byte aligned buffer takes the vector-store instance, the same buffer one element later the
    per-element-store instance; fp16 = the float32 values saturated and rounded to nearest even (include/ldpc_hip.h)"""
    sim = jpl[0].sim
    a, ma = _generate(sim, JPL_SEED, JPL_FIRST, JPL_B, 2.0, 1408, 1024)
    b, mb = _generate(sim, JPL_SEED, JPL_FIRST, JPL_B, 2.0, 1408, 1024, offset=1)            # + 4 bytes
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(ma, mb)
    ha, _ = _generate(sim, JPL_SEED, JPL_FIRST, JPL_B, 2.0, 1408, 1024, f16=True)
    hb, _ = _generate(sim, JPL_SEED, JPL_FIRST, JPL_B, 2.0, 1408, 1024, f16=True, offset=1)  # + 2 bytes
    assert ha.dtype == np.float16 and np.array_equal(ha.view(np.uint16), hb.view(np.uint16))
    assert np.array_equal(ha.view(np.uint16), np.clip(a, -65504.0, 65504.0).astype(np.float16).view(np.uint16))


def test_no_generator(hip):
    """a source without G: messages and codewords all zero, llr = sc (-1 + sg z)"""
    code = _stub(hip, 49)
    sim = hip.Sim(code, 36, 46, max_batch=64)
    assert sim.encoder == "none"
    import torch
    dev = torch.device("cuda", 0)
    B = 37
    out = torch.empty((B, 49), dtype=torch.float32, device=dev)
    msg = torch.full((B, 36), 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sim.generate(11, 70, B, 2.0, out.data_ptr(), msg.data_ptr(), None)
    torch.cuda.synchronize()
    assert not msg.cpu().numpy().any()
    ids = 70 + np.arange(B)
    ref, rad, sg, sc = fs.llrs(11, ids, np.zeros((B, 46), np.uint8), 36, 46, 49, 2.0)
    z, _ = fs.normals(11, ids, 46)
    assert np.array_equal(ref[:, :46], sc * (-1.0 + sg * z))
    _check_llrs("no generator, 2 dB", out.cpu().numpy(), ref, rad, sg, sc, 46)
    sim.close(); code.close()


def test_64_bit_frame_ids(ragged):
    """frames 2^32 - 2 .. 2^32 + 1: the counter's high word"""
    sim, G = ragged
    ids = np.arange(2 ** 32 - 2, 2 ** 32 + 2, dtype=np.uint64)
    got, gmsg = _dense_case("frames 2^32 - 2 .. 2^32 + 1, 2 dB", sim, G, 0x0123456789ABCDEF, ids, 36, 46, 49, 2.0)
    for i in range(4):
        for j in range(i):
            assert (got[i, :46] != got[j, :46]).mean() > 0.9 and not np.array_equal(gmsg[i], gmsg[j])
    # frame 2^32 is not frame 0, frame 2^32 + 1 not frame 1
    low, lmsg = _dense_case("frames 0 .. 1, 2 dB", sim, G, 0x0123456789ABCDEF, np.arange(2), 36, 46, 49, 2.0)
    assert (low[:, :46] != got[2:, :46]).mean() > 0.9 and not np.array_equal(lmsg, gmsg[2:])


def test_seed_separation(ragged):
    """seeds 7 and 7 + 2^32: the key's high word"""
    sim, G = ragged
    ids = 100 + np.arange(37)
    a, ma = _dense_case("seed 7, 2 dB", sim, G, 7, ids, 36, 46, 49, 2.0)
    b, mb = _dense_case("seed 7 + 2^32, 2 dB", sim, G, 7 + 2 ** 32, ids, 36, 46, 49, 2.0)
    assert (a[:, :46] != b[:, :46]).mean() > 0.9
    assert 0.3 < (ma != mb).mean() < 0.7


def test_fp16_saturation(jpl):
    """46 dB: sc = 2/sigma^2 = 1.27e5 is above fp16's largest finite value, 65 504.  The fp16 output saturates, as the header
    promises; the float32 output of the same frames is finite and within the bound"""
    ecc, ids, msg, cws = jpl
    ref, rad, sg, sc = fs.llrs(JPL_SEED, ids, cws, 1024, 1280, 1408, 46.0)
    assert sc > 1.2e5
    h, hmsg = _generate(ecc.sim, JPL_SEED, JPL_FIRST, JPL_B, 46.0, 1408, 1024, f16=True)
    assert np.array_equal(hmsg, msg) and h.dtype == np.float16
    assert not np.isinf(h).any() and not np.isnan(h).any()
    want = np.where(cws[:, :1280] == 1, 65504.0, -65504.0).astype(np.float16)
    assert np.array_equal(h[:, :1280].view(np.uint16), want.view(np.uint16))
    assert not h[:, 1280:].view(np.uint16).any()
    got, _ = _generate(ecc.sim, JPL_SEED, JPL_FIRST, JPL_B, 46.0, 1408, 1024)
    _check_llrs("jpl.1024 46 dB", got, ref, rad, sg, sc, 1280)


def test_tally_against_a_numpy_recount(ragged):
    """batch 37: neither the 4 frames of a workgroup nor (k = 36) the 64 lanes of a wave divide the work evenly"""
    import torch
    sim, G = ragged
    dev = torch.device("cuda", 0)
    B, N, k, seed, first = 37, 49, 36, 0xBEEF, 400
    _generate(sim, seed, first, B, 2.0, N, k)                          # the message words stay inside the source
    msg = fs.message_bits(seed, first + np.arange(B), k)
    bits = np.zeros((B, N), np.uint8)
    bits[:, :k] = msg
    bits[:, k:] = np.random.default_rng(5).integers(0, 2, size=(B, N - k))
    for f, n in [(0, 0), (5, 35), (9, 3), (9, 17), (9, 35), (36, 20),  # message part: bit 0, bit 35, three in one frame, the last frame
                 (2, 36), (3, 48), (9, 40)]:                           # positions >= k do not count
        bits[f, n] ^= 1
    iters = np.random.default_rng(6).integers(1, 51, size=B).astype(np.int32)
    wrong = bits[:, :k] != msg
    want = np.array([B, int(wrong.any(axis=1).sum()), int(wrong.sum()), int(iters.sum())], np.int64)
    assert want.tolist()[:3] == [37, 4, 6]
    start = np.array([10, 20, 30, 1000], np.int64)
    d_bits, d_iters, tally = torch.from_numpy(bits).to(dev), torch.from_numpy(iters).to(dev), torch.from_numpy(start).to(dev)
    torch.cuda.synchronize()
    sim.tally(B, d_bits.data_ptr(), None, tally.data_ptr(), None)      # no iteration counts: the fourth counter stays
    torch.cuda.synchronize()
    assert tally.cpu().numpy().tolist() == (start + want * [1, 1, 1, 0]).tolist()
    sim.tally(B, d_bits.data_ptr(), d_iters.data_ptr(), tally.data_ptr(), None)               # the counters accumulate
    torch.cuda.synchronize()
    assert tally.cpu().numpy().tolist() == (start + want * [2, 2, 2, 1]).tolist()
