"""GPU: the caller's own messages through the device encoders -- ldpc_sim_encode_messages, ldpc_sim_generate_from,
ldpc_sim_extract_messages (csrc/sim.hip: sim_load_bytes_kernel, sim_load_packed_kernel, sim_pack_codeword_kernel, sim_extract_kernel).

Per source, the smallest that reach every branch (dense / quasi-cyclic / encoder from H / systematic form; one message word and many;
k % 32 = 0, 7, 16, 23; k % 16 = 0 with 16 and with 32 bits in the last word: the 16-byte loads; packed codeword rows of whole words and
ragged ones; the 16 384-frame chunk of the bit-sliced scratch):
  1. replay: the messages ldpc_sim_encode_batch / ldpc_sim_generate / _f16 drew, fed back, give the same codeword bytes and, at 2 dB, the
     same float32 and fp16 LLRs bit for bit;
  2. independent messages (numpy-drawn, all ones, unit messages) against the CPU restatement of the source's rule, and H c = 0;
  3. formats: packed in = bytes in, packed out = np.packbits(bytes out, little), pad bits in ignored, bytes 2 3 254 255 read as 0 1 0 1,
     buffers that miss the alignment of the vector paths;
  4. ldpc_sim_tally counts against the caller's messages;
  5. round trip: encode -> generate_from at 40 dB -> f32 min-sum decode -> extract_messages, both formats, returns the messages.  Where
     every position is transmitted the decoder must stop before its first iteration; a punctured tail (LLR 0) has to be filled in by
     iterations, which cannot move a message bit: every check-to-variable message there is zero or agrees with the codeword;
  6. refusals.
Every output buffer carries one guard row past the batch, which must stay untouched."""
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import dvbs2_short
from tests import encode_messages_spec as bitspec
from tests import sparse_encoder_spec as sparse_spec
from tests import systematic_encoder_spec as sys_spec
from tests.helpers import CODES, load

pytestmark = pytest.mark.gpu

SEED, FIRST = 0x5EEDC0DE, 2 ** 32 + 11


class Source:
    """sim: the frame source; code: what a decoder is built from; restate(msg [F][k]) -> codewords [F][n_tx]; H: dense, for H c = 0
    where n_tx = N (None: the sparse syndrome is used, or none)"""

    def __init__(self, sim, code, N, n_tx, restate, kind, syndrome=None, owners=()):
        self.sim, self.code, self.N, self.n_tx, self.k = sim, code, N, n_tx, sim.k
        self.restate, self.kind, self.syndrome, self.owners = restate, kind, syndrome, owners
        assert sim.encoder == kind

    def close(self):
        for o in self.owners:
            o.close()


@functools.lru_cache(maxsize=None)
def _sys_form(name):
    H = sys_spec.toy_40x90() if name == "40x90" else load(name).H
    mp, pp, P = sys_spec.systematic_form(H)
    return H, mp, pp, P


def _dense_moon(hip, B, n_tx):
    c = load("moon.7.13")
    code = hip.Code.from_csr(c.graph.row_ptr, c.graph.col_idx, c.N)
    sim = hip.Sim(code, 7, n_tx, G=c.G, max_batch=B)
    G = c.G.astype(np.int64)
    restate = lambda m: np.concatenate([m, ((m.astype(np.int64) @ G) & 1).astype(np.uint8)], axis=1)[:, :n_tx]
    return Source(sim, code, c.N, n_tx, restate, "dense", lambda cw: sys_spec.syndrome(c.H, cw), (sim, code))


def _qc_jpl1024(hip, B):
    c = load("jpl.1024.4.5")
    ecc = hip.ECC(CODES, "ldpc/hip-minsum/jpl.1024.4.5/50/4/5", max_batch=B)
    assert (ecc.message_length, ecc.codeword_length, ecc.unpunctured_length) == (c.k, c.n_tx, c.N) and c.n_tx < c.N
    code = c.hip_code(hip)
    restate = lambda m: np.stack([np.concatenate([r, oracle.encode_qc(c.gq[0], c.gq[1], r)]) for r in m])[:, :c.n_tx]
    return Source(ecc.sim, code, c.N, c.n_tx, restate, "qc", None, (ecc, code))


def _sparse(hip, B, rp, ci, N):
    code = hip.Code.from_csr(rp, ci, N)
    K = N - (len(rp) - 1)
    sim = hip.Sim(code, K, N, from_H=True, max_batch=B)
    order = sparse_spec.triangular_order(rp, ci, N)
    return Source(sim, code, N, N, lambda m: sparse_spec.encode(rp, ci, N, order, m), "sparse", lambda cw: sparse_spec.syndrome(rp, ci, cw), (sim, code))


def _sparse_moon(hip, B):
    c = load("moon.7.13")
    return _sparse(hip, B, c.graph.row_ptr, c.graph.col_idx, c.N)


def _systematic(hip, B, name, n_tx=None):
    H, mp, pp, P = _sys_form(name)
    N = H.shape[1]
    n_tx = N if n_tx is None else n_tx
    code = hip.Code.from_csr(*sys_spec.csr(H), N)
    sim = hip.Sim(code, None, n_tx, systematic=True, max_batch=B)
    assert sim.k == len(mp)
    return Source(sim, code, N, n_tx, lambda m: sys_spec.encode(N, mp, pp, P, m)[:, :n_tx], "systematic", lambda cw: sys_spec.syndrome(H, cw), (sim, code))


CASES = {
    "dense-moon-ntx20": (67, lambda hip, B: _dense_moon(hip, B, 20)),                   # one message word of 7 bits; codeword rows of 3 bytes
    "dense-moon-ntx17": (67, lambda hip, B: _dense_moon(hip, B, 17)),                   # a ragged last codeword byte
    "qc-jpl1024": (67, _qc_jpl1024),                                                     # its G.q, punctured n_tx = 1280: rows of 40 words
    "sparse-moon-chunk": (16384 + 33, _sparse_moon),                                     # crosses the 16 384-frame chunk of the scratch
    "sparse-dvbs2-short": (67, lambda hip, B: _sparse(hip, B, *dvbs2_short.csr(), dvbs2_short.N)),      # k = 7200, rows of 2025 bytes
    "sparse-toy-k48": (67, lambda hip, B: _sparse(hip, B, *sparse_spec.toy_decodable(70, 48))),         # k % 32 = 16: a 16-byte last word
    "systematic-1920": (67, lambda hip, B: _systematic(hip, B, "1920.1280.3.303")),      # parity positions among the message positions
    "systematic-40x90": (67, lambda hip, B: _systematic(hip, B, "40x90")),               # k = 55; rows of 12 bytes: word stores
}


def _messages(k, B, seed):
    """numpy-drawn messages, with the all-ones message and the unit messages e_0, e_31, e_32, e_{k-1} (where they exist) in front"""
    msg = np.random.default_rng(seed).integers(0, 2, (B, k)).astype(np.uint8)
    msg[0] = 1
    units = [i for i in dict.fromkeys((0, 31, 32, k - 1)) if i < k]
    for r, i in enumerate(units, start=1):
        if r < B:
            msg[r] = 0
            msg[r, i] = 1
    return msg


class Dev:
    """torch buffers with a guard row"""

    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)

    def full(self, rows, cols, fill, dtype):
        return self.torch.full((rows + 1, cols), fill, dtype=dtype, device=self.dev)

    def put(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def put_at_offset(self, a, off):
        """(tensor that owns the memory, device pointer off bytes past a 256-byte boundary) holding the bytes of a"""
        flat = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        t = self.torch.zeros(flat.size + off, dtype=self.torch.uint8, device=self.dev)
        t[off:] = self.torch.from_numpy(flat).to(self.dev)
        assert t.data_ptr() % 256 == 0
        return t, t.data_ptr() + off

    def sync(self):
        self.torch.cuda.synchronize()

    def get(self, t, rows, fill):
        """the first `rows` rows on the host; the guard row must still hold `fill`"""
        self.sync()
        a = t.cpu().numpy()
        assert (a[rows:] == fill).all(), "a row past the batch was written"
        return a[:rows]


def _encode(d, src, B, msg_t, msg_fmt, cw_fmt, msg_ptr=None):
    torch = d.torch
    cols = src.n_tx if cw_fmt == "bytes" else bitspec.codeword_row_bytes(src.n_tx)
    out = d.full(B, cols, 7, torch.uint8)
    d.sync()
    src.sim.encode_messages(B, msg_ptr if msg_ptr is not None else msg_t.data_ptr(), out.data_ptr(), msg_fmt, cw_fmt, None)
    return d.get(out, B, 7)


@pytest.mark.parametrize("case", list(CASES))
def test_source(hip, case):
    B, make = CASES[case]
    src = make(hip, B)
    sim, k, n_tx, N = src.sim, src.k, src.n_tx, src.N
    d = Dev()
    torch = d.torch
    mp, pp = sim.positions()
    print(f"{case}: {src.kind} N={N} k={k} n_tx={n_tx} batch={B}")

    # ---- 1. replay against the kernels of ldpc_sim_encode_batch / ldpc_sim_generate / _f16
    cw0, m0 = d.full(B, n_tx, 7, torch.uint8), d.full(B, k, 9, torch.uint8)
    l0, m1 = d.full(B, N, 777.0, torch.float32), d.full(B, k, 9, torch.uint8)
    h0 = d.full(B, N, 777.0, torch.float16)
    d.sync()
    sim.encode_batch(SEED, FIRST, B, cw0.data_ptr(), m0.data_ptr(), None)
    sim.generate(SEED, FIRST, B, 2.0, l0.data_ptr(), m1.data_ptr(), None)
    sim.generate(SEED, FIRST, B, 2.0, h0.data_ptr(), None, None, llr_f16=True)
    drawn = d.get(m0, B, 9)
    assert np.array_equal(d.get(m1, B, 9), drawn) and drawn.max() == 1 and 0.3 < drawn.mean() < 0.7
    cw1 = _encode(d, src, B, m0, "bytes", "bytes")
    assert np.array_equal(cw1, d.get(cw0, B, 7)), "replayed codeword bytes differ"
    l1, h1 = d.full(B, N, 777.0, torch.float32), d.full(B, N, 777.0, torch.float16)
    d.sync()
    sim.generate_from(SEED, FIRST, B, 2.0, m0.data_ptr(), l1.data_ptr(), "bytes", None)
    sim.generate_from(SEED, FIRST, B, 2.0, m0.data_ptr(), h1.data_ptr(), "bytes", None, llr_f16=True)
    a, b = d.get(l0, B, 777.0), d.get(l1, B, 777.0)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "replayed float32 LLRs differ"
    assert (b[:, n_tx:].view(np.uint32) == 0).all() and (b[:, :n_tx] != 0).all()
    a, b = d.get(h0, B, 777.0), d.get(h1, B, 777.0)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16)), "replayed fp16 LLRs differ"
    assert (b[:, n_tx:].view(np.uint16) == 0).all()
    del cw0, l0, h0, l1, h1, m1

    # ---- 2. independent messages against the CPU restatement
    msg = _messages(k, B, seed=len(case) * 1000 + k)
    msg_t = d.put(msg)
    cw = _encode(d, src, B, msg_t, "bytes", "bytes")
    assert cw.max() <= 1
    sample = np.arange(B) if B <= 256 else np.unique(np.concatenate([[0, 1, 2, 3, 4, 16383, 16384, B - 1],
                                                                       np.random.default_rng(5).choice(B, 56, replace=False)]))[:64]
    if B > 256:
        assert len(sample) == 64 and {16383, 16384, B - 1} <= set(sample.tolist())
    want = src.restate(msg[sample])
    assert want.shape == (len(sample), n_tx) and np.array_equal(cw[sample], want), "codewords differ from the CPU restatement"
    assert np.array_equal(np.pad(cw, ((0, 0), (0, N - n_tx)))[:, mp], msg) if n_tx == N else np.array_equal(cw[:, mp[mp < n_tx]], msg[:, mp < n_tx])
    if n_tx == N and src.syndrome is not None:
        assert not src.syndrome(cw[sample]).any(), "H c != 0"

    # ---- 3. formats
    packed_msg = bitspec.pack_messages(msg)
    want_packed = np.packbits(cw, axis=1, bitorder="little")
    assert want_packed.shape[1] == bitspec.codeword_row_bytes(n_tx) and np.array_equal(want_packed, bitspec.pack_codewords(cw))
    pm_t = d.put(packed_msg)
    assert np.array_equal(_encode(d, src, B, pm_t, "packed", "bytes"), cw), "packed messages in"
    assert np.array_equal(_encode(d, src, B, msg_t, "bytes", "packed"), want_packed), "packed codewords out"
    assert np.array_equal(_encode(d, src, B, pm_t, "packed", "packed"), want_packed), "packed in, packed out"
    if k % 32:
        dirty = packed_msg.copy().view("<u4")
        dirty[:, -1] |= np.uint32((0xFFFFFFFF << (k % 32)) & 0xFFFFFFFF)
        assert not np.array_equal(dirty.view(np.uint8), packed_msg)
        assert np.array_equal(_encode(d, src, B, d.put(dirty.view(np.uint8)), "packed", "packed"), want_packed), "pad bits of the last message word"
    junk = np.random.default_rng(7).choice(np.array([0, 2, 254], np.uint8), size=msg.shape)
    loud = msg | junk
    assert {2, 3, 254, 255} <= set(np.unique(loud).tolist())
    assert np.array_equal(_encode(d, src, B, d.put(loud), "bytes", "bytes"), cw), "only bit 0 of a message byte counts"
    # message bytes one byte off a 16-byte boundary (the byte loads where k % 16 = 0), and packed codewords to such an address
    keep, p = d.put_at_offset(loud, 1)
    assert np.array_equal(_encode(d, src, B, None, "bytes", "bytes", msg_ptr=p), cw), "unaligned message bytes"
    PB = bitspec.codeword_row_bytes(n_tx)
    flat = torch.full(((B + 1) * PB + 1,), 7, dtype=torch.uint8, device=d.dev)
    d.sync()
    sim.encode_messages(B, msg_t.data_ptr(), flat.data_ptr() + 1, "bytes", "packed", None)
    d.sync()
    fl = flat.cpu().numpy()
    assert fl[0] == 7 and (fl[1 + B * PB:] == 7).all() and np.array_equal(fl[1:1 + B * PB].reshape(B, PB), want_packed), "unaligned packed codewords"
    del keep, flat

    # ---- 4. tally: the caller's messages are what is compared against
    llr = d.full(B, N, 777.0, torch.float32)
    d.sync()
    sim.generate_from(SEED, FIRST, B, 40.0, pm_t.data_ptr(), llr.data_ptr(), "packed", None)
    l40 = d.get(llr, B, 777.0)
    assert (l40[:, n_tx:] == 0).all() and np.array_equal((l40[:, :n_tx] > 0).astype(np.uint8), cw) and (np.abs(l40[:, :n_tx]) > 1.0).all()
    bits = np.zeros((B, N), np.uint8)
    bits[:, :n_tx] = cw
    bits[:, mp] = msg                                              # (message positions past n_tx, if any)
    flips = {0: [mp[0], mp[k - 1]], B // 2: [mp[k // 2]], B - 1: [mp[min(1, k - 1)]]}
    nbits = 0
    for f, cols in flips.items():
        for c in set(int(x) for x in cols):
            bits[f, c] ^= 1
            nbits += 1
    if len(pp):
        bits[1, pp[0]] ^= 1                                        # a parity position: not a message-bit error
    iters = (np.arange(B) % 5).astype(np.int32)

    def tally(bits_np):
        t = torch.zeros(4, dtype=torch.int64, device=d.dev)
        b_t, i_t = d.put(bits_np), d.put(iters)
        d.sync()
        sim.tally(B, b_t.data_ptr(), i_t.data_ptr(), t.data_ptr(), None)
        d.sync()
        return t.cpu().numpy().tolist()

    assert tally(bits) == [B, len(flips), nbits, int(iters.sum())]

    # ---- 5. round trip through an f32 min-sum decoder
    dec = hip.Decoder(src.code, "min", "f32", B)
    out, its, conv = d.full(B, N, 9, torch.uint8), torch.full((B + 1,), -1, dtype=torch.int32, device=d.dev), torch.full((B + 1,), 9, dtype=torch.uint8, device=d.dev)
    d.sync()
    dec.decode_batch_dev(llr.data_ptr(), out.data_ptr(), B, 20, its.data_ptr(), conv.data_ptr(), None)
    dec.synchronize()
    decoded = d.get(out, B, 9)
    if n_tx == N:
        assert (d.get(conv, B, 9) == 1).all() and (d.get(its, B, -1) == 0).all(), "a noiseless frame needed an iteration"
        assert np.array_equal(decoded, cw)
    assert tally(decoded) == [B, 0, 0, int(iters.sum())]
    back, backp = d.full(B, k, 9, torch.uint8), d.full(B, bitspec.message_row_bytes(k), 9, torch.uint8)
    d.sync()
    sim.extract_messages(B, out.data_ptr(), back.data_ptr(), "bytes", None)
    sim.extract_messages(B, out.data_ptr(), backp.data_ptr(), "packed", None)
    assert np.array_equal(d.get(back, B, 9), msg), "extracted message bytes"
    assert np.array_equal(d.get(backp, B, 9), packed_msg), "extracted packed messages"
    loud_bits = d.put(decoded | np.uint8(0xFE))                   # only bit 0 of a decoded byte is read
    d.sync()
    sim.extract_messages(B, loud_bits.data_ptr(), back.data_ptr(), "bytes", None)
    assert np.array_equal(d.get(back, B, 9), msg)
    dec.close()
    src.close()


def test_refusals(hip):
    import torch
    c = load("moon.7.13")
    code = hip.Code.from_csr(c.graph.row_ptr, c.graph.col_idx, c.N)
    dev = torch.device("cuda", 0)
    B = 4
    msg = torch.ones((B + 1, 7), dtype=torch.uint8, device=dev)
    cw = torch.full((B + 1, 20), 7, dtype=torch.uint8, device=dev)
    llr = torch.full((B + 1, 20), 777.0, dtype=torch.float32, device=dev)
    back = torch.full((B + 1, 7), 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def refused(code_, fn, *a, **kw):
        with pytest.raises(hip.LdpcError) as e:
            fn(*a, **kw)
        assert e.value.code == code_, str(e.value)
        return str(e.value)

    plain = hip.Sim(code, 7, 20, max_batch=B)
    assert plain.encoder == "none"
    assert "no encoder" in refused(-5, plain.encode_messages, B, msg.data_ptr(), cw.data_ptr())
    assert "no encoder" in refused(-5, plain.generate_from, 1, 0, B, 2.0, msg.data_ptr(), llr.data_ptr())
    bits = torch.zeros((B, 20), dtype=torch.uint8, device=dev)
    bits[:, 2] = 1
    torch.cuda.synchronize()
    plain.extract_messages(B, bits.data_ptr(), back.data_ptr())
    torch.cuda.synchronize()
    got = back.cpu().numpy()
    assert (got[B] == 9).all() and np.array_equal(got[:B], bits.cpu().numpy()[:, :7])
    plain.close()

    sim = hip.Sim(code, 7, 20, G=c.G, max_batch=B)
    m, w, l, k = msg.data_ptr(), cw.data_ptr(), llr.data_ptr(), back.data_ptr()
    for batch in (B + 1, 0, -1):
        refused(-1, sim.encode_messages, batch, m, w)
        refused(-1, sim.generate_from, 1, 0, batch, 2.0, m, l)
        refused(-1, sim.extract_messages, batch, w, k)
    for args in ((B, None, w), (B, m, None)):
        refused(-1, sim.encode_messages, *args)
    refused(-1, sim.generate_from, 1, 0, B, 2.0, None, l)
    refused(-1, sim.generate_from, 1, 0, B, 2.0, m, None)
    refused(-1, sim.extract_messages, B, None, k)
    refused(-1, sim.extract_messages, B, w, None)
    for fmt in (2, -1):
        refused(-1, sim.encode_messages, B, m, w, fmt, "bytes")
        refused(-1, sim.encode_messages, B, m, w, "bytes", fmt)
        refused(-1, sim.generate_from, 1, 0, B, 2.0, m, l, fmt)
        refused(-1, sim.extract_messages, B, w, k, fmt)
    refused(-1, sim.encode_messages, B, m + 1, w, "packed", "bytes")          # packed message rows are whole aligned words
    torch.cuda.synchronize()
    assert (cw.cpu().numpy() == 7).all() and (llr.cpu().numpy() == 777.0).all() and (back.cpu().numpy()[B] == 9).all()   # a refused call writes nothing
    sim.encode_messages(B, m, w)                                              # and the source still works
    torch.cuda.synchronize()
    got = cw.cpu().numpy()
    want = np.concatenate([np.ones(7, np.uint8), c.G.sum(0).astype(np.uint8) & 1])
    assert (got[B] == 7).all() and (got[:B] == want).all()
    sim.close(); code.close()
