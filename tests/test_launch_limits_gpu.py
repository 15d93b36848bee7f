"""GPU: the frame source and the chain around it past the limits of their launches -- the host-side forks that only a large call takes.

The rule every test asserts.  An entry point given a batch within its object's max_batch either writes exactly what the same entry point
writes when the batch is handed over in slices of at most 4096 frames (first_frame and the pointers advanced; compared bit for bit, whole
buffers, on the device), or refuses with LDPC_EINVAL in words that name the limit, before anything is written.  It never returns
LDPC_EHIP and never writes part of its output.  The 70 001-frame cases of test 1 must take the first branch.

The sliced calls are the reference for the bulk: the other files pin them to the CPU restatements at small batch, and replay across a
batch split is a tested property.  So that a large call is not judged against the same code alone, the frames 0, 16 383, 16 384, 65 535,
65 536 and the last one are also compared with the numpy specs directly, with each spec's own comparison: bit for bit, and for the noisy
LLRs and samples the 16 * 2^-24 units of tests/test_frame_source_gpu.py, tests/test_modulation_gpu.py and tests/test_fading_gpu.py.

  1. 70 001 frames (above the 65 536 the device reports as its largest gridDim.y, where sim_frame_kernel and pack_bits_kernel keep the
     frame; no multiple of 4, 32 or 64), first_frame = 2^32 - 3: every entry point of the frame source on one source per encoder, the
     modulated, interleaved and fading paths and the stand-alone demappers and table kernels on the dense source and the source
     without a generator, and the decoder's byte and packed results on moon.7.13.  Measured on MI355X: the runtime runs a grid of
     70 001 in y although the device reports 65 536, so these cases pass with one launch as with the slices of 65 536 the host makes;
     with slices that do not advance first_frame or the packed pointer, 9 of the 11 cases fail (all but the two of the generator-less
     source on the modulated path, whose codewords are zero and whose noise another kernel draws);
  2. the turns of the encoder from H (csrc/sim_sparse.hip: 16 384 frames a turn): one full turn, a second turn of one frame, two full
     turns and a ragged third of 33 frames, every frame against tests/sparse_encoder_spec.py and against the dense source of the
     implied generator;
  3. the second pass of the grid-stride loops (sim_grid, il_grid: 2^20 workgroups of 256) of the kernels whose item is one byte:
     deinterleave_llr in int8, interleave_bits, extract_messages to bytes, with 2^28 < items <= 2^28 + 2^20.  interleave_bits to packed
     rows takes its second pass from packed codewords: from bytes its input would be eight times the output, 2 GB; bytes to packed runs
     at the same batch as bytes to bytes, in one pass.  jpl.1024's k = 1024 makes batch * k a multiple of 256 whatever the batch: the
     ragged last workgroup of a second pass is the table kernels' to show.  The kernels whose item is a word (sim_load_bytes_kernel,
     sim_load_packed_kernel, sim_pack_codeword_kernel, the packed sim_extract_kernel) are left out: a second pass there needs buffers
     of several GB; they use the same loop shape;
  4. the stores of the sample and gain buffers the host grants (vec4: n_sym even and samples 16-byte aligned; vec2: n_sym even and gains
     8-byte aligned): samples at a 16-byte aligned pointer and 8 bytes past it, gains at an 8-byte aligned pointer and 4 bytes past it,
     n_sym even and odd -- identical bytes, nothing written outside them.
Every output buffer is pre-filled and carries one guard row past the batch."""
import numpy as np
import pytest

from oracle import frame_source as fsrc
from oracle import oracle
from tests import encode_messages_spec as bitspec
from tests import fading_spec as fs
from tests import interleaver_spec as ils
from tests import modulation_spec as ms
from tests import product_modulation_spec as ps
from tests import sparse_encoder_spec as sparse_spec
from tests import test_encode_messages_gpu as enc
from tests.helpers import load
from tests.test_fading_gpu import _source120, _source203, _source_table
from tests.test_modulation_gpu import TABLES, _same
from tests.test_product_modulation_gpu import _uneven
from tests.test_systematic_encoder_gpu import _qc_words

pytestmark = pytest.mark.gpu

B1 = 70001
SEED, FIRST = 0x5EEDB16BA7C4, 2 ** 32 - 3                        # the frame ids cross 2^32
SLICE = 4096
SAMPLED = (0, 16383, 16384, 65535, 65536, B1 - 1)
BOUND = 16.0                                                      # x 2^-24 units: the bar of the files named above
LIMIT_WORDS = ("more than one launch holds", "limit", "at most")   # the first: the words of the refusals the library has today
I8_QS = 2.5


class Dev:
    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.u8, self.i8, self.f32, self.f16, self.i32 = torch.uint8, torch.int8, torch.float32, torch.float16, torch.int32

    def full(self, rows, cols, fill, dtype):
        return self.torch.full((rows + 1, cols), fill, dtype=dtype, device=self.dev)

    def sync(self):
        self.torch.cuda.synchronize()

    def rows(self, t, idx):
        """the rows idx of a device tensor, on the host"""
        return t[self.torch.as_tensor(list(idx), device=self.dev)].cpu().numpy()

    def free(self):
        self.torch.cuda.empty_cache()


def at(t, f0):
    """the device pointer of row f0"""
    return t.data_ptr() + f0 * t.stride(0) * t.element_size()


def same_bits(a, b):
    """bit for bit (a NaN equals itself, -0 differs from +0)"""
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def run(hip, d, B, outs, call):
    """the rule.  outs: {name: (cols, dtype, fill)}; call(f0, n, ptr): the entry point on frames f0 .. f0 + n - 1, ptr(name) = where row f0
    of that output goes.  -> {name: tensor [B + 1][cols]} of the whole call, or None if it was refused as the rule allows"""
    whole = {k: d.full(B, cols, fill, dt) for k, (cols, dt, fill) in outs.items()}
    sliced = {k: d.full(B, cols, fill, dt) for k, (cols, dt, fill) in outs.items()}
    d.sync()
    try:
        call(0, B, lambda name: whole[name].data_ptr())
    except hip.LdpcError as e:
        d.sync()
        assert e.code == hip.EINVAL, f"a batch of {B} within max_batch failed with code {e.code}: {e}"
        assert any(w in str(e) for w in LIMIT_WORDS), f"the refusal does not name a limit: {e}"
        for k, (_, _, fill) in outs.items():
            assert bool((whole[k] == fill).all()), f"{k}: a refused call wrote"
        return None
    for f0 in range(0, B, SLICE):
        call(f0, min(SLICE, B - f0), lambda name, f0=f0: at(sliced[name], f0))
    d.sync()
    for k, (_, _, fill) in outs.items():
        assert bool((whole[k][B] == fill).all()), f"{k}: the row past the batch was written"
        assert same_bits(whole[k], sliced[k]), f"{k}: {B} frames in one call differ from slices of {SLICE}"
    return whole


def pack_rows(d, t, row_bytes):
    """[R][n] bytes (bit 0 of each) -> [R][row_bytes] packed, LSB first, pad bits 0: LDPC_BITS_PACKED, on the device"""
    torch = d.torch
    R, n = t.shape
    p = torch.zeros((R, row_bytes * 8), dtype=torch.uint8, device=d.dev)
    p[:, :n] = t & 1
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=d.dev)
    return (p.view(R, row_bytes, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


def with_guard(d, t, fill):
    """t [B][cols] -> [B + 1][cols], the guard row filled"""
    out = d.torch.full((t.shape[0] + 1, t.shape[1]), fill, dtype=t.dtype, device=d.dev)
    out[:-1] = t
    return out


# ---- 1. the sources
class Src:
    def __init__(self, sim, code, N, n_tx, restate, owners, drawn=True):
        self.sim, self.code, self.N, self.n_tx, self.k, self.restate, self.owners, self.drawn = sim, code, N, n_tx, sim.k, restate, owners, drawn

    def messages(self, ids):
        """the spec's messages of these frames (a source without a generator draws none: zeros)"""
        ids = np.asarray(ids, dtype=np.uint64)
        return fsrc.message_bits(SEED, ids, self.k) if self.drawn else np.zeros((len(ids), self.k), np.uint8)

    def close(self):
        for o in self.owners:
            o.close()


def _dense_restate(G, n_tx):
    G = G.astype(np.int64)
    return lambda m: np.concatenate([m, ((m.astype(np.int64) @ G) & 1).astype(np.uint8)], axis=1)[:, :n_tx]


def _from_fading(s):
    return Src(s.sim, s.code, s.N, s.n_tx, _dense_restate(s.G, s.n_tx), s.owners)


def _none203(hip, B):
    s = _source203(hip, B, generator=False)
    assert s.sim.encoder == "none"
    return Src(s.sim, s.code, s.N, s.n_tx, lambda m: np.zeros((len(m), s.n_tx), np.uint8), s.owners, drawn=False)


def _from_enc(s):
    return Src(s.sim, s.code, s.N, s.n_tx, s.restate, s.owners)


def _qc_small(hip, B):
    """circulants of 32, 3 block rows, 2 block columns: k = 96, N = 160, n_tx = 153 cuts into the last parity word"""
    sz, brows, bcols = 32, 3, 2
    words = np.random.default_rng(3232).integers(0, 2 ** 32, size=(brows, bcols, 1), dtype=np.uint64).astype(np.uint32)
    gbits = ((words[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.uint8).reshape(brows, bcols, sz)
    k, N, n_tx = sz * brows, sz * (brows + bcols), sz * (brows + bcols) - 7
    code = hip.Code.from_csr(np.array([0, 2], np.int32), np.array([0, 1], np.int32), N)      # the source needs only N
    sim = hip.Sim(code, k, n_tx, max_batch=B, G_qc=(sz, words))
    assert sim.encoder == "qc"
    return Src(sim, code, N, n_tx, lambda m: np.stack([np.concatenate([r, oracle.encode_qc(sz, gbits, r)]) for r in m])[:, :n_tx], (sim, code))


SOURCES = {
    "dense203": lambda hip, B: _from_fading(_source203(hip, B)),
    "dense120": lambda hip, B: _from_fading(_source120(hip, B)),
    "none203": _none203,
    "sparse-moon": lambda hip, B: _from_enc(enc._sparse_moon(hip, B)),
    "systematic-40x90": lambda hip, B: _from_enc(enc._systematic(hip, B, "40x90")),
    "qc-32x3x2": _qc_small,
}


def _check_llrs(what, got, src, ids, cw, db):
    ref, rad, sg, sc = fsrc.llrs(SEED, ids, cw, src.k, src.n_tx, src.N, db)
    assert got.dtype == np.float32 and np.isfinite(got).all() and not got[:, src.n_tx:].view(np.uint32).any(), what
    mult = np.abs(got[:, :src.n_tx].astype(np.float64) - ref[:, :src.n_tx]) / (2.0 ** -24 * sc * (1.0 + sg * rad))
    print(f"{what}: worst LLR error {mult.max():.2f} x 2^-24 sc (1 + sg ra) (bound {BOUND:g})")
    assert mult.max() <= BOUND, (what, float(mult.max()))


@pytest.mark.parametrize("name", list(SOURCES))
def test_frame_source_past_the_y_grid_limit(hip, name):
    B = B1
    d = Dev()
    torch = d.torch
    src = SOURCES[name](hip, B)
    sim, N, n_tx, k = src.sim, src.N, src.n_tx, src.k
    mp, pp = sim.positions()
    ids = np.uint64(FIRST) + np.array(SAMPLED, dtype=np.uint64)
    want_msg = src.messages(ids)
    want_cw = src.restate(want_msg)
    assert want_cw.shape == (len(SAMPLED), n_tx)
    db = 2.0

    # ldpc_sim_encode_batch
    r = run(hip, d, B, {"cw": (n_tx, d.u8, 7), "msg": (k, d.u8, 9)}, lambda f0, n, p: sim.encode_batch(SEED, FIRST + f0, n, p("cw"), p("msg"), None))
    assert r is not None, "ldpc_sim_encode_batch refused 70 001 frames"
    cw, msg = r["cw"], r["msg"]
    assert np.array_equal(d.rows(msg, SAMPLED), want_msg) and np.array_equal(d.rows(cw, SAMPLED), want_cw), "encode_batch against the spec"
    # ldpc_sim_generate, float32 and fp16
    r = run(hip, d, B, {"llr": (N, d.f32, 777.0), "msg": (k, d.u8, 9)}, lambda f0, n, p: sim.generate(SEED, FIRST + f0, n, db, p("llr"), p("msg"), None))
    assert r is not None, "ldpc_sim_generate refused 70 001 frames"
    llr = r["llr"]
    assert torch.equal(r["msg"], msg)
    _check_llrs(f"{name} generate", d.rows(llr, SAMPLED), src, ids, want_cw, db)
    r = run(hip, d, B, {"llr": (N, d.f16, 777.0), "msg": (k, d.u8, 9)},
            lambda f0, n, p: sim.generate(SEED, FIRST + f0, n, db, p("llr"), p("msg"), None, llr_f16=True))
    assert r is not None, "ldpc_sim_generate_f16 refused 70 001 frames"
    llr16 = r["llr"]
    assert torch.equal(r["msg"], msg) and same_bits(llr16[:B], llr[:B].clamp(-65504.0, 65504.0).to(torch.float16)), "fp16 = the float32 values rounded"
    assert np.array_equal(d.rows(llr16, SAMPLED).view(np.uint16), ms.round_f16(d.rows(llr, SAMPLED)).view(np.uint16))

    kw, PB = (k + 31) // 32, bitspec.codeword_row_bytes(n_tx)
    assert bitspec.message_row_bytes(k) == 4 * kw
    msg_p = with_guard(d, pack_rows(d, msg[:B], 4 * kw), 9)
    assert np.array_equal(d.rows(msg_p, SAMPLED), bitspec.pack_messages(want_msg))
    if sim.encoder != "none":
        # ldpc_sim_encode_messages, both formats both ways; ldpc_sim_generate_from
        cw_p = pack_rows(d, cw[:B], PB)
        assert np.array_equal(d.rows(cw_p, SAMPLED), bitspec.pack_codewords(want_cw))
        for mf, m_t in (("bytes", msg), ("packed", msg_p)):
            for cf, cols, want in (("bytes", n_tx, cw[:B]), ("packed", PB, cw_p)):
                r = run(hip, d, B, {"cw": (cols, d.u8, 7)}, lambda f0, n, p: sim.encode_messages(n, at(m_t, f0), p("cw"), mf, cf, None))
                assert r is not None, f"ldpc_sim_encode_messages {mf} -> {cf} refused 70 001 frames"
                assert torch.equal(r["cw"][:B], want), f"encode_messages {mf} -> {cf} differs from encode_batch"
                assert np.array_equal(d.rows(r["cw"], SAMPLED), want_cw if cf == "bytes" else bitspec.pack_codewords(want_cw)), (mf, cf, "against the spec")
            for f16, ref, dt in ((False, llr, d.f32), (True, llr16, d.f16)):
                r = run(hip, d, B, {"llr": (N, dt, 777.0)},
                        lambda f0, n, p: sim.generate_from(SEED, FIRST + f0, n, db, at(m_t, f0), p("llr"), mf, None, llr_f16=f16))
                assert r is not None, "ldpc_sim_generate_from refused 70 001 frames"
                assert same_bits(r["llr"], ref), f"generate_from {mf} f16={f16} differs from generate"
                if not f16:
                    _check_llrs(f"{name} generate_from {mf}", d.rows(r["llr"], SAMPLED), src, ids, want_cw, db)
        del cw_p

    # decoded bytes [B][N]: the codeword, the message at its positions, errors in every 7th frame (a message bit) and 5th (a parity bit)
    mp_t = torch.as_tensor(mp.astype(np.int64), device=d.dev)
    bits = torch.zeros((B + 1, N), dtype=torch.uint8, device=d.dev)
    bits[:B, :n_tx] = cw[:B]
    bits[:B, mp_t] = msg[:B]
    f = torch.arange(B, device=d.dev)
    hit = f[f % 7 == 0]
    bits[hit, mp_t[hit % k]] ^= 1
    if len(pp):
        hit5 = f[f % 5 == 0]
        bits[hit5, int(pp[0])] ^= 1
    # ldpc_sim_extract_messages, bytes and packed
    want_back = bits[:B][:, mp_t]
    r = run(hip, d, B, {"m": (k, d.u8, 9)}, lambda f0, n, p: sim.extract_messages(n, at(bits, f0), p("m"), "bytes", None))
    assert r is not None and torch.equal(r["m"][:B], want_back), "extract_messages, bytes"
    assert np.array_equal(d.rows(r["m"], SAMPLED), d.rows(bits, SAMPLED)[:, mp])
    r = run(hip, d, B, {"m": (4 * kw, d.u8, 9)}, lambda f0, n, p: sim.extract_messages(n, at(bits, f0), p("m"), "packed", None))
    assert r is not None and torch.equal(r["m"][:B], pack_rows(d, want_back, 4 * kw)), "extract_messages, packed"
    assert np.array_equal(d.rows(r["m"], SAMPLED), bitspec.pack_messages(d.rows(bits, SAMPLED)[:, mp]))
    # ldpc_sim_tally against a recount on the device: the messages are those of the source's last call
    iters = (torch.arange(B + 1, device=d.dev) % 5).to(torch.int32).reshape(B + 1, 1)
    wrong = want_back != msg[:B]
    recount = [B, int(wrong.any(1).sum()), int(wrong.sum()), int(iters[:B].sum())]
    assert recount[1] == (B + 6) // 7 == recount[2]
    t_whole, t_sliced = torch.zeros(4, dtype=torch.int64, device=d.dev), torch.zeros(4, dtype=torch.int64, device=d.dev)
    scratch = d.full(B, n_tx, 7, d.u8)
    d.sync()
    sim.encode_batch(SEED, FIRST, B, scratch.data_ptr(), None, None)
    sim.tally(B, bits.data_ptr(), iters.data_ptr(), t_whole.data_ptr(), None)
    for f0 in range(0, B, SLICE):
        n = min(SLICE, B - f0)
        sim.encode_batch(SEED, FIRST + f0, n, at(scratch, f0), None, None)
        sim.tally(n, at(bits, f0), at(iters, f0), t_sliced.data_ptr(), None)
    d.sync()
    assert t_whole.cpu().numpy().tolist() == recount and t_sliced.cpu().numpy().tolist() == recount
    assert torch.equal(scratch, cw)
    src.close()
    d.free()


# ---- 1. the modulated path, the demappers and the table kernels
class Obj:
    """the 16QAM table object (m = 4) or a product object of b bits an axis, with the specs' demappers for it"""

    def __init__(self, hip, kind, b=None):
        self.kind = kind
        if kind == "table":
            self.pts, self.m = TABLES["16qam"](), 4
            self.mod = hip.Modulation(self.pts)
            self.demap = lambda sym, n_tx, N, nv, fmt, qs: ms.demap(self.pts, sym, n_tx, N, nv, fmt, qs)
            self.demap_il = lambda sym, pos, N, nv, fmt, qs: ils.demap_il(self.pts, sym, pos, N, nv, fmt, qs)
            self.demap_csi = lambda sym, a, pos, N, nv, fmt, qs: fs.demap_il_csi(self.pts, sym, a, pos, N, nv, fmt, qs)
        else:
            li, lq = _uneven(b, 60 + b), (_uneven(b, 70 + b) * np.float32(0.6)).astype(np.float32)
            self.pts, self.m = ps.materialise(li, lq), 2 * b
            self.mod = hip.Modulation.product(li, lq)
            self.demap = lambda sym, n_tx, N, nv, fmt, qs: ps.demap(li, lq, sym, n_tx, N, nv, fmt, qs)
            self.demap_il = lambda sym, pos, N, nv, fmt, qs: ils.demap_il_product(li, lq, sym, pos, N, nv, fmt, qs)
            self.demap_csi = lambda sym, a, pos, N, nv, fmt, qs: fs.demap_il_csi_product(li, lq, sym, a, pos, N, nv, fmt, qs)
        assert self.mod.bits == self.m


FMTS = (("f32", ms.LLR_F32, 0.0), ("i8", ms.LLR_I8, I8_QS))


def _units(what, got, want, unit):
    err = np.abs(got.astype(np.float64) - want) / (2.0 ** -24 * unit)
    print(f"{what}: worst error {float(err.max()):.2f} x 2^-24 units (bound {BOUND:g})")
    assert err.max() <= BOUND, (what, float(err.max()))


@pytest.mark.parametrize("kind,b", [("table", None), ("product", 3)], ids=["16qam", "product-3"])
@pytest.mark.parametrize("name", ["dense203", "none203"])
def test_modulated_path_past_the_y_grid_limit(hip, name, kind, b):
    B = B1
    d = Dev()
    torch = d.torch
    src = SOURCES[name](hip, B)
    sim, N, n_tx, k = src.sim, src.N, src.n_tx, src.k
    o = Obj(hip, kind, b)
    mod, m = o.mod, o.m
    ns = mod.symbols(n_tx)
    pos = _source_table(src, m)
    il = hip.Interleaver(pos, N)
    fad, block, K = hip.Fading(3, 4.0), 3, 4.0
    db = 6.0
    nv = sim.noise_var(mod, db)
    ids = np.uint64(FIRST) + np.array(SAMPLED, dtype=np.uint64)
    want_msg = src.messages(ids)
    want_cw = src.restate(want_msg)
    want_tx = ils.interleave(want_cw, pos)
    ones = np.ones((len(SAMPLED), ns), np.float32)
    dt_of = {"f32": d.f32, "i8": d.i8}
    fill_of = {"f32": 777.0, "i8": 99}

    def sampled_sym(t):
        return d.rows(t, SAMPLED).reshape(len(SAMPLED), ns, 2)

    # ldpc_sim_transmit, ldpc_sim_generate_mod, ldpc_demap_dev
    r = run(hip, d, B, {"sym": (2 * ns, d.f32, 777.0), "msg": (k, d.u8, 9)},
            lambda f0, n, p: sim.transmit(mod, SEED, FIRST + f0, n, db, p("sym"), None, "bytes", p("msg"), None))
    assert r is not None, "ldpc_sim_transmit refused 70 001 frames"
    sym = r["sym"]
    assert np.array_equal(d.rows(r["msg"], SAMPLED), want_msg)
    want, unit, _ = fs.transmit(o.pts, m, SEED, ids, want_cw, nv, ones)
    _units(f"{name} transmit", sampled_sym(sym), want, unit)
    for fmt, code, qs in FMTS:
        outs = {"llr": (N, dt_of[fmt], fill_of[fmt])}
        r = run(hip, d, B, outs, lambda f0, n, p: sim.generate_mod(mod, SEED, FIRST + f0, n, db, p("llr"), fmt, qs, None, "bytes", None, None))
        assert r is not None, "ldpc_sim_generate_mod refused 70 001 frames"
        r2 = run(hip, d, B, outs, lambda f0, n, p: hip.demap(mod, n, n_tx, N, at(sym, f0), nv, p("llr"), fmt, qs, None))
        assert r2 is not None and same_bits(r["llr"], r2["llr"]), f"generate_mod {fmt} is not demap(transmit)"
        _same(d.rows(r["llr"], SAMPLED), o.demap(sampled_sym(sym), n_tx, N, nv, code, qs or 4.0), (name, "generate_mod", fmt))
    # the same through the table; ldpc_deinterleave_llr_dev of the demapper's LLRs in transmitted order
    r = run(hip, d, B, {"sym": (2 * ns, d.f32, 777.0)}, lambda f0, n, p: sim.transmit_il(mod, il, SEED, FIRST + f0, n, db, p("sym"), None, "bytes", None, None))
    assert r is not None, "ldpc_sim_transmit_il refused 70 001 frames"
    sym_il = r["sym"]
    want, unit, _ = fs.transmit(o.pts, m, SEED, ids, want_tx, nv, ones)
    _units(f"{name} transmit_il", sampled_sym(sym_il), want, unit)
    for fmt, code, qs in FMTS:
        outs = {"llr": (N, dt_of[fmt], fill_of[fmt])}
        r = run(hip, d, B, outs, lambda f0, n, p: sim.generate_mod_il(mod, il, SEED, FIRST + f0, n, db, p("llr"), fmt, qs, None, "bytes", None, None))
        assert r is not None, "ldpc_sim_generate_mod_il refused 70 001 frames"
        r2 = run(hip, d, B, outs, lambda f0, n, p: hip.demap_il(mod, il, n, at(sym_il, f0), nv, p("llr"), fmt, qs, None))
        assert r2 is not None and same_bits(r["llr"], r2["llr"]), f"generate_mod_il {fmt} is not demap_il(transmit_il)"
        _same(d.rows(r["llr"], SAMPLED), o.demap_il(sampled_sym(sym_il), pos, N, nv, code, qs or 4.0), (name, "generate_mod_il", fmt))
        tx_llr = d.full(B, n_tx, fill_of[fmt], dt_of[fmt])
        d.sync()
        hip.demap(mod, B, n_tx, n_tx, sym_il.data_ptr(), nv, tx_llr.data_ptr(), fmt, qs, None)
        r3 = run(hip, d, B, outs, lambda f0, n, p: hip.deinterleave_llr(il, n, at(tx_llr, f0), p("llr"), fmt, None))
        assert r3 is not None and same_bits(r3["llr"], r["llr"]), f"deinterleave_llr {fmt} of demap is not demap_il"
        _same(d.rows(r3["llr"], SAMPLED), ils.deinterleave(d.rows(tx_llr, SAMPLED), pos, N), (name, "deinterleave_llr", fmt))
        del tx_llr
    # the fading channel
    r = run(hip, d, B, {"sym": (2 * ns, d.f32, 777.0), "gain": (ns, d.f32, 555.0)},
            lambda f0, n, p: sim.transmit_il_fading(mod, il, fad, SEED, FIRST + f0, n, db, p("sym"), p("gain"), None, "bytes", None, None))
    assert r is not None, "ldpc_sim_transmit_il_fading refused 70 001 frames"
    sym_f, gain = r["sym"], r["gain"]
    want_a, unit_a = fs.gains(SEED, ids, ns, block, K)
    _units(f"{name} gains", d.rows(gain, SAMPLED), want_a, unit_a)
    want, unit, _ = fs.transmit(o.pts, m, SEED, ids, want_tx, nv, want_a, unit_a)
    _units(f"{name} transmit_il_fading", sampled_sym(sym_f), want, unit)
    for fmt, code, qs in FMTS:
        outs = {"llr": (N, dt_of[fmt], fill_of[fmt])}
        r = run(hip, d, B, dict(outs, gain=(ns, d.f32, 555.0)),
                lambda f0, n, p: sim.generate_mod_il_fading(mod, il, fad, SEED, FIRST + f0, n, db, p("llr"), fmt, qs, p("gain"), None, "bytes", None, None))
        assert r is not None, "ldpc_sim_generate_mod_il_fading refused 70 001 frames"
        assert same_bits(r["gain"], gain), "the gains of generate_mod_il_fading are not those of transmit_il_fading"
        r2 = run(hip, d, B, outs, lambda f0, n, p: hip.demap_il_csi(mod, il, n, at(sym_f, f0), at(gain, f0), nv, p("llr"), fmt, qs, None))
        assert r2 is not None and same_bits(r["llr"], r2["llr"]), f"generate_mod_il_fading {fmt} is not demap_il_csi(transmit_il_fading)"
        _same(d.rows(r["llr"], SAMPLED), o.demap_csi(sampled_sym(sym_f), d.rows(gain, SAMPLED), pos, N, nv, code, qs or 4.0), (name, "generate_mod_il_fading", fmt))
    # ldpc_interleave_bits_dev on the codewords, rows of N bytes
    cw = d.full(B, n_tx, 7, d.u8)
    d.sync()
    sim.encode_batch(SEED, FIRST, B, cw.data_ptr(), None, None)
    cwN = torch.zeros((B + 1, N), dtype=torch.uint8, device=d.dev)
    cwN[:B, :n_tx] = cw[:B] | 0xFE                                 # only bit 0 of a byte is read
    d.sync()
    assert np.array_equal(d.rows(cw, SAMPLED), want_cw)
    for fo, cols, want in (("bytes", n_tx, want_tx), ("packed", (n_tx + 7) // 8, ils.pack(want_tx))):
        r = run(hip, d, B, {"tx": (cols, d.u8, 0x5A)}, lambda f0, n, p: hip.interleave_bits(il, n, at(cwN, f0), p("tx"), "bytes", fo, None))
        assert r is not None and np.array_equal(d.rows(r["tx"], SAMPLED), want), f"interleave_bits bytes -> {fo}"
    il.close(); mod.close()
    src.close()
    d.free()


def test_decoder_results_past_the_y_grid_limit(hip):
    """ldpc_decode_batch_dev and ldpc_decode_batch_dev_packed (pack_bits_kernel keeps the frame in blockIdx.y) on moon.7.13, min-sum, 5
    iterations, 12 dB: packed = the bytes packed, both = their sliced calls, the sampled frames = the oracle's"""
    B = B1
    d = Dev()
    c = load("moon.7.13")
    src = _from_enc(enc._sparse_moon(hip, B))
    N = src.N
    PB = (N + 7) // 8
    llr = d.full(B, N, 777.0, d.f32)
    d.sync()
    src.sim.generate(SEED, FIRST, B, 12.0, llr.data_ptr(), None, None)
    d.sync()
    dec = hip.Decoder(src.code, "min", "f32", B)

    def unpacked(f0, n, p):
        dec.decode_batch_dev(at(llr, f0), p("bits"), n, 5, p("its"), p("conv"), None)
        dec.synchronize()

    def packed(f0, n, p):
        dec.decode_batch_dev_packed(at(llr, f0), p("bits"), n, 5, p("its"), p("conv"), None)
        dec.synchronize()

    a = run(hip, d, B, {"bits": (N, d.u8, 9), "its": (1, d.i32, -1), "conv": (1, d.u8, 9)}, unpacked)
    assert a is not None, "ldpc_decode_batch_dev refused 70 001 frames"
    b = run(hip, d, B, {"bits": (PB, d.u8, 9), "its": (1, d.i32, -1), "conv": (1, d.u8, 9)}, packed)
    assert b is not None, "ldpc_decode_batch_dev_packed refused 70 001 frames"
    assert d.torch.equal(b["bits"][:B], pack_rows(d, a["bits"][:B], PB)), "packed results are not the bytes packed"
    assert d.torch.equal(a["its"], b["its"]) and d.torch.equal(a["conv"], b["conv"])
    obits, _, oconv = oracle.decode_batch(c.graph, "min", 5, d.rows(llr, SAMPLED))
    assert np.array_equal(d.rows(a["bits"], SAMPLED), obits) and np.array_equal(d.rows(a["conv"], SAMPLED)[:, 0] != 0, oconv != 0)
    assert np.array_equal(d.rows(b["bits"], SAMPLED), np.packbits(obits, axis=1, bitorder="little"))
    ids = np.uint64(FIRST) + np.array(SAMPLED, dtype=np.uint64)
    assert np.array_equal(obits, src.restate(src.messages(ids))), "12 dB: the sampled frames decode to their codewords"
    dec.close()
    src.close()
    d.free()


# ---- 2. the turns of the encoder from H
def _turn_outputs(d, sim, B, N, K, n_tx, first):
    """-> device tensors (codewords, messages, float32 LLRs at 40 dB) of B frames, the guard rows checked"""
    cw, msg, llr, msg2 = d.full(B, n_tx, 7, d.u8), d.full(B, K, 9, d.u8), d.full(B, N, 777.0, d.f32), d.full(B, K, 9, d.u8)
    d.sync()
    sim.encode_batch(SEED, first, B, cw.data_ptr(), msg.data_ptr(), None)
    sim.generate(SEED, first, B, 40.0, llr.data_ptr(), msg2.data_ptr(), None)
    d.sync()
    assert bool((cw[B] == 7).all()) and bool((msg[B] == 9).all()) and bool((llr[B] == 777.0).all()) and d.torch.equal(msg, msg2)
    return cw[:B], msg[:B], llr[:B]


@pytest.mark.parametrize("name", ["moon", "toy"])
def test_encoder_from_H_turns(hip, name):
    d = Dev()
    torch = d.torch
    if name == "moon":
        c = load("moon.7.13")
        rp, ci, N, K, n_tx, G = c.graph.row_ptr, c.graph.col_idx, c.N, 7, c.N, c.G
        order = sparse_spec.triangular_order(rp, ci, N)
    else:
        rp, ci, N = sparse_spec.toy(70, 45)
        K, n_tx = 45, N - 7
        order = sparse_spec.triangular_order(rp, ci, N)
        G = sparse_spec.encode(rp, ci, N, order, np.eye(K, dtype=np.uint8))[:, K:]      # the generator this H implies, row by row
    top, first = 32801, 2 ** 32 - 16390                                                # the ids cross 2^32 inside the second turn
    want_msg = fsrc.message_bits(SEED, np.uint64(first) + np.arange(top, dtype=np.uint64), K)
    want_cw = sparse_spec.encode(rp, ci, N, order, want_msg)[:, :n_tx]
    code = hip.Code.from_csr(rp, ci, N)
    dn = hip.Sim(code, K, n_tx, G=G, max_batch=top)
    assert dn.encoder == "dense"
    ref_cw, ref_msg, ref_llr = _turn_outputs(d, dn, top, N, K, n_tx, first)
    for max_batch, batches in ((16385, (16384, 16385)), (40000, (16384, 16385, top))):
        sim = hip.Sim(code, K, n_tx, from_H=True, max_batch=max_batch)
        assert sim.encoder == "sparse"
        for B in batches:
            cw, msg, llr = _turn_outputs(d, sim, B, N, K, n_tx, first)
            what = (name, max_batch, B)
            assert torch.equal(cw, ref_cw[:B]) and torch.equal(msg, ref_msg[:B]) and same_bits(llr, ref_llr[:B]), (what, "the dense source of the implied generator")
            l = llr.cpu().numpy()
            assert (l[:, n_tx:] == 0).all() and (np.abs(l[:, :n_tx]) > 1.0).all(), what
            assert np.array_equal(msg.cpu().numpy(), want_msg[:B]), (what, "messages")
            assert np.array_equal(cw.cpu().numpy(), want_cw[:B]), (what, "encode_batch against the spec")
            assert np.array_equal((l[:, :n_tx] > 0).astype(np.uint8), want_cw[:B]), (what, "generate at 40 dB against the spec")
        sim.close()
    dn.close(); code.close()
    d.free()


# ---- 3. the second pass of the grid-stride loops
TWO28 = 1 << 28


def _pattern(d, n, salt, dtype):
    """n elements of a counter-based pattern, every byte value, made in slices so that no int64 temporary of the full size is held"""
    torch = d.torch
    out = torch.empty(n, dtype=dtype, device=d.dev)
    step = 1 << 24
    for a in range(0, n, step):
        i = torch.arange(a, min(n, a + step), device=d.dev, dtype=torch.int64)
        h = (((i + salt) * 2654435761) >> 11) ^ (i >> 5) ^ i
        out[a:a + step] = ((h & 0xFF) - (128 if dtype == torch.int8 else 0)).to(dtype)
    return out


def _window(batch, row):
    total = batch * row
    assert TWO28 < total <= TWO28 + (1 << 20), (batch, row, total)
    return total


def _table4100():
    return np.random.default_rng(4100).permutation(4100)[:4001].astype(np.int32), 4100


def test_second_pass_deinterleave_llr_int8(hip):
    d = Dev()
    pos, N = _table4100()
    n_tx, B = len(pos), 65473
    assert _window(B, N) % 256 != 0
    il = hip.Interleaver(pos, N)
    x = _pattern(d, B * n_tx, 1, d.i8).reshape(B, n_tx)
    r = run(hip, d, B, {"llr": (N, d.i8, 99)}, lambda f0, n, p: hip.deinterleave_llr(il, n, at(x, f0), p("llr"), "i8", None))
    assert r is not None
    last = (0, B - 2, B - 1)                                        # the items of the second pass are in the last frame
    _same(d.rows(r["llr"], last), ils.deinterleave(d.rows(x, last), pos, N), "deinterleave_llr i8")
    del r, x
    il.close()
    d.free()


def test_second_pass_interleave_bits(hip):
    d = Dev()
    pos, N = _table4100()
    n_tx = len(pos)
    il = hip.Interleaver(pos, N)
    # bytes to bytes: an item is one transmitted bit; bytes to packed at the same batch, one pass
    B = 67093
    assert _window(B, n_tx) % 256 != 0
    x = _pattern(d, B * N, 2, d.u8).reshape(B, N)
    last = (0, B - 2, B - 1)
    want = ils.interleave(d.rows(x, last) & 1, pos)
    r = run(hip, d, B, {"tx": (n_tx, d.u8, 0x5A)}, lambda f0, n, p: hip.interleave_bits(il, n, at(x, f0), p("tx"), "bytes", "bytes", None))
    assert r is not None and np.array_equal(d.rows(r["tx"], last), want)
    del r
    r = run(hip, d, B, {"tx": ((n_tx + 7) // 8, d.u8, 0x5A)}, lambda f0, n, p: hip.interleave_bits(il, n, at(x, f0), p("tx"), "bytes", "packed", None))
    assert r is not None and np.array_equal(d.rows(r["tx"], last), ils.pack(want))
    del r, x
    d.free()
    # packed to packed: an item is one output byte of eight transmitted bits
    in_row, out_row = (N + 7) // 8, (n_tx + 7) // 8
    B = 535800
    assert _window(B, out_row) % 256 != 0
    x = _pattern(d, B * in_row, 3, d.u8).reshape(B, in_row)
    last = (0, B - 2, B - 1)
    r = run(hip, d, B, {"tx": (out_row, d.u8, 0x5A)}, lambda f0, n, p: hip.interleave_bits(il, n, at(x, f0), p("tx"), "packed", "packed", None))
    cwb = np.unpackbits(d.rows(x, last), axis=1, bitorder="little")[:, :N]
    assert r is not None and np.array_equal(d.rows(r["tx"], last), ils.pack(ils.interleave(cwb, pos)))
    del r, x
    il.close()
    d.free()


def test_second_pass_extract_messages_bytes(hip):
    d = Dev()
    c = load("jpl.1024.4.5")
    B = 262145
    _window(B, c.k)
    code = c.hip_code(hip)
    sim = hip.Sim(code, c.k, c.n_tx, G_qc=_qc_words(hip, "jpl.1024.4.5"), max_batch=B)
    assert sim.encoder == "qc"
    bits = _pattern(d, B * c.N, 4, d.u8).reshape(B, c.N)
    r = run(hip, d, B, {"m": (c.k, d.u8, 9)}, lambda f0, n, p: sim.extract_messages(n, at(bits, f0), p("m"), "bytes", None))
    last = (0, B - 2, B - 1)
    assert r is not None and np.array_equal(d.rows(r["m"], last), d.rows(bits, last)[:, :c.k] & 1)
    del r, bits
    sim.close(); code.close()
    d.free()


# ---- 4. the sample and gain stores
PAD, MARK = 256, 0xA5


def _offset_buffer(d, nbytes, off):
    """(the tensor that owns the memory, a pointer off bytes past a 256-byte boundary with nbytes to write, marked bytes around it)"""
    t = d.torch.full((PAD + off + nbytes + PAD,), MARK, dtype=d.u8, device=d.dev)
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + PAD + off


def _written(d, t, nbytes, off):
    d.sync()
    a = t.cpu().numpy()
    assert (a[:PAD + off] == MARK).all() and (a[PAD + off + nbytes:] == MARK).all(), "written outside the buffer"
    return a[PAD + off:PAD + off + nbytes].tobytes()


@pytest.mark.parametrize("kind,b", [("table", None), ("product", 1)], ids=["16qam", "product-1"])
def test_sample_and_gain_stores_at_every_alignment(hip, kind, b):
    B = 5
    d = Dev()
    o = Obj(hip, kind, b)
    mod = o.mod
    parities = set()
    for n_tx in (184, 186):
        src = _source203(hip, B, n_tx=n_tx)
        sim, N = src.sim, src.N
        ns = mod.symbols(n_tx)
        parities.add(ns % 2)
        il = hip.Interleaver(_source_table(src, o.m), N)
        fad = hip.Fading(3, 0.0)
        sb, gb = B * ns * 8, B * ns * 4
        first, db = 2 ** 32 - 2, 6.0

        def samples(call, off):
            t, p = _offset_buffer(d, sb, off)
            d.sync()
            call(p)
            return _written(d, t, sb, off)

        for what, call in (("transmit", lambda p: sim.transmit(mod, SEED, first, B, db, p, None, "bytes", None, None)),
                           ("transmit_il", lambda p: sim.transmit_il(mod, il, SEED, first, B, db, p, None, "bytes", None, None))):
            a, c = samples(call, 0), samples(call, 8)
            assert a == c, (what, n_tx, "samples 8 bytes past a 16-byte boundary")
        got = {}
        for so in (0, 8):
            for go in (0, 4):
                ts, p_s = _offset_buffer(d, sb, so)
                tg, p_g = _offset_buffer(d, gb, go)
                d.sync()
                sim.transmit_il_fading(mod, il, fad, SEED, first, B, db, p_s, p_g, None, "bytes", None, None)
                got[(so, go)] = (_written(d, ts, sb, so), _written(d, tg, gb, go))
        ref = got[(0, 0)]
        assert all(v == ref for v in got.values()), ("transmit_il_fading", n_tx, [k for k, v in got.items() if v != ref])
        assert samples(lambda p: sim.transmit_il_fading(mod, il, fad, SEED, first, B, db, p, None, None, "bytes", None, None), 8) == ref[0], "d_gain NULL"
        a32 = np.frombuffer(ref[1], np.float32)
        assert np.isfinite(a32).all() and (a32 >= 2.0 ** -20).all() and len(np.unique(a32)) > B
        llrs = []
        for go in (0, 4):
            tg, p_g = _offset_buffer(d, gb, go)
            llr = d.full(B, N, 777.0, d.f32)
            d.sync()
            sim.generate_mod_il_fading(mod, il, fad, SEED, first, B, db, llr.data_ptr(), "f32", 0.0, p_g, None, "bytes", None, None)
            assert _written(d, tg, gb, go) == ref[1], ("generate_mod_il_fading", n_tx, go, "gains")
            l = llr.cpu().numpy()
            assert (l[B] == 777.0).all()
            llrs.append(l[:B].tobytes())
        assert llrs[0] == llrs[1]
        il.close()
        src.close()
    assert parities == {0, 1}, "n_sym even (the vector stores, where the pointer allows them) and odd (never)"
    mod.close()
