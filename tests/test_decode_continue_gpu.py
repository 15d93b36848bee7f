"""GPU: ldpc_decode_state_* and ldpc_decode_batch_dev_continue on all eighteen continuing instances of the on-chip layered min-sum kernel for
any H (csrc/layered_csr.hip layered_csr_cont_kernel<8|20|32, cell> and <..., Ruled<cell>>) against tests/decode_continue_spec.py, bit for bit:
np.array_equal everywhere, no tolerance.  The chain of three calls of tests/decode_continue_cases.py with both kinds, the three output formats,
d_soft offset by one element, a guard band around d_soft, and without a soft output; a reset state against decode_batch_dev_soft on the same
context; fp16 and int8 LLRs; slots of a larger state; more frames than workgroups; frames that are not finite (f32 cells); the refusals."""
import numpy as np
import pytest

from tests import decode_continue_cases as D
from tests import decode_continue_spec as cspec
from tests import layered_shapes as S
from tests import soft_output_cases as K
from tests import soft_output_spec as spec
from tests.helpers import load
from tests.test_soft_output_gpu import ENV, FILL, NP_OF, Dev, _decoder, _names

pytestmark = pytest.mark.gpu

LLR_FMT = {np.dtype(np.float32): "f32", np.dtype(np.float16): "f16", np.dtype(np.int8): "i8"}


def _cont_name(name, cell, ruled):
    return _names(name, cell, ruled)[1].replace("layered_csr_soft_kernel", "layered_csr_cont_kernel")


class Cont:
    """the device buffers of one decoder's continuing calls, through torch"""

    def __init__(self, dec, F, N):
        import torch
        self.torch, self.dec, self.dev, self.F, self.N = torch, dec, torch.device("cuda", 0), F, N
        self.bits = torch.zeros((F, N), dtype=torch.uint8, device=self.dev)
        self.iters = torch.zeros(F, dtype=torch.int32, device=self.dev)
        self.conv = torch.zeros(F, dtype=torch.uint8, device=self.dev)

    def call(self, state, llr, max_iters, kind="posterior", fmt="f32", soft_qscale=0.0, offset=0, first=0, want_soft=True):
        """-> bits, sweeps, flags, soft [F, N] (None without a soft output); offset: elements d_soft starts after a 256-byte boundary.  The
        elements before and after the F N written ones must keep their fill"""
        torch = self.torch
        assert llr.shape == (self.F, self.N)
        d_llr = torch.from_numpy(np.array(llr)).to(self.dev)
        es = np.dtype(NP_OF[fmt]).itemsize
        raw = torch.full(((self.F * self.N + 2 + offset) * es,), FILL, dtype=torch.uint8, device=self.dev)
        self.bits.fill_(7); self.iters.fill_(-7); self.conv.fill_(7)
        torch.cuda.synchronize()
        self.dec.decode_batch_dev_continue(state, d_llr.data_ptr(), self.bits.data_ptr(), self.F, max_iters, raw.data_ptr() + offset * es if want_soft else None,
                                           kind, fmt, soft_qscale, self.iters.data_ptr(), self.conv.data_ptr(), None, LLR_FMT[llr.dtype], first)
        self.dec.synchronize()
        b, i, c = self.bits.cpu().numpy(), self.iters.cpu().numpy(), self.conv.cpu().numpy().astype(bool)
        host = raw.cpu().numpy()
        if not want_soft:
            assert (host == FILL).all()
            return b, i, c, None
        a, z = offset * es, (offset + self.F * self.N) * es
        assert (host[:a] == FILL).all() and (host[z:] == FILL).all(), "the guard band around d_soft was written"
        return b, i, c, host[a:z].view(NP_OF[fmt]).reshape(self.F, self.N)


def _check(got, ref, kind, fmt, cell, what, soft_qscale=0.0, rows=None):
    bits, sweeps, conv, P, C = ref if rows is None else tuple(r[rows] for r in ref)
    got = got if rows is None else tuple(None if g is None else g[rows] for g in got)
    assert np.array_equal(got[1], sweeps), (what, "sweeps", got[1], sweeps)
    assert np.array_equal(got[2], conv), (what, "flags")
    assert np.array_equal(got[0], bits), (what, "bits")
    if got[3] is not None:
        want = spec.soft(cell, P, C, kind, fmt, soft_qscale, K.QSCALE)
        assert got[3].dtype == want.dtype and np.array_equal(D.bits_of(got[3]), D.bits_of(want)), (what, "soft", np.flatnonzero((D.bits_of(got[3]) != D.bits_of(want)).any(axis=1)))


@pytest.mark.parametrize("ruled", [False, True], ids=["plain", "ruled"])
@pytest.mark.parametrize("cell", K.CELLS)
@pytest.mark.parametrize("name", K.NAMES)
def test_every_continuing_instance_bit_exact(hip, monkeypatch, name, cell, ruled):
    """the chain of three calls: after each, bits, sweeps, flags and the soft output are the specification's -- both kinds, on call 2 the three
    formats, the 16-byte path and (d_soft offset by one element; "w20", whose N is odd) the element path.  Without a soft output on calls 1
    and 2 the third call gives what it gave: the state's sums are written without one"""
    monkeypatch.delenv(ENV, raising=False)
    rule = K.rule_of(name, cell, ruled)
    calls = D.chain_llrs(name)
    refs, _ = D.chain(name, cell, rule)
    F, N = calls[0][0].shape
    dec = _decoder(hip, name, cell, rule, F)
    plain_name, soft_name = _names(name, cell, ruled)
    cont_name = _cont_name(name, cell, ruled)
    d = Dev(dec, calls[0][0])
    before = d.plain(K.SWEEPS)
    assert dec.kernel_name == plain_name, dec.kernel_name
    before = before, d.soft(K.SWEEPS, "extrinsic", "f32")
    assert dec.kernel_name == soft_name, dec.kernel_name
    state = hip.DecodeState(dec, F)
    assert state.frames == F and state.nbytes > 0
    c = Cont(dec, F, N)
    for kind in spec.KINDS:
        for fmt in spec.FORMATS:
            for off in (0, 1):
                state.reset()
                for i, ((llr, mi), ref) in enumerate(zip(calls, refs)):
                    f, o = (fmt, off) if i == 1 else ("f32", 0)
                    got = c.call(state, llr, mi, kind, f, offset=o)
                    assert dec.kernel_name == cont_name, dec.kernel_name
                    _check(got, ref, kind, f, cell, (name, cell, rule, "call", i + 1, kind, f, o))
    state.reset()
    for i, ((llr, mi), ref) in enumerate(zip(calls, refs)):
        got = c.call(state, llr, mi, "extrinsic", "f32", want_soft=i == 2)
        _check(got, ref, "extrinsic", "f32", cell, (name, cell, rule, "call", i + 1, "no soft output before the third"))
    after = d.plain(K.SWEEPS)
    assert dec.kernel_name == plain_name, dec.kernel_name
    after = after, d.soft(K.SWEEPS, "extrinsic", "f32")
    assert dec.kernel_name == soft_name, dec.kernel_name
    for x, y in zip(before, after):
        assert all(np.array_equal(D.bits_of(a), D.bits_of(b)) for a, b in zip(x, y)), (name, cell, rule, "plain and soft calls around the chain")
    state.close()
    dec.close()


@pytest.mark.parametrize("cell", K.CELLS)
@pytest.mark.parametrize("name", K.NAMES)
def test_from_a_reset_state_it_is_the_soft_call(hip, monkeypatch, name, cell):
    """against decode_batch_dev_soft on the same context and frames, fresh and again after reset() of a used state"""
    monkeypatch.delenv(ENV, raising=False)
    llr = K.frames(name)
    F, N = llr.shape
    dec = _decoder(hip, name, cell, K.PLAIN, F)
    d, c = Dev(dec, llr), Cont(dec, F, N)
    state = hip.DecodeState(dec, F)
    for used in (False, True):
        for kind in spec.KINDS:
            want = d.soft(K.SWEEPS, kind, "f32")
            got = c.call(state, llr, K.SWEEPS, kind, "f32")
            assert all(np.array_equal(D.bits_of(a), D.bits_of(b)) for a, b in zip(got, want)), (name, cell, kind, used)
            if used or kind == spec.KINDS[0]:
                c.call(state, D.chain_llrs(name)[1][0], 3)          # use it
            state.reset()
    state.close()
    dec.close()


@pytest.mark.parametrize("cell", K.CELLS)
def test_llr_formats(hip, monkeypatch, cell):
    """call 2 of the chain with fp16 LLRs (every cell) and with int8 LLRs (int8 cells); "w8": the 16-byte loads of every format"""
    monkeypatch.delenv(ENV, raising=False)
    name, g = "w8", S.case("w8")
    (llr, mi1), (scaled, mi2), _ = D.chain_llrs(name)
    F, N = llr.shape
    refs, states = D.chain(name, cell, K.PLAIN)
    dec = _decoder(hip, name, cell, K.PLAIN, F)
    c = Cont(dec, F, N)
    state = hip.DecodeState(dec, F)
    seconds = [scaled.astype(np.float16)] + ([spec.quantize(scaled, K.QSCALE).astype(np.int8)] if cell == "i8" else [])
    for l2 in seconds:
        as_given = l2 if l2.dtype == np.int8 else l2.astype(np.float32)
        ref2, _ = cspec.call(cell, g, states[0], as_given, mi2, K.PLAIN[0], K.PLAIN[1], K.QSCALE)
        assert (ref2[1][:8] >= 1).any()
        for kind in spec.KINDS:
            state.reset()
            _check(c.call(state, llr, mi1, kind, "f32"), refs[0], kind, "f32", cell, (cell, "call 1"))
            _check(c.call(state, l2, mi2, kind, "f32"), ref2, kind, "f32", cell, (cell, str(l2.dtype), "call 2", kind))
    # the host route through torch tensors
    state.reset()
    dec.decode_batch_continue(state, np.array(llr), mi1)
    b, i, cv, s = dec.decode_batch_continue(state, np.array(scaled), mi2, kind="extrinsic", soft_fmt="f16")
    _check((b, i, cv.astype(bool), s), refs[1], "extrinsic", "f16", cell, (cell, "decode_batch_continue"))
    state.close()
    dec.close()


def test_slots_of_a_larger_state(hip, monkeypatch):
    """a state of 30 slots, the chain in slots 10 .. 19 only: slots 0 .. 9 and 20 .. 29 then behave as from reset, 10 .. 19 as the chain"""
    monkeypatch.delenv(ENV, raising=False)
    name, cell = "w20", "f16"
    calls = D.chain_llrs(name)
    refs, _ = D.chain(name, cell, K.PLAIN)
    fresh = K.ref(name, cell, K.PLAIN, K.SWEEPS)
    F, N = calls[0][0].shape
    dec = _decoder(hip, name, cell, K.PLAIN, F)
    c = Cont(dec, F, N)
    state = hip.DecodeState(dec, 30)
    assert state.frames == 30
    for (llr, mi), ref in zip(calls[:2], refs[:2]):
        _check(c.call(state, llr, mi, "extrinsic", "f32", first=10), ref, "extrinsic", "f32", cell, (name, "slots 10..19"))
    for first in (0, 20):
        _check(c.call(state, calls[0][0], K.SWEEPS, "extrinsic", "f32", first=first), fresh, "extrinsic", "f32", cell, (name, "as from reset", first))
    _check(c.call(state, calls[2][0], calls[2][1], "extrinsic", "f32", first=10), refs[2], "extrinsic", "f32", cell, (name, "slots 10..19, call 3"))
    state.close()
    dec.close()


def test_more_frames_than_workgroups(hip, monkeypatch):
    """the ten frames tiled to 600 on one fp16 context, "w20": calls 1 and 2 of the chain against the tiled specification"""
    monkeypatch.delenv(ENV, raising=False)
    name, F, cell = "w20", 600, "f16"
    calls = D.chain_llrs(name)
    refs, _ = D.chain(name, cell, K.PLAIN)
    idx = np.random.default_rng(600).permutation(np.tile(np.arange(10), F // 10))
    dec = _decoder(hip, name, cell, K.PLAIN, F)
    c = Cont(dec, F, calls[0][0].shape[1])
    state = hip.DecodeState(dec, F)
    for i, ((llr, mi), ref) in enumerate(zip(calls[:2], refs[:2])):
        want = tuple(r[idx] for r in ref)
        _check(c.call(state, np.ascontiguousarray(llr[idx]), mi, "extrinsic", "f32", offset=i), want, "extrinsic", "f32", cell, (name, F, "call", i + 1))
    state.close()
    dec.close()


def test_frames_that_are_not_finite(hip, monkeypatch):
    """f32 cells, "w20": call 1 with -inf in one noisy frame and a NaN in the noiseless codeword.  The finite frames' call-2 results are those
    of the chain without the two (isolation); both poisoned slots hold a sum that is not finite and come back failed in call 2, whatever they
    are given; after reset of the two slots a call equals a decode from reset.  The values of a slot that holds a NaN are not compared"""
    monkeypatch.delenv(ENV, raising=False)
    name, cell = "w20", "f32"
    bad, f, col, _ = K.nonfinite(name)
    calls = D.chain_llrs(name)
    refs, _ = D.chain(name, cell, K.PLAIN)
    fresh = K.ref(name, cell, K.PLAIN, K.SWEEPS)
    F, N = bad.shape
    others = [i for i in range(F) if i not in (f, 9)]
    dec = _decoder(hip, name, cell, K.PLAIN, F)
    c = Cont(dec, F, N)
    state = hip.DecodeState(dec, F)
    got = c.call(state, bad, calls[0][1], "posterior", "f32")
    _check(got, refs[0], "posterior", "f32", cell, (name, "call 1, the finite frames"), rows=others)
    assert not got[2][f] and not got[2][9]
    got = c.call(state, calls[1][0], calls[1][1], "posterior", "f32")
    _check(got, refs[1], "posterior", "f32", cell, (name, "call 2, the finite frames"), rows=others)
    assert not got[2][f] and got[1][f] == calls[1][1], "the slot of the -inf frame stays failed"
    assert not got[2][9] and got[1][9] == calls[1][1], "the slot of the NaN frame stays failed"
    state.reset(f, 1)
    state.reset(9, 1)
    got = c.call(state, calls[0][0], K.SWEEPS, "posterior", "f32")
    _check(got, fresh, "posterior", "f32", cell, (name, "after reset of the two slots"), rows=[f, 9])
    state.close()
    dec.close()


def test_other_kernel_families_refuse(hip):
    import torch
    g = S.case("w8")
    llr = K.frames("w8")
    flooding = hip.Decoder(g.code(hip), "min", "f32", len(llr))
    pk = hip.Decoder(load("jpl.1024.4.5").hip_code(hip), "min", "f16pk", 4)
    served = _decoder(hip, "w8", "f32", K.PLAIN, 4)
    state = hip.DecodeState(served, 4)
    assert "layered_csr" not in flooding.kernel_name and "fused_pk16_kernel" in pk.kernel_name
    dev = torch.device("cuda", 0)
    for dec, n in ((flooding, g.N), (pk, 1024)):
        l, b = torch.zeros((4, n), device=dev), torch.zeros((4, n), dtype=torch.uint8, device=dev)
        family = dec.kernel_name
        for what in ("create", "continue"):
            with pytest.raises(hip.LdpcError) as e:
                if what == "create":
                    hip.DecodeState(dec, 4)
                else:
                    dec.decode_batch_dev_continue(state, l.data_ptr(), b.data_ptr(), 4, 5)
            assert e.value.code == hip._lib.EUNSUPPORTED and family in str(e.value) and "layered_csr_kernel" in str(e.value) and "LDPC_SCHED_LAYERED" in str(e.value), (what, str(e.value))
        dec.close()
    state.close()
    served.close()


def test_invalid_arguments(hip, monkeypatch):
    import torch
    monkeypatch.delenv(ENV, raising=False)
    llr = K.frames("w8")
    F, N = llr.shape
    dev = torch.device("cuda", 0)
    l, b, s = torch.from_numpy(np.array(llr)).to(dev), torch.zeros((F, N), dtype=torch.uint8, device=dev), torch.zeros((F, N + 1), device=dev)
    for cell in ("f32", "i8"):
        dec = _decoder(hip, "w8", cell, K.PLAIN, F)
        other = _decoder(hip, "w8", cell, K.PLAIN, F)
        state, foreign = hip.DecodeState(dec, F + 2), hip.DecodeState(other, F + 2)
        assert state.nbytes == foreign.nbytes and state.frames == F + 2

        def bad(what, st=state, soft=s.data_ptr(), kind="posterior", fmt="f32", qs=0.0, llr_fmt="f32", code=hip._lib.EINVAL, batch=F, first=0, mi=5,
                llr=l.data_ptr(), bits=b.data_ptr()):
            with pytest.raises(hip.LdpcError) as e:
                dec.decode_batch_dev_continue(st, llr, bits, batch, mi, soft, kind, fmt, qs, None, None, None, llr_fmt, first)
            assert e.value.code == code, (cell, what, str(e.value))

        bad("null state", st=None)
        bad("null d_llr", llr=None)
        bad("null d_bits", bits=None)
        bad("f32 LLRs at an odd byte", llr=l.data_ptr() + 2)
        bad("f16 LLRs at an odd byte", llr=l.data_ptr() + 1, llr_fmt="f16")
        bad("a batch above the context's max_batch (inside the state's frames)", batch=F + 1)
        bad("a state made for another context", st=foreign)
        bad("negative first", first=-1)
        bad("negative batch", batch=-1)
        bad("first + batch above the state's frames", first=3)
        bad("negative sweep limit", mi=-1)
        bad("unknown kind", kind=2)
        bad("unknown format", fmt=3)
        bad("unknown LLR format", llr_fmt=3)
        bad("negative scale", fmt="i8", qs=-1.0)
        bad("NaN scale", fmt="i8", qs=float("nan"))
        bad("infinite scale", fmt="i8", qs=float("inf"))
        bad("f32 output at an odd byte", soft=s.data_ptr() + 2)
        bad("f16 output at an odd byte", soft=s.data_ptr() + 1, fmt="f16")
        for first, count in ((-1, 1), (0, -1), (F, 3)):
            with pytest.raises(hip.LdpcError) as e:
                state.reset(first, count)
            assert e.value.code == hip._lib.EINVAL
        with pytest.raises(hip.LdpcError) as e:
            hip.DecodeState(dec, 0)
        assert e.value.code == hip._lib.EINVAL
        if cell == "i8":
            bad("a scale that is not the context's", fmt="i8", qs=2.0)
            dec.decode_batch_dev_continue(state, l.data_ptr(), b.data_ptr(), F, 5, s.data_ptr(), "posterior", "i8", dec.qscale)
        else:
            bad("int8 LLRs on a float context", llr_fmt="i8", code=hip._lib.EUNSUPPORTED)
            dec.decode_batch_dev_continue(state, l.data_ptr(), b.data_ptr(), F, 5, s.data_ptr() + 1, "posterior", "i8", 2.0)      # int8 output: any byte
        dec.decode_batch_dev_continue(state, l.data_ptr(), b.data_ptr(), F, 5, None, first=2)                                      # no soft output: legal
        dec.decode_batch_dev_continue(state, l.data_ptr(), b.data_ptr(), 0, 5, first=F + 2)                                        # no frames: nothing to do
        state.reset(F + 2, 0)
        dec.synchronize()
        # a state that outlives its context: refused by every context, also by one created afterwards (which may sit at the same address),
        # and by a reset on the context's stream; it can still be destroyed
        other.close()
        later = _decoder(hip, "w8", cell, K.PLAIN, F)
        for d in (dec, later):
            with pytest.raises(hip.LdpcError) as e:
                d.decode_batch_dev_continue(foreign, l.data_ptr(), b.data_ptr(), F, 5)
            assert e.value.code == hip._lib.EINVAL, str(e.value)
        with pytest.raises(hip.LdpcError) as e:
            foreign.reset()
        assert e.value.code == hip._lib.EINVAL, str(e.value)
        state.close(); foreign.close()
        later.close(); dec.close()
