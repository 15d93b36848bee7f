"""GPU: ldpc_decode_batch_dev_soft on all eighteen soft instances of the on-chip layered min-sum kernel for any H (csrc/layered_csr.hip
layered_csr_soft_kernel<8|20|32, cell> and <..., Ruled<cell>>) against tests/soft_output_spec.py, bit for bit: np.array_equal everywhere, no
tolerance -- both kinds, the three output formats, max_iters 0, 1 and 25, the 16-byte path and (d_soft offset by one element; "w20", whose N
is odd) the element path, a guard band around d_soft.  bits, sweeps and flags are the plain call's on the same context, which is run before
and after and still reports the plain instance.  Frames that are not finite beside finite ones (f32 cells), more frames than workgroups,
the refusals of the other kernel families and the LDPC_EINVAL cases."""
import numpy as np
import pytest

from tests import layered_shapes as S
from tests import soft_output_cases as K
from tests import soft_output_spec as spec
from tests.helpers import load

pytestmark = pytest.mark.gpu

ENV = "LDPC_LAYERED_CSR_THREADS"
NP_OF = {"f32": np.float32, "f16": np.float16, "i8": np.int8}
CTYPE = {"f16": "_Float16", "f32": "float", "i8": "signed char"}
FILL = 0x5A


def _names(name, cell, ruled):
    """-> the plain instance's name, the soft instance's"""
    t = CTYPE[cell]
    if ruled:
        arg = f"<{S.DCLASS[name]}, ldpc::Ruled<{t}>>"
    else:
        arg = f"<{S.DCLASS[name]}>" if cell == "f16" else f"<{S.DCLASS[name]}, {t}>"
    return "ldpc::layered_csr_kernel" + arg, "ldpc::layered_csr_soft_kernel" + arg


def _decoder(hip, name, cell, rule, F):
    g = S.case(name)
    kw = {} if rule == K.PLAIN else dict(cn_scale=rule[0], cn_offset=rule[1])
    path = "fused" if cell == "f32" and rule == K.PLAIN else "auto"
    dec = hip.Decoder(g.code(hip, g.layer_ptr), "min", cell, F, schedule="layered", path=path, **kw)
    assert dec.path == "fused"
    return dec


class Dev:
    """the device buffers of one decoder's calls, through torch"""

    def __init__(self, dec, llr):
        import torch
        self.torch, self.dec, self.dev = torch, dec, torch.device("cuda", 0)
        self.F, self.N = llr.shape
        self.llr = torch.from_numpy(np.array(llr)).to(self.dev)
        self.llr_fmt = {np.dtype(np.float32): "f32", np.dtype(np.float16): "f16", np.dtype(np.int8): "i8"}[llr.dtype]
        self.bits = torch.zeros((self.F, self.N), dtype=torch.uint8, device=self.dev)
        self.iters = torch.zeros(self.F, dtype=torch.int32, device=self.dev)
        self.conv = torch.zeros(self.F, dtype=torch.uint8, device=self.dev)

    def _clear(self):
        self.bits.fill_(7); self.iters.fill_(-7); self.conv.fill_(7)
        self.torch.cuda.synchronize()

    def _results(self):
        self.dec.synchronize()
        return self.bits.cpu().numpy(), self.iters.cpu().numpy(), self.conv.cpu().numpy().astype(bool)

    def plain(self, max_iters):
        self._clear()
        self.dec.decode_batch_dev(self.llr.data_ptr(), self.bits.data_ptr(), self.F, max_iters, self.iters.data_ptr(), self.conv.data_ptr(),
                                  llr_f16=self.llr_fmt == "f16", llr_i8=self.llr_fmt == "i8")
        return self._results()

    def soft(self, max_iters, kind, fmt, soft_qscale=0.0, offset=0):
        """-> bits, sweeps, flags, soft [F, N]; offset: elements d_soft starts after a 256-byte boundary.  The elements before and after
        the F N written ones must keep their fill"""
        es = np.dtype(NP_OF[fmt]).itemsize
        raw = self.torch.full(((self.F * self.N + 2 + offset) * es,), FILL, dtype=self.torch.uint8, device=self.dev)
        self._clear()
        self.dec.decode_batch_dev_soft(self.llr.data_ptr(), self.bits.data_ptr(), raw.data_ptr() + offset * es, self.F, max_iters, kind, fmt, soft_qscale,
                                       self.iters.data_ptr(), self.conv.data_ptr(), None, self.llr_fmt)
        b, i, c = self._results()
        host = raw.cpu().numpy()
        a, z = offset * es, (offset + self.F * self.N) * es
        assert (host[:a] == FILL).all() and (host[z:] == FILL).all(), "the guard band around d_soft was written"
        return b, i, c, host[a:z].view(NP_OF[fmt]).reshape(self.F, self.N)


def _bits_of(a):
    return np.ascontiguousarray(a).view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _check(got, ref, kind, fmt, cell, what, soft_qscale=0.0):
    bits, sweeps, conv, P, C = ref
    assert np.array_equal(got[1], sweeps), (what, "sweeps", got[1], sweeps)
    assert np.array_equal(got[2], conv), (what, "flags")
    assert np.array_equal(got[0], bits), (what, "bits")
    want = spec.soft(cell, P, C, kind, fmt, soft_qscale, K.QSCALE)
    assert got[3].dtype == want.dtype and np.array_equal(_bits_of(got[3]), _bits_of(want)), (what, "soft", np.flatnonzero((_bits_of(got[3]) != _bits_of(want)).any(axis=1)))


@pytest.mark.parametrize("ruled", [False, True], ids=["plain", "ruled"])
@pytest.mark.parametrize("cell", K.CELLS)
@pytest.mark.parametrize("name", K.NAMES)
def test_every_soft_instance_bit_exact(hip, monkeypatch, name, cell, ruled):
    monkeypatch.delenv(ENV, raising=False)
    rule = K.rule_of(name, cell, ruled)
    llr = K.frames(name)
    ref25 = K.ref(name, cell, rule, K.SWEEPS)
    assert K.exercised(ref25[1], ref25[2]), (name, cell, rule)
    dec = _decoder(hip, name, cell, rule, len(llr))
    plain_name, soft_name = _names(name, cell, ruled)
    d = Dev(dec, llr)
    before = {mi: d.plain(mi) for mi in (0, 1, K.SWEEPS)}
    assert dec.kernel_name == plain_name, dec.kernel_name
    for mi in (0, 1, K.SWEEPS):
        ref = K.ref(name, cell, rule, mi)
        for kind in spec.KINDS:
            for fmt in spec.FORMATS:
                # the 16-byte path where N % 8 == 0, and the element path: N odd ("w20"), or d_soft aligned to its element only
                for off in (0, 1) if mi == K.SWEEPS else (0,):
                    what = (name, cell, rule, mi, kind, fmt, off)
                    got = d.soft(mi, kind, fmt, offset=off)
                    assert dec.kernel_name == soft_name, dec.kernel_name
                    _check(got, ref, kind, fmt, cell, what)
                    assert all(np.array_equal(x, y) for x, y in zip(got[:3], before[mi])), (what, "the plain call's results")
    for mi in (0, 1, K.SWEEPS):
        after = d.plain(mi)
        assert dec.kernel_name == plain_name, dec.kernel_name
        assert all(np.array_equal(x, y) for x, y in zip(after, before[mi])), (name, cell, rule, mi, "plain after soft")
    dec.close()


@pytest.mark.parametrize("cell", K.CELLS)
def test_llr_formats_and_the_output_scale(hip, monkeypatch, cell):
    """fp16 LLRs (every cell), int8 LLRs (int8 cells), an int8 output scale of its own (float cells), the context's (int8 cells); "w8": the
    16-byte loads of every format"""
    monkeypatch.delenv(ENV, raising=False)
    name, g = "w8", S.case("w8")
    l16 = K.frames(name).astype(np.float16)
    ref = spec.decode(cell, g, l16.astype(np.float32), K.SWEEPS, K.PLAIN[0], K.PLAIN[1], K.QSCALE)
    assert ref[2][:8].any() and (ref[1][:8] > 1).any()
    dec = _decoder(hip, name, cell, K.PLAIN, len(l16))
    d = Dev(dec, l16)
    for kind in spec.KINDS:
        for fmt, qs in (("f32", 0.0), ("i8", K.QSCALE if cell == "i8" else 2.5)):
            _check(d.soft(K.SWEEPS, kind, fmt, qs), ref, kind, fmt, cell, (cell, "f16 LLRs", kind, fmt), qs)
    if cell == "i8":
        q = spec.quantize(K.frames(name), K.QSCALE).astype(np.int8)
        d8, r8 = Dev(dec, q), K.ref(name, cell, K.PLAIN, K.SWEEPS)
        for kind in spec.KINDS:
            for fmt in spec.FORMATS:
                _check(d8.soft(K.SWEEPS, kind, fmt), r8, kind, fmt, cell, (cell, "i8 LLRs", kind, fmt))
    # the host route through torch tensors
    b, i, c, s = dec.decode_batch_soft(l16, K.SWEEPS, kind="extrinsic", soft_fmt="f16")
    _check((b, i, c.astype(bool), s), ref, "extrinsic", "f16", cell, (cell, "decode_batch_soft"))
    dec.close()


def test_frames_that_are_not_finite(hip, monkeypatch):
    """f32 cells: -inf in a frame that then converges and is failed by the veto, a NaN in the noiseless codeword, beside eight finite frames.
    The posterior is the specification's by bit pattern on every frame; the finite frames are what they are without the two (isolation);
    an extrinsic row of a frame that is not finite is compared with NaN == NaN (inf - inf: the NaN's sign is the machine's)"""
    monkeypatch.delenv(ENV, raising=False)
    name = "w20"
    llr, f, col, ref = K.nonfinite(name)
    clean = K.ref(name, "f32", K.PLAIN, K.SWEEPS)
    assert not ref[2][f] and not ref[2][9] and np.isneginf(ref[3][f, col]) and np.isnan(ref[3][9, 5])
    dec = _decoder(hip, name, "f32", K.PLAIN, len(llr))
    d = Dev(dec, llr)
    plain = d.plain(K.SWEEPS)
    others = [i for i in range(10) if i not in (f, 9)]
    for fmt in spec.FORMATS:
        got = d.soft(K.SWEEPS, "posterior", fmt)
        _check(got, ref, "posterior", fmt, "f32", (name, "not finite", fmt))
        assert all(np.array_equal(x, y) for x, y in zip(got[:3], plain))
        assert np.array_equal(got[3][others], spec.soft("f32", clean[3], clean[4], "posterior", fmt)[others]), fmt
    got = d.soft(K.SWEEPS, "extrinsic", "f32")
    want = spec.soft("f32", ref[3], ref[4], "extrinsic", "f32")
    assert np.array_equal(_bits_of(got[3][others]), _bits_of(want[others]))
    assert np.array_equal(got[3][[f, 9]], want[[f, 9]], equal_nan=True) and np.isnan(want[f, col]) and np.isnan(want[9, 5])
    dec.close()


def test_more_frames_than_workgroups(hip, monkeypatch):
    """the ten frames tiled to 600 on one fp16 context, "w20": more frames than the launch has workgroups, the rest taken from the counter"""
    monkeypatch.delenv(ENV, raising=False)
    name, F = "w20", 600
    ten, ref = K.frames(name), K.ref(name, "f16", K.PLAIN, K.SWEEPS)
    idx = np.random.default_rng(600).permutation(np.tile(np.arange(len(ten)), F // len(ten)))
    dec = _decoder(hip, name, "f16", K.PLAIN, F)
    d = Dev(dec, np.ascontiguousarray(ten[idx]))
    want = tuple(r[idx] for r in ref)
    _check(d.soft(K.SWEEPS, "extrinsic", "f32"), want, "extrinsic", "f32", "f16", (name, F))
    _check(d.soft(K.SWEEPS, "posterior", "f16", offset=1), want, "posterior", "f16", "f16", (name, F, "offset"))
    dec.close()


def test_other_kernel_families_refuse(hip):
    g = S.case("w8")
    llr = K.frames("w8")
    flooding = hip.Decoder(g.code(hip), "min", "f32", len(llr))
    pk = hip.Decoder(load("jpl.1024.4.5").hip_code(hip), "min", "f16pk", 4)
    assert "layered_csr" not in flooding.kernel_name and "fused_pk16_kernel" in pk.kernel_name
    for dec, n in ((flooding, g.N), (pk, 1024)):
        import torch
        dev = torch.device("cuda", 0)
        l, b, s = torch.zeros((4, n), device=dev), torch.zeros((4, n), dtype=torch.uint8, device=dev), torch.zeros((4, n), device=dev)
        family = dec.kernel_name
        with pytest.raises(hip.LdpcError) as e:
            dec.decode_batch_dev_soft(l.data_ptr(), b.data_ptr(), s.data_ptr(), 4, 5)
        assert e.value.code == hip._lib.EUNSUPPORTED and family in str(e.value) and "layered_csr_kernel" in str(e.value) and "LDPC_SCHED_LAYERED" in str(e.value), str(e.value)
        dec.close()


def test_invalid_arguments(hip, monkeypatch):
    import torch
    monkeypatch.delenv(ENV, raising=False)
    llr = K.frames("w8")
    F, N = llr.shape
    dev = torch.device("cuda", 0)
    l, b, s = torch.from_numpy(np.array(llr)).to(dev), torch.zeros((F, N), dtype=torch.uint8, device=dev), torch.zeros((F, N + 1), device=dev)
    for cell in ("f32", "i8"):
        dec = _decoder(hip, "w8", cell, K.PLAIN, F)

        def bad(what, soft=s.data_ptr(), kind="posterior", fmt="f32", qs=0.0, llr_fmt="f32", code=hip._lib.EINVAL):
            with pytest.raises(hip.LdpcError) as e:
                dec.decode_batch_dev_soft(l.data_ptr(), b.data_ptr(), soft, F, 5, kind, fmt, qs, None, None, None, llr_fmt)
            assert e.value.code == code, (cell, what, str(e.value))

        bad("null d_soft", soft=None)
        bad("unknown kind", kind=2)
        bad("unknown format", fmt=3)
        bad("unknown LLR format", llr_fmt=3)
        bad("negative scale", fmt="i8", qs=-1.0)
        bad("NaN scale", fmt="i8", qs=float("nan"))
        bad("infinite scale", fmt="i8", qs=float("inf"))
        bad("f32 output at an odd byte", soft=s.data_ptr() + 2)
        bad("f16 output at an odd byte", soft=s.data_ptr() + 1, fmt="f16")
        if cell == "i8":
            bad("a scale that is not the context's", fmt="i8", qs=2.0)
            dec.decode_batch_dev_soft(l.data_ptr(), b.data_ptr(), s.data_ptr(), F, 5, "posterior", "i8", dec.qscale)
        else:
            bad("int8 LLRs on a float context", llr_fmt="i8", code=hip._lib.EUNSUPPORTED)
            dec.decode_batch_dev_soft(l.data_ptr(), b.data_ptr(), s.data_ptr() + 1, F, 5, "posterior", "i8", 2.0)      # int8 output: any byte
        dec.decode_batch_dev_soft(l.data_ptr(), b.data_ptr(), s.data_ptr(), 0, 5)                                        # no frames: nothing to do
        dec.synchronize()
        dec.close()
