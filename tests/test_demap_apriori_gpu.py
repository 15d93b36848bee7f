"""GPU: ldpc_demap_dev_il_apriori (csrc/demap_apriori.hip) against tests/demap_apriori_spec.py on the inputs of tests/demap_apriori_cases.py:
the seven table objects m = 1..6, three noise levels, the ragged shape through an interleaver with gains (a 0 and a NaN) and the aligned one
with a NULL d_gain, the three a-priori sets (the "normal" one holds a NaN at every punctured position: it is never read).
  max-log   bit for bit in the three output formats (a NaN is a NaN, whatever its payload);
  log-MAP   within the bar the specification derives, of its float64 brute force;
  0 at the punctured positions, a guard row before and after d_llr untouched, isolation from a frame whose a-priori values are NaN,
  the refusal for a product object, the LDPC_EINVAL cases."""
import numpy as np
import pytest

from tests import demap_apriori_cases as K
from tests import demap_apriori_spec as spec
from tests import demap_logmap_cases as cl
from tests import interleaver_spec as ils
from tests import modulation_spec as ms

pytestmark = pytest.mark.gpu

FMTS = (("f32", ms.LLR_F32, 0.0), ("f16", ms.LLR_F16, 0.0), ("i8", ms.LLR_I8, 2.5))
NP_OF = {"f32": np.float32, "f16": np.float16, "i8": np.int8}
FILL = 0x5A
B = K.B


class Dev:
    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)

    def put(self, a):
        return self.torch.from_numpy(np.array(a)).to(self.dev)

    def run(self, hip, mod, il, sym, gain, nv, la, N, fmt="f32", qs=0.0):
        """-> rows [B][N]; the guard rows before and after must keep their fill"""
        es = np.dtype(NP_OF[fmt]).itemsize
        raw = self.torch.full(((B + 2) * N * es,), FILL, dtype=self.torch.uint8, device=self.dev)
        self.torch.cuda.synchronize()
        hip.demap_il_apriori(mod, il, B, sym.data_ptr(), None if gain is None else gain.data_ptr(), nv, la.data_ptr(), raw.data_ptr() + N * es, fmt, qs, None)
        self.torch.cuda.synchronize()
        host = raw.cpu().numpy()
        assert (host[:N * es] == FILL).all() and (host[(B + 1) * N * es:] == FILL).all(), "a guard row around d_llr was written"
        return host[N * es:(B + 1) * N * es].view(NP_OF[fmt]).reshape(B, N)


def _same(got, want):
    """bit for bit, a NaN equal to any NaN"""
    assert got.dtype == want.dtype and got.shape == want.shape
    if got.dtype == np.int8:
        return np.array_equal(got, want)
    gn, wn = np.isnan(got), np.isnan(want)
    view = np.uint32 if got.dtype == np.float32 else np.uint16
    return np.array_equal(gn, wn) and np.array_equal(got.view(view)[~gn], want.view(view)[~wn])


@pytest.mark.parametrize("name", K.IDS)
def test_against_the_spec(hip, name):
    c = cl.case("table", name)
    d = Dev()
    mod = c.make(hip)
    logmap = mod.with_rule("logmap")
    for shape in K.SHAPES:
        pos, N = K.positions(shape), K.n_codeword(shape)
        il = hip.Interleaver(np.array(pos), N)
        holes = ils.holes(pos, N)
        for level in K.LEVELS:
            sym, a, _, _, nv = K.inputs(name, level, shape)
            dsym, dgain = d.put(sym), None if a is None else d.put(a)
            for which in K.SETS:
                what = (name, shape, level, which)
                la_cw = K.apriori(name, level, shape, which)
                dla = d.put(la_cw)
                per = K.reference(name, level, shape, which, spec.MAXLOG)[0]
                for fmt, code, qs in FMTS:
                    got = d.run(hip, mod, il, dsym, dgain, nv, dla, N, fmt, qs)
                    assert _same(got, spec.place(per, pos, N, code, qs if qs else 4.0)), what + (fmt,)
                    assert not got[:, holes].any(), what + (fmt, "punctured positions")
                # log-MAP
                want, T, A, _ = K.brute(name, level, shape, which, spec.LOGMAP)
                bar = spec.logmap_bar(want, c.m, T, A)
                got = d.run(hip, logmap, il, dsym, dgain, nv, dla, N)
                tx = got[:, pos]
                w, b = want.reshape(B, -1)[:, :len(pos)], bar.reshape(B, -1)[:, :len(pos)]
                fin = np.isfinite(w)
                assert np.array_equal(np.isfinite(tx), fin) and not got[:, holes].any(), what + ("log-MAP",)
                err = np.abs(tx.astype(np.float64) - w)
                assert (err[fin] <= b[fin]).all(), what + ("log-MAP", float((err[fin] / b[fin]).max()))
        il.close()


def test_a_nan_apriori_frame_stays_alone(hip):
    name, level, shape = "16qam", "mid", "ragged"
    c = cl.case("table", name)
    d = Dev()
    pos, N = K.positions(shape), K.n_codeword(shape)
    mod, il = c.make(hip), hip.Interleaver(np.array(pos), N)
    sym, a, _, _, nv = K.inputs(name, level, shape)
    la = np.array(K.apriori(name, level, shape, "normal"))
    clean = d.run(hip, mod, il, d.put(sym), d.put(a), nv, d.put(la), N)
    la[1] = np.nan
    got = d.run(hip, mod, il, d.put(sym), d.put(a), nv, d.put(la), N)
    assert _same(got[[0, 2]], clean[[0, 2]]) and np.isnan(got[1][pos]).all() and not got[1][ils.holes(pos, N)].any()


def test_refusals(hip):
    import torch
    dev = torch.device("cuda", 0)
    N = 64
    il = hip.Interleaver(np.arange(N, dtype=np.int32), N)
    mod = hip.Modulation("16qam")
    sym, gain = torch.zeros((B, N // 4, 2), device=dev), torch.ones((B, N // 4), device=dev)
    la, out = torch.zeros((B, N), device=dev), torch.zeros((B, N + 1), device=dev)

    def call(m=mod, s=sym.data_ptr(), g=gain.data_ptr(), nv=0.5, l=la.data_ptr(), o=out.data_ptr(), fmt="f32", qs=0.0, batch=B):
        hip.demap_il_apriori(m, il, batch, s, g, nv, l, o, fmt, qs, None)

    def bad(code, **kw):
        with pytest.raises(hip.LdpcError) as e:
            call(**kw)
        assert e.value.code == code, (kw, str(e.value))
        return str(e.value)

    call()
    call(g=None)                                            # a NULL d_gain: gains of 1
    product = hip.Modulation.product(np.array([-1.0, 1.0], np.float32), np.array([-1.0, 1.0], np.float32))
    msg = bad(hip._lib.EUNSUPPORTED, m=product)
    assert "product" in msg and "iterat" in msg, msg
    E = hip._lib.EINVAL
    bad(E, l=None)
    bad(E, l=la.data_ptr() + 2)
    bad(E, s=None)
    bad(E, o=None)
    bad(E, s=sym.data_ptr() + 4)
    bad(E, g=gain.data_ptr() + 2)
    bad(E, o=out.data_ptr() + 2)
    bad(E, fmt="f16", o=out.data_ptr() + 1)
    bad(E, nv=0.0)
    bad(E, nv=float("nan"))
    bad(E, batch=0)
    bad(E, fmt=3)
    bad(E, fmt="i8", qs=-1.0)
    # overlap: in place, the last element of d_apriori on the first of d_llr, the first of d_apriori inside d_llr
    bad(E, l=out.data_ptr())
    both = torch.zeros((2 * B * N,), device=dev)
    bad(E, l=both.data_ptr(), o=both.data_ptr() + 4 * (B * N - 1))
    bad(E, l=both.data_ptr() + 4 * (B * N - 1), o=both.data_ptr())
    call(l=both.data_ptr(), o=both.data_ptr() + 4 * B * N)  # back to back: no shared byte
    torch.cuda.synchronize()
    il.close()
