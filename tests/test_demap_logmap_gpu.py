"""GPU: the log-MAP LLR rule of the soft demappers (csrc/demap.h demap_llrs_logmap, csrc/demap_product.h axis_llrs_logmap,
csrc/demap_rm.hip; ldpc_modulation_with_rule) against tests/demap_logmap_spec.py, on the inputs of tests/demap_logmap_cases.py: thirteen
objects (table m = 1..6 and an irregular 8-point table, product b = 1..6), three noise variances each, batch 3.

Per object and noise variance, on ldpc_demap_dev (N = 67, n_tx = 61: element stores, a ragged symbol, a zero tail; N = n_tx = 120: the
vector stores), ldpc_demap_dev_il (6 punctured positions), ldpc_demap_dev_il_csi (gains with a 0 and a NaN) and ldpc_demap_dev_rm
(fan-in 0..3, E = 118 > N, with and without gains, accumulate 0, and a second round accumulated onto the first):
  f32      every element within demap_logmap_spec.bound of the float64 specification: 2^-14 + 2 ulp a term, for ldpc_demap_dev_rm times
           the position's fan-in plus one ulp per addition; NaN exactly where the specification has it; the positions nothing names 0
           (accumulate 1: untouched);
  fp16, i8 bit-equal to the specification's converter applied to the f32 output of the same call on the same buffers (the same device
           function with another store; a value near a rounding boundary may not be compared with the float64 specification);
  fixed    bit for bit the max-log object's output on the same buffers: everything for m = 1 and b = 1; every element the specification
  points   marks as collapsed (at the third variance more than half of them); the symbols of gain 0; the NaN mask;
  copies   a with_rule("maxlog") copy gives its source's bits on every entry point and format.
The worst gap, as a fraction of the bound, is printed per object.  Then the interface: the three fused ldpc_sim_generate_mod* calls
refuse a log-MAP object with LDPC_EUNSUPPORTED and name the rule; ldpc_sim_transmit ignores it; a bad rule value is LDPC_EINVAL.
Every output buffer is pre-filled and carries one guard row past the batch."""
import numpy as np
import pytest

from tests import demap_logmap_cases as lc
from tests import demap_logmap_spec as ls
from tests import modulation_spec as ms
from tests import ratematch_spec as rs
from tests.test_fading_gpu import _source203
from tests.test_modulation_gpu import FILL, NP_OF, Dev, _same

pytestmark = pytest.mark.gpu

FMTS = (("f32", ms.LLR_F32, 0.0), ("f16", ms.LLR_F16, 0.0), ("i8", ms.LLR_I8, 2.5))
B = lc.B


def _convert(f32, code, qs):
    return f32 if code == ms.LLR_F32 else ls.to_f16(f32) if code == ms.LLR_F16 else ls.to_i8(f32, qs)


def _scatter(per, pos, n_pos, fill=0):
    """per [B][n_sym][m] -> [B][n_pos] through an injective table; `fill` at the positions it does not name"""
    out = np.full((per.shape[0], n_pos), fill, per.dtype)
    out[:, pos] = per.reshape(per.shape[0], -1)[:, :len(pos)]
    return out


class Entry:
    """one call shape: run(mod, fmt, qs) -> the rows, and what the specification says about them"""

    def __init__(self, name, run, want, fixed, terms=1, mag=None, written=None):
        self.name, self.run, self.want, self.fixed, self.terms, self.mag, self.written = name, run, want, fixed, terms, mag, written


def _entries(hip, d, c, level, keep):
    """the call shapes of object c at one noise variance; `keep` holds the device objects alive"""
    nv = c.noise_var(level)
    inp = lc.inputs(c, level)
    dev = {k: (d.put(sym), None if a is None else d.put(a)) for k, (sym, a) in inp.items()}
    keep.append(dev)
    out = []

    def fixed_of(sym, a):
        f = c.spec("collapsed", sym, nv, a) | np.isnan(c.spec("maxlog", sym, nv, a))
        return f if a is None else f | np.broadcast_to((a == 0)[..., None], f.shape)

    def plain(key, n_tx, n):
        sym, _ = inp[key]

        def run(mod, fmt, qs):
            o = d.full(B, n, FILL[fmt], fmt)
            d.sync()
            hip.demap(mod, B, n_tx, n, dev[key][0].data_ptr(), nv, o.data_ptr(), fmt, qs, None)
            return d.get(o, B, FILL[fmt])
        return Entry(f"demap {key}", run, ls.place(c.spec("llrs", sym, nv), n_tx, n), ls.place(fixed_of(sym, None), n_tx, n) | (np.arange(n) >= n_tx))

    out += [plain("ragged", lc.N_TX, lc.N), plain("aligned", lc.N_ALIGNED, lc.N_ALIGNED)]
    pos = lc.interleaver()
    il = hip.Interleaver(pos, lc.N)
    keep.append(il)
    for key, a in (("ragged", None), ("csi", inp["csi"][1])):
        sym = inp[key][0]

        def run(mod, fmt, qs, key=key, a=a):
            o = d.full(B, lc.N, FILL[fmt], fmt)
            d.sync()
            if a is None:
                hip.demap_il(mod, il, B, dev[key][0].data_ptr(), nv, o.data_ptr(), fmt, qs, None)
            else:
                hip.demap_il_csi(mod, il, B, dev[key][0].data_ptr(), dev[key][1].data_ptr(), nv, o.data_ptr(), fmt, qs, None)
            return d.get(o, B, FILL[fmt])
        out.append(Entry("demap_il" if a is None else "demap_il_csi", run, _scatter(c.spec("llrs", sym, nv, a), pos, lc.N), _scatter(fixed_of(sym, a), pos, lc.N, True)))
    rpos = lc.rm_table()
    E = len(rpos)
    rm = hip.Ratematch(rpos, lc.N)
    keep.append(rm)
    sent = rs.fanin(rpos, lc.N) > 0

    def sums(key):
        sym, a = inp[key]
        per = c.spec("llrs", sym, nv, a).reshape(B, -1)[:, :E]
        want, fan = lc.per_position(per, rpos, lc.N)
        mag, _ = lc.per_position(np.where(np.isfinite(per), np.abs(per), 0.0), rpos, lc.N)
        notfixed, _ = lc.per_position((~fixed_of(sym, a)).reshape(B, -1)[:, :E].astype(np.int64), rpos, lc.N)
        return want, fan, mag, notfixed == 0

    for key in ("rm", "rm-gains"):
        want, fan, mag, fixed = sums(key)

        def run(mod, fmt, qs, key=key):
            o = d.full(B, lc.N, FILL[fmt], fmt)
            d.sync()
            hip.demap_rm(mod, rm, B, dev[key][0].data_ptr(), None if dev[key][1] is None else dev[key][1].data_ptr(), nv, o.data_ptr(), fmt, qs, False, None)
            return d.get(o, B, FILL[fmt])
        out.append(Entry(f"demap_rm {key}", run, want, fixed, np.maximum(fan, 1), mag))
    # two rounds into one soft buffer: "rm-gains" with accumulate 0, then "rm-round2" onto it
    w1, fan, g1, f1 = sums("rm-gains")
    w2, _, g2, f2 = sums("rm-round2")

    def run2(mod, fmt, qs):
        o = d.full(B, lc.N, FILL[fmt], fmt)
        d.sync()
        for key, acc in (("rm-gains", False), ("rm-round2", True)):
            hip.demap_rm(mod, rm, B, dev[key][0].data_ptr(), dev[key][1].data_ptr(), nv, o.data_ptr(), fmt, qs, acc, None)
        return d.get(o, B, FILL[fmt])

    def second_alone(mod):
        o = d.full(B, lc.N, FILL["f32"], "f32")
        d.sync()
        hip.demap_rm(mod, rm, B, dev["rm-round2"][0].data_ptr(), dev["rm-round2"][1].data_ptr(), nv, o.data_ptr(), "f32", 0.0, False, None)
        return d.get(o, B, FILL["f32"])
    e = Entry("demap_rm two rounds", run2, w1 + w2, f1 & f2, np.maximum(2 * fan, 1), g1 + g2)
    e.rounds = (out[-1].run, second_alone, sent)
    out.append(e)
    return out


@pytest.mark.parametrize("kind,n", lc.OBJECTS, ids=lc.IDS)
def test_logmap_against_the_spec(hip, kind, n):
    c = lc.case(kind, n)
    d = Dev()
    src = c.make(hip)
    mod, copy = src.with_rule("logmap"), src.with_rule("maxlog")
    assert (src.rule, mod.rule, copy.rule, mod.bits) == ("maxlog", "logmap", "maxlog", c.m)
    assert np.array_equal(mod.points, src.points) and mod.energy == src.energy and (mod.axis_levels is None) == (kind == "table")
    worst, calls = 0.0, 0
    for level in lc.LEVELS:
        keep = []
        for e in _entries(hip, d, c, level, keep):
            what = (kind, n, level, e.name)
            got, ml = e.run(mod, "f32", 0.0), e.run(src, "f32", 0.0)
            nan = np.isnan(e.want)
            assert np.array_equal(np.isnan(got), nan), (what, "NaN mask")
            gap, lim = np.abs(got.astype(np.float64) - e.want)[~nan], ls.bound(e.want, e.terms, e.mag)[~nan]
            print(f"{what}: worst gap {gap.max():.3e}, {float((gap / lim).max()):.3f} of the bound")
            assert (gap <= lim).all(), (what, gap.max(), float((gap / lim).max()))
            worst = max(worst, float((gap / lim).max()))
            fixed = np.broadcast_to(e.fixed, got.shape) if not c.single else np.ones(got.shape, bool)
            _same(np.where(fixed, got, 0), np.where(fixed, ml, 0), (what, "fixed points"))
            if level == "collapse":
                assert fixed.mean() > 0.5, (what, fixed.mean())
            elif not c.single and c.m > 2 and level == "low":
                assert (np.abs(got - ml)[~nan] > 0.05).any(), (what, "no correction at all")
            for fmt, code, qs in FMTS:
                if hasattr(e, "rounds"):                      # accumulate 1: the converter onto the first round's buffer in that format
                    first, second, sent = e.rounds
                    want_fmt = rs.combine(second(mod), sent, code, qs or 4.0, old=first(mod, fmt, qs))
                else:
                    want_fmt = _convert(got, code, qs or 4.0)
                got_fmt = got if fmt == "f32" and not hasattr(e, "rounds") else e.run(mod, fmt, qs)
                _same(got_fmt, want_fmt, (what, fmt, "the converter on the f32 output"))
                _same(e.run(copy, fmt, qs), ml if fmt == "f32" else e.run(src, fmt, qs), (what, fmt, "the max-log copy"))
                calls += 3
        for k in keep:
            if hasattr(k, "close"):
                k.close()
    print(f"{kind}-{n}: m = {c.m}, {calls} calls, worst gap {worst:.3f} of the bound")
    for o in (mod, copy, src):
        o.close()


def test_interface(hip):
    d = Dev()
    src = _source203(hip)
    il, fad = hip.Interleaver(np.arange(src.n_tx, dtype=np.int32), src.N), hip.Fading(4, 0.0)
    for make in (lambda: hip.Modulation("16qam"), lambda: hip.Modulation("64qam")):
        base = make()
        mod = base.with_rule(ls.LOGMAP)
        assert mod.rule == "logmap" and base.rule == "maxlog" and mod.with_rule("maxlog").rule == "maxlog"
        for bad in (-1, 2, 7, "exact"):
            with pytest.raises(hip.LdpcError) as err:
                base.with_rule(bad)
            assert err.value.code == hip.EINVAL and "rule" in str(err.value)
        Bs = 2
        llr = d.full(Bs, src.N, 777.0, "f32")
        d.sync()
        for call in (lambda m: src.sim.generate_mod(m, 5, 0, Bs, 4.0, llr.data_ptr()),
                     lambda m: src.sim.generate_mod_il(m, il, 5, 0, Bs, 4.0, llr.data_ptr()),
                     lambda m: src.sim.generate_mod_il_fading(m, il, fad, 5, 0, Bs, 4.0, llr.data_ptr())):
            with pytest.raises(hip.LdpcError) as err:
                call(mod)
            assert err.value.code == -5 and "log-MAP" in str(err.value) and "LDPC_DEMAP_LOGMAP" in str(err.value)     # LDPC_EUNSUPPORTED
            assert (d.get(llr, Bs, 777.0) == 777.0).all()
            call(mod.with_rule("maxlog"))
            assert (d.get(llr, Bs, 777.0) != 777.0).all()
            llr.fill_(777.0)
            d.sync()
        # the transmit-only calls ignore the rule: the same symbols
        ns = mod.symbols(src.n_tx)
        s0, s1 = d.full(Bs, 2 * ns, 777.0, "f32"), d.full(Bs, 2 * ns, 777.0, "f32")
        d.sync()
        src.sim.transmit(base, 5, 0, Bs, 4.0, s0.data_ptr())
        src.sim.transmit(mod, 5, 0, Bs, 4.0, s1.data_ptr())
        _same(d.get(s0, Bs, 777.0), d.get(s1, Bs, 777.0), "transmit")
        # the two-step route serves the log-MAP object
        hip.demap(mod, Bs, src.n_tx, src.N, s1.data_ptr(), src.sim.noise_var(mod, 4.0), llr.data_ptr(), "f32", 0.0, None)
        assert np.isfinite(d.get(llr, Bs, 777.0)).all()
    with pytest.raises(hip.LdpcError) as err:
        hip.lib().ldpc_modulation_with_rule(None, 1) or hip._lib.check(hip.lib().ldpc_last_error_code())
    assert err.value.code == hip.EINVAL
    il.close()
    src.close()
