#!/usr/bin/env python3
"""tools/encoder_rate.py [frames] [--sparse-only | --systematic-only | --messages caller | --modulation qpsk|8psk|table32|64qam|256qam|1024qam|4096qam|grid64 [--interleaver none|block|random [--fading BLOCK[,K]]]] -- device encoder throughput, quasi-cyclic rotate-and-xor (Fast/Encoder.hs:26-63,
sim.hip sim_parity_qc_kernel) against the dense packed GF(2) mat-vec of the expanded generator (Orig.hs:25-26), on the shipped AR4JA
codes: the encoder alone (ldpc_sim_encode_batch: messages + parity -> codeword bytes) and the whole frame source
(ldpc_sim_generate: + BPSK, AWGN, LLRs).  HIP events on the launch stream, median of 7.
Then the encoder FROM H (sim_sparse.hip) on the DVB-S2 structures of tests/dvbs2_short.py and tests/dvbs2_natural.py, in helper order:
the encoder alone, the whole generate, the encoder-less generate (all-zero codewords) of the same shape, and -- the yardstick: a BER
loop is at most doubled while generate costs no more than it -- the fp16-lam layered decode of that batch at 2 dB.  One warm-up,
median of 5.  --sparse-only: only that part.
--systematic-only: the encoder from ANY H (sim_systematic.hip, Sim(systematic=True)): on jpl.4096.4.5 next to the dense encoder of the
expanded generator (the same K x r product) and the quasi-cyclic one, codewords compared on the device and their SHA-256 printed; then on
codes/1920.1280.3.303 (no generator, not accumulator-shaped) generate against the fp16-lam layered decode of the same frames at 2 dB.
--messages caller: the caller's own messages (ldpc_sim_encode_messages) on the quasi-cyclic source of jpl.4096.4.5, the systematic form of
codes/1920.1280.3.303 (both [frames], default 65 536) and the encoder from H of tests/dvbs2_short.py (a quarter of that): bytes -> bytes and
packed -> packed next to ldpc_sim_encode_batch on the same source and batch and a device-to-device copy of batch * k bytes.  One warm-up,
median of 5.  The bar: bytes -> bytes <= encode_batch + 2 x that copy.
--modulation qpsk|8psk|table32: the modulated path (csrc/sim_mod.hip, csrc/demap.hip) on the quasi-cyclic source of jpl.4096.4.5: ldpc_sim_generate_mod
(float32 and int8 LLRs) next to ldpc_sim_generate of the same source and batch in the same run, ldpc_sim_transmit alone, and ldpc_demap_dev alone
into float32 and into int8 with the bytes it moves next to a device-to-device copy of as many bytes.  table32: a 4 + 12 + 16 ring table.  One
warm-up, median of 5; run each modulation as its own process under its own time limit.  The bar (qpsk only): generate_mod <= 1.25 x generate.
Where a lane's m LLRs fit no vector store (8psk, table32) the demapper stores them one by one; the LDS-transpose alternative lost the A/B
recorded in profiles/r14_modulation.txt and is not in the library.
--modulation 64qam|256qam|1024qam|4096qam: the same lines for the product built-ins (csrc/demap_product.hip, csrc/sim_mod_product.hip; no bar).
grid64: the 8 x 8 grid as a 64-point table object.  64qam also runs that table in the same process, the two alternating, and prints the one
bar of product constellations: ldpc_demap_dev -> f32 and ldpc_sim_generate_mod -> f32 on the product object no slower than on the table.
--interleaver none|block|random (with --modulation): the bit interleaver (csrc/demap_il.hip, csrc/sim_mod_il.hip) on the same source, after the
lines above.  none: the identity table; block: the block table of floor(n_tx / m) rows and m columns over the first rows * m bits, the last
n_tx mod m bits in place; random: a seeded random permutation of the transmitted prefix.  Into float32 and into int8, two rounds of the legs
alternating in this process, each leg one warm-up and the median of 5: ldpc_demap_dev | ldpc_demap_dev_il | ldpc_demap_dev into a
[batch][n_tx] buffer + ldpc_deinterleave_llr_dev (the two-pass baseline; its LLRs are compared with the fused ones bit for bit), and
ldpc_sim_generate_mod | ldpc_sim_generate_mod_il | ldpc_sim_transmit_il + ldpc_demap_dev_il (the only unfused way to the same LLRs).  No bar.
--fading BLOCK[,K] (with --modulation and --interleaver): ONLY the fading channel and the per-symbol channel state (csrc/demap_csi.hip,
csrc/sim_mod_fading.hip) on the same source and table, BLOCK symbols per fading block, Rician factor K (default 0): into float32 and into
int8, two rounds of the legs alternating, each leg one warm-up and the median of 5: ldpc_demap_dev_il | ldpc_demap_dev_il_csi (with the
bytes model (12 + m size) / (8 + m size) next to the measured ratio), and ldpc_sim_generate_mod_il | ldpc_sim_generate_mod_il_fading |
ldpc_sim_transmit_il_fading + ldpc_demap_dev_il_csi (its LLRs are compared with the fused ones bit for bit).  No bar."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecc_ldpc_amd as E  # noqa: E402


def timed(fn, stream, reps=7):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream); fn(); b.record(stream); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def sparse_leg(B, dev, st):
    import statistics
    from tests import dvbs2_natural, dvbs2_short
    for label, mod in (("dvbs2-short", dvbs2_short), ("dvbs2-natural", dvbs2_natural)):
        rp, ci = mod.csr()
        N, K = mod.N, mod.K
        perm, lp = E.Code.csr_layer_order(rp, ci, N)
        code = E.Code.from_csr(*E.Code.permute_rows(rp, ci, perm), N)
        code.set_layers(lp)
        sim = E.Sim(code, K, N, from_H=True, max_batch=B)
        plain = E.Sim(code, K, N, max_batch=B)
        assert (sim.encoder, plain.encoder) == ("sparse", "none")
        cw = torch.empty((B, N), dtype=torch.uint8, device=dev)
        llr = torch.empty((B, N), dtype=torch.float32, device=dev)
        t_enc = timed(lambda: sim.encode_batch(1, 0, B, cw.data_ptr(), None, st.cuda_stream), st, 5)
        t_zero = timed(lambda: plain.generate(1, 0, B, 2.0, llr.data_ptr(), None, st.cuda_stream), st, 5)
        t_gen = timed(lambda: sim.generate(1, 0, B, 2.0, llr.data_ptr(), None, st.cuda_stream), st, 5)
        ones = float(cw[:, K:].float().mean())
        del cw
        dec = E.Decoder(code, "min", "f16", B, schedule="layered")
        bits = torch.empty((B, N), dtype=torch.uint8, device=dev)
        its = torch.empty(B, dtype=torch.int32, device=dev)
        conv = torch.empty(B, dtype=torch.uint8, device=dev)
        dec.set_timing(True)
        ts = []
        for r in range(6):                                           # the first launch warms up
            dec.decode_batch_dev(llr.data_ptr(), bits.data_ptr(), B, 50, its.data_ptr(), conv.data_ptr(), st.cuda_stream)
            dec.synchronize(); torch.cuda.synchronize()
            n, ms = dec.kernel_time()
            if r:
                ts.append(ms / max(n, 1))
        t_dec = statistics.median(ts)
        tally = torch.zeros(4, dtype=torch.int64, device=dev)
        sim.tally(B, bits.data_ptr(), its.data_ptr(), tally.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize()
        fr, fe, be, _ = tally.cpu().tolist()
        print(f"{label:14s} N={N} K={K} sparse encoder (from H, helper order): {B} frames  encode_batch {t_enc:7.3f} ms = {B * K / t_enc / 1e6:8.1f} Gbit/s info"
              f" | generate {t_gen:7.3f} ms | encoder-less generate {t_zero:7.3f} ms | parity ones {ones:.4f}", flush=True)
        print(f"{'':14s} fp16-lam layered decode of that batch at 2 dB ({dec.kernel_name}): {t_dec:7.3f} ms, sweeps {float(its.float().mean()):.2f}, "
              f"converged {float(conv.float().mean()):.4f}, tally {fr} frames {fe} frame errors {be} message-bit errors"
              f" | generate / decode = {t_gen / t_dec:.3f} ({'within' if t_gen <= t_dec else 'MISSES'} the bar generate <= decode)", flush=True)
        dec.close(); sim.close(); plain.close(); code.close()
        del llr, bits
        torch.cuda.empty_cache()


def decode_time(code, llr, B, N, dev, st):
    """-> (median kernel ms of five fp16-lam layered decodes after a warm-up, decoder, bits, its, conv)"""
    import statistics
    dec = E.Decoder(code, "min", "f16", B, schedule="layered")
    bits = torch.empty((B, N), dtype=torch.uint8, device=dev)
    its = torch.empty(B, dtype=torch.int32, device=dev)
    conv = torch.empty(B, dtype=torch.uint8, device=dev)
    dec.set_timing(True)
    ts = []
    for r in range(6):                                           # the first launch warms up
        dec.decode_batch_dev(llr.data_ptr(), bits.data_ptr(), B, 50, its.data_ptr(), conv.data_ptr(), st.cuda_stream)
        dec.synchronize(); torch.cuda.synchronize()
        n, ms = dec.kernel_time()
        if r:
            ts.append(ms / max(n, 1))
    return statistics.median(ts), dec, bits, its, conv


def sha(t):
    import hashlib
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]


def systematic_leg(B, dev, st):
    from tests.helpers import load
    name = "ldpc/hip-minsum/jpl.4096.4.5/50/4/5"
    c = load("jpl.4096.4.5")
    cws = {}
    for enc in ("dense", "qc", "systematic", "dense", "systematic"):     # the two compared legs twice, alternating: their spread
        ecc = None
        if enc == "systematic":
            code = c.hip_code(E)
            sim = E.Sim(code, None, c.n_tx, systematic=True, max_batch=B)
            k, n_tx, N = sim.k, c.n_tx, c.N
        else:
            if enc == "dense":
                os.environ["LDPC_SIM_ENCODER"] = "dense"
            else:
                os.environ.pop("LDPC_SIM_ENCODER", None)
            ecc = E.ECC(os.path.join(ROOT, "codes"), name, max_batch=B)
            sim, k, n_tx, N = ecc.sim, ecc.message_length, ecc.codeword_length, ecc.unpunctured_length
        assert sim.encoder == enc and (k, n_tx, N) == (c.k, c.n_tx, c.N)
        cw = torch.empty((B, n_tx), dtype=torch.uint8, device=dev)
        llr = torch.empty((B, N), dtype=torch.float32, device=dev)
        t_enc = timed(lambda: sim.encode_batch(1, 0, B, cw.data_ptr(), None, st.cuda_stream), st)
        t_gen = timed(lambda: sim.generate(1, 0, B, 2.0, llr.data_ptr(), None, st.cuda_stream), st)
        print(f"jpl.4096.4.5 {enc:10s} encoder: {B} frames  encode_batch {t_enc:7.3f} ms = {B * k / t_enc / 1e6:8.1f} Gbit/s info"
              f" | generate (encode + AWGN + LLR) {t_gen:7.3f} ms | codewords sha256 {sha(cw)} LLRs sha256 {sha(llr)}", flush=True)
        if enc in cws:
            assert torch.equal(cws[enc], cw)
        cws[enc] = cw
        (ecc or sim).close()
        if ecc is None:
            code.close()
        del llr
    assert torch.equal(cws["dense"], cws["systematic"]) and torch.equal(cws["qc"], cws["systematic"]), "encoders disagree"
    print("             codewords of the dense, quasi-cyclic and systematic encoders identical", flush=True)
    cws.clear()
    torch.cuda.empty_cache()
    m = load("1920.1280.3.303")
    rp, ci, N = m.graph.row_ptr, m.graph.col_idx, m.N
    perm, lp = E.Code.csr_layer_order(rp, ci, N)
    code = E.Code.from_csr(*E.Code.permute_rows(rp, ci, perm), N)
    code.set_layers(lp)
    sim = E.Sim(code, None, N, systematic=True, max_batch=B)
    K = sim.k
    plain = E.Sim(code, K, N, max_batch=B)
    assert (sim.encoder, plain.encoder) == ("systematic", "none")
    cw = torch.empty((B, N), dtype=torch.uint8, device=dev)
    llr = torch.empty((B, N), dtype=torch.float32, device=dev)
    t_enc = timed(lambda: sim.encode_batch(1, 0, B, cw.data_ptr(), None, st.cuda_stream), st, 5)
    t_zero = timed(lambda: plain.generate(1, 0, B, 2.0, llr.data_ptr(), None, st.cuda_stream), st, 5)
    t_gen = timed(lambda: sim.generate(1, 0, B, 2.0, llr.data_ptr(), None, st.cuda_stream), st, 5)
    par = torch.from_numpy(sim.positions()[1].astype("int64")).to(dev)
    ones = float(cw[:, par].float().mean())
    del cw
    t_dec, dec, bits, its, conv = decode_time(code, llr, B, N, dev, st)
    tally = torch.zeros(4, dtype=torch.int64, device=dev)
    sim.tally(B, bits.data_ptr(), its.data_ptr(), tally.data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    fr, fe, be, _ = tally.cpu().tolist()
    print(f"1920.1280.3.303 N={N} K={K} systematic encoder (from H, helper order): {B} frames  encode_batch {t_enc:7.3f} ms = {B * K / t_enc / 1e6:8.1f} Gbit/s info"
          f" | generate {t_gen:7.3f} ms | encoder-less generate {t_zero:7.3f} ms | parity ones {ones:.4f}", flush=True)
    print(f"{'':15s} fp16-lam layered decode of that batch at 2 dB ({dec.kernel_name}): {t_dec:7.3f} ms, sweeps {float(its.float().mean()):.2f}, "
          f"converged {float(conv.float().mean()):.4f}, tally {fr} frames {fe} frame errors {be} message-bit errors"
          f" | generate / decode = {t_gen / t_dec:.3f} ({'within' if t_gen <= t_dec else 'MISSES'} the bar generate <= decode)", flush=True)
    dec.close(); sim.close(); plain.close(); code.close()


def caller_leg(B, dev, st):
    from tests import dvbs2_short
    from tests.helpers import load

    def qc():
        ecc = E.ECC(os.path.join(ROOT, "codes"), "ldpc/hip-minsum/jpl.4096.4.5/50/4/5", max_batch=B)
        return ecc.sim, ecc.codeword_length, B, [ecc]

    def systematic():
        m = load("1920.1280.3.303")
        code = E.Code.from_csr(m.graph.row_ptr, m.graph.col_idx, m.N)
        return E.Sim(code, None, m.N, systematic=True, max_batch=B), m.N, B, [code]

    def sparse():
        Bs = max(1, B // 4)
        code = E.Code.from_csr(*dvbs2_short.csr(), dvbs2_short.N)
        return E.Sim(code, dvbs2_short.K, dvbs2_short.N, from_H=True, max_batch=Bs), dvbs2_short.N, Bs, [code]

    print(f"{'source':34s} {'frames':>7s} {'bytes->bytes':>13s} {'packed->packed':>15s} {'encode_batch':>13s} {'copy batch*k B':>15s} {'bar':>9s}  (ms, median of 5)")
    for label, make in (("qc jpl.4096.4.5", qc), ("systematic 1920.1280.3.303", systematic), ("sparse dvbs2-short", sparse)):
        sim, n_tx, b, owners = make()
        k = sim.k
        kb, pb = 4 * ((k + 31) // 32), (n_tx + 7) // 8
        msg = torch.empty((b, k), dtype=torch.uint8, device=dev)
        cw = torch.empty((b, n_tx), dtype=torch.uint8, device=dev)
        cw2 = torch.empty((b, n_tx), dtype=torch.uint8, device=dev)
        sim.encode_batch(1, 0, b, cw.data_ptr(), msg.data_ptr(), st.cuda_stream)      # the messages it draws: the same work for every leg
        w = torch.arange(8, device=dev, dtype=torch.int32)
        pmsg = torch.zeros((b, kb), dtype=torch.uint8, device=dev)
        bits = torch.nn.functional.pad(msg, (0, 8 * kb - k)).view(b, kb, 8).to(torch.int32)
        pmsg.copy_((bits << w).sum(-1).to(torch.uint8))
        pcw = torch.empty((b, pb), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(msg)
        torch.cuda.synchronize()
        t_bb = timed(lambda: sim.encode_messages(b, msg.data_ptr(), cw2.data_ptr(), "bytes", "bytes", st.cuda_stream), st, 5)
        t_pp = timed(lambda: sim.encode_messages(b, pmsg.data_ptr(), pcw.data_ptr(), "packed", "packed", st.cuda_stream), st, 5)
        t_enc = timed(lambda: sim.encode_batch(1, 0, b, cw.data_ptr(), None, st.cuda_stream), st, 5)
        t_cp = timed(lambda: dst.copy_(msg), st, 5)
        assert torch.equal(cw, cw2), "encode_messages and encode_batch disagree on the same messages"
        cbits = torch.nn.functional.pad(cw, (0, 8 * pb - n_tx)).view(b, pb, 8).to(torch.int32)
        assert torch.equal(pcw, (cbits << w).sum(-1).to(torch.uint8)), "packed codewords differ from the packed bytes"
        bar = t_enc + 2 * t_cp
        print(f"{label:34s} {b:7d} {t_bb:13.3f} {t_pp:15.3f} {t_enc:13.3f} {t_cp:15.3f} {bar:9.3f}  bytes->bytes {'within' if t_bb <= bar else 'MISSES'} the bar"
              f" (encode_batch + 2 copies); packed->packed / bytes->bytes = {t_pp / t_bb:.3f}", flush=True)
        sim.close()
        for o in owners:
            o.close()
        del msg, cw, cw2, pmsg, pcw, dst, bits, cbits
        torch.cuda.empty_cache()


PRODUCT_BUILTINS = ("64qam", "256qam", "1024qam", "4096qam")


def make_modulation(which):
    import numpy as np
    from tests import modulation_spec as ms
    if which in PRODUCT_BUILTINS:
        return E.Modulation(which)
    pts = {"qpsk": lambda: ms.builtin(ms.QPSK), "8psk": lambda: ms.builtin(ms.PSK8), "grid64": ms.grid64,
           "table32": lambda: ms.rings((1.0, 2.84, 5.27), (4, 12, 16), (np.pi / 4, np.pi / 12, 0.0))}[which]()
    return E.Modulation(pts)


def table_positions(kind, n_tx, m):
    """none: the identity; block: floor(n_tx / m) rows and m columns over the first rows * m bits, the rest in place; random: seeded"""
    import numpy as np
    if kind == "none":
        return np.arange(n_tx)
    if kind == "block":
        rows = n_tx // m
        return np.concatenate([E.Interleaver.block_positions(rows, m), np.arange(rows * m, n_tx)])
    return np.random.default_rng(1).permutation(n_tx)


def modulation_leg(which, B, dev, st, interleaver=None):
    from tests import modulation_spec as ms
    mod = make_modulation(which)
    m = mod.bits
    ecc = E.ECC(os.path.join(ROOT, "codes"), "ldpc/hip-minsum/jpl.4096.4.5/50/4/5", max_batch=B)
    sim, k, n_tx, N = ecc.sim, ecc.message_length, ecc.codeword_length, ecc.unpunctured_length
    ns = mod.symbols(n_tx)
    s_ = st.cuda_stream
    llr = torch.empty((B, N), dtype=torch.float32, device=dev)
    q = torch.empty((B, N), dtype=torch.int8, device=dev)
    sym = torch.empty((B, ns, 2), dtype=torch.float32, device=dev)
    nv = sim.noise_var(mod, 2.0)
    t_gen = timed(lambda: sim.generate(1, 0, B, 2.0, llr.data_ptr(), None, s_), st, 5)
    t_mod = timed(lambda: sim.generate_mod(mod, 1, 0, B, 2.0, llr.data_ptr(), "f32", 0.0, None, "bytes", None, s_), st, 5)
    t_gen2 = timed(lambda: sim.generate(1, 0, B, 2.0, llr.data_ptr(), None, s_), st, 5)           # again, after: the spread of the yardstick
    t_mod8 = timed(lambda: sim.generate_mod(mod, 1, 0, B, 2.0, q.data_ptr(), "i8", 4.0, None, "bytes", None, s_), st, 5)
    t_tx = timed(lambda: sim.transmit(mod, 1, 0, B, 2.0, sym.data_ptr(), None, "bytes", None, s_), st, 5)
    print(f"jpl.4096.4.5 qc source, {which} (m = {m}, {ns} symbols a frame), {B} frames, 2 dB, median of 5 (ms):", flush=True)
    gen = min(t_gen, t_gen2)
    bar = f" ({'within' if t_mod <= 1.25 * gen else 'MISSES'} the bar 1.25)" if which == "qpsk" else " (no bar)"
    print(f"  ldpc_sim_generate f32 {t_gen:8.3f} (again {t_gen2:8.3f}) | ldpc_sim_generate_mod f32 {t_mod:8.3f} = {t_mod / gen:.3f} x generate"
          f"{bar} | generate_mod int8 {t_mod8:8.3f} | ldpc_sim_transmit {t_tx:8.3f}", flush=True)
    for fmt, out, size in (("f32", llr, 4), ("i8", q, 1)):
        nbytes = B * (ns * 8 + N * size)
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        t_dm = timed(lambda: E.demap(mod, B, n_tx, N, sym.data_ptr(), nv, out.data_ptr(), fmt, 4.0, s_), st, 5)
        t_cp = timed(lambda: dst.copy_(src), st, 5)            # reads nbytes / 2 and writes nbytes / 2: the same bytes moved
        print(f"  ldpc_demap_dev -> {fmt:3s} {t_dm:8.3f} ms, {nbytes / 1e6:9.1f} MB moved = {nbytes / t_dm / 1e9:7.2f} TB/s | device copy of as many bytes {t_cp:8.3f} ms"
              f" = {nbytes / t_cp / 1e9:7.2f} TB/s | demap / copy = {t_dm / t_cp:.2f}", flush=True)
        del src, dst
    # the fused kernel against its two halves on this run's data
    two = torch.empty((B, N), dtype=torch.float32, device=dev)
    sim.generate_mod(mod, 1, 0, B, 2.0, llr.data_ptr(), "f32", 0.0, None, "bytes", None, s_)
    sim.transmit(mod, 1, 0, B, 2.0, sym.data_ptr(), None, "bytes", None, s_)
    E.demap(mod, B, n_tx, N, sym.data_ptr(), nv, two.data_ptr(), "f32", 0.0, s_)
    torch.cuda.synchronize()
    assert torch.equal(llr.view(torch.int32), two.view(torch.int32)), "generate_mod differs from transmit + demap"
    print(f"  generate_mod = transmit + demap bit for bit; LLRs sha256 {sha(llr[:256])}", flush=True)
    if which == "64qam":
        # the bar: the product object against the same 64 points as a table, alternating in this process; the samples demapped are this
        # run's 64qam symbols for both (the two level sets are the same, only the labels differ)
        tab = E.Modulation(ms.grid64())
        assert tab.bits == m
        res = {}
        for rep in range(2):
            for label, o in (("product", mod), ("table", tab)):
                t_d = timed(lambda: E.demap(o, B, n_tx, N, sym.data_ptr(), nv, llr.data_ptr(), "f32", 4.0, s_), st, 5)
                t_g = timed(lambda: sim.generate_mod(o, 1, 0, B, 2.0, llr.data_ptr(), "f32", 0.0, None, "bytes", None, s_), st, 5)
                res.setdefault(label, []).append((t_d, t_g))
        for i, call in enumerate(("ldpc_demap_dev -> f32", "ldpc_sim_generate_mod -> f32")):
            p, t = [r[i] for r in res["product"]], [r[i] for r in res["table"]]
            print(f"  {call:30s} product object {p[0]:8.3f} {p[1]:8.3f} ms | 64-point table (grid64) {t[0]:8.3f} {t[1]:8.3f} ms | product / table = {min(p) / min(t):.3f}"
                  f" ({'within' if max(p) <= min(t) else 'MISSES'} the bar: no slower)", flush=True)
        tab.close()
    if interleaver:
        sim.transmit(mod, 1, 0, B, 2.0, sym.data_ptr(), None, "bytes", None, s_)
        torch.cuda.synchronize()
        del llr, q, two
        interleaver_leg(interleaver, mod, sim, B, n_tx, N, sym, nv, dev, st)
    mod.close(); ecc.close()


def interleaver_leg(kind, mod, sim, B, n_tx, N, sym, nv, dev, st):
    m, s_ = mod.bits, st.cuda_stream
    il = E.Interleaver(table_positions(kind, n_tx, m), N)
    ns = mod.symbols(n_tx)
    print(f"  interleaver {kind}: n_tx = {n_tx}, N = {N}, {N - n_tx} punctured; two rounds, legs alternating, each one warm-up + median of 5 (ms):", flush=True)
    for fmt, dt, size in (("f32", torch.float32, 4), ("i8", torch.int8, 1)):
        out = torch.empty((B, N), dtype=dt, device=dev)
        two = torch.empty((B, N), dtype=dt, device=dev)
        mid = torch.empty((B, n_tx), dtype=dt, device=dev)

        def two_pass():
            E.demap(mod, B, n_tx, n_tx, sym.data_ptr(), nv, mid.data_ptr(), fmt, 4.0, s_)
            E.deinterleave_llr(il, B, mid.data_ptr(), two.data_ptr(), fmt, s_)

        def unfused():
            sim.transmit_il(mod, il, 1, 0, B, 2.0, sym.data_ptr(), None, "bytes", None, s_)
            E.demap_il(mod, il, B, sym.data_ptr(), nv, two.data_ptr(), fmt, 4.0, s_)

        demap_legs = (("ldpc_demap_dev", lambda: E.demap(mod, B, n_tx, N, sym.data_ptr(), nv, out.data_ptr(), fmt, 4.0, s_)),
                      ("ldpc_demap_dev_il", lambda: E.demap_il(mod, il, B, sym.data_ptr(), nv, out.data_ptr(), fmt, 4.0, s_)),
                      ("demap + deinterleave_llr", two_pass))
        gen_legs = (("ldpc_sim_generate_mod", lambda: sim.generate_mod(mod, 1, 0, B, 2.0, out.data_ptr(), fmt, 4.0, None, "bytes", None, s_)),
                    ("ldpc_sim_generate_mod_il", lambda: sim.generate_mod_il(mod, il, 1, 0, B, 2.0, out.data_ptr(), fmt, 4.0, None, "bytes", None, s_)),
                    ("transmit_il + demap_il", unfused))
        for legs, what in ((demap_legs, "demap"), (gen_legs, "generate_mod")):
            res = {name: [] for name, _ in legs}
            for _ in range(2):
                for name, fn in legs:
                    res[name].append(timed(fn, st, 5))
            base, fused, other = (res[name] for name, _ in legs)
            nbytes = B * (ns * 8 + N * size)
            extra = f" | {nbytes / 1e6:.1f} MB moved: {nbytes / min(base) / 1e9:.2f} and {nbytes / min(fused) / 1e9:.2f} TB/s" if what == "demap" else ""
            print(f"  -> {fmt:3s} " + " | ".join(f"{name} {t[0]:8.3f} {t[1]:8.3f}" for name, t in res.items())
                  + f" | fused / plain = {min(fused) / min(base):.3f}, fused / two-pass = {min(fused) / min(other):.3f}{extra}", flush=True)
            if what == "demap":
                E.demap_il(mod, il, B, sym.data_ptr(), nv, out.data_ptr(), fmt, 4.0, s_)
                two_pass()
            else:
                unfused()
                sim.generate_mod_il(mod, il, 1, 0, B, 2.0, out.data_ptr(), fmt, 4.0, None, "bytes", None, s_)
            torch.cuda.synchronize()
            iv = torch.int32 if fmt == "f32" else torch.int8
            assert torch.equal(out.view(iv), two.view(iv)), f"{what}: the fused LLRs differ from the two-pass ones ({fmt})"
        del out, two, mid
    print(f"  fused = two-pass bit for bit (demap_il = demap + deinterleave_llr; generate_mod_il = transmit_il + demap_il)", flush=True)
    il.close()


def fading_leg(which, kind, block, K, B, dev, st):
    mod = make_modulation(which)
    m, s_ = mod.bits, st.cuda_stream
    ecc = E.ECC(os.path.join(ROOT, "codes"), "ldpc/hip-minsum/jpl.4096.4.5/50/4/5", max_batch=B)
    sim, n_tx, N = ecc.sim, ecc.codeword_length, ecc.unpunctured_length
    ns = mod.symbols(n_tx)
    il = E.Interleaver(table_positions(kind, n_tx, m), N)
    fad = E.Fading(block, K)
    db = 2.0
    nv = sim.noise_var(mod, db)
    sym = torch.empty((B, ns, 2), dtype=torch.float32, device=dev)
    gain = torch.empty((B, ns), dtype=torch.float32, device=dev)
    sim.transmit_il_fading(mod, il, fad, 1, 0, B, db, sym.data_ptr(), gain.data_ptr(), None, "bytes", None, s_)
    torch.cuda.synchronize()
    print(f"jpl.4096.4.5 qc source, {which} (m = {m}, {ns} symbols a frame), interleaver {kind}, fading block = {block}, K = {K:g}, {B} frames, {db} dB; mean gain "
          f"{float(gain.mean()):.4f}; two rounds, legs alternating, each one warm-up + median of 5 (ms):", flush=True)
    for fmt, dt, size in (("f32", torch.float32, 4), ("i8", torch.int8, 1)):
        out = torch.empty((B, N), dtype=dt, device=dev)
        two = torch.empty((B, N), dtype=dt, device=dev)

        def unfused():
            sim.transmit_il_fading(mod, il, fad, 1, 0, B, db, sym.data_ptr(), gain.data_ptr(), None, "bytes", None, s_)
            E.demap_il_csi(mod, il, B, sym.data_ptr(), gain.data_ptr(), nv, two.data_ptr(), fmt, 4.0, s_)

        demap_legs = (("ldpc_demap_dev_il", lambda: E.demap_il(mod, il, B, sym.data_ptr(), nv, out.data_ptr(), fmt, 4.0, s_)),
                      ("ldpc_demap_dev_il_csi", lambda: E.demap_il_csi(mod, il, B, sym.data_ptr(), gain.data_ptr(), nv, out.data_ptr(), fmt, 4.0, s_)))
        gen_legs = (("ldpc_sim_generate_mod_il", lambda: sim.generate_mod_il(mod, il, 1, 0, B, db, out.data_ptr(), fmt, 4.0, None, "bytes", None, s_)),
                    ("ldpc_sim_generate_mod_il_fading", lambda: sim.generate_mod_il_fading(mod, il, fad, 1, 0, B, db, out.data_ptr(), fmt, 4.0, None, None, "bytes", None, s_)),
                    ("transmit_il_fading + demap_il_csi", unfused))
        for legs, what in ((demap_legs, "demap"), (gen_legs, "generate_mod")):
            res = {name: [] for name, _ in legs}
            for _ in range(2):
                for name, fn in legs:
                    res[name].append(timed(fn, st, 5))
            ts = [res[name] for name, _ in legs]
            line = f"  -> {fmt:3s} " + " | ".join(f"{name} {t[0]:8.3f} {t[1]:8.3f}" for name, t in res.items())
            if what == "demap":
                model = (12.0 + m * size) / (8.0 + m * size)
                nbytes = B * (ns * 12 + N * size)
                line += f" | csi / plain = {min(ts[1]) / min(ts[0]):.3f} (bytes model {model:.3f}) | {nbytes / 1e6:.1f} MB moved = {nbytes / min(ts[1]) / 1e9:.2f} TB/s"
            else:
                line += f" | fading / awgn = {min(ts[1]) / min(ts[0]):.3f} (one more Philox call a lane), fused / two-step = {min(ts[1]) / min(ts[2]):.3f}"
            print(line, flush=True)
        unfused()
        sim.generate_mod_il_fading(mod, il, fad, 1, 0, B, db, out.data_ptr(), fmt, 4.0, None, None, "bytes", None, s_)
        torch.cuda.synchronize()
        iv = torch.int32 if fmt == "f32" else torch.int8
        assert torch.equal(out.view(iv), two.view(iv)), f"generate_mod_il_fading differs from transmit_il_fading + demap_il_csi ({fmt})"
        del out, two
    print("  generate_mod_il_fading = transmit_il_fading + demap_il_csi bit for bit", flush=True)
    il.close(); mod.close(); ecc.close()


def main():
    argv = sys.argv[1:]
    fading = None
    if "--fading" in argv:
        i = argv.index("--fading")
        try:
            parts = argv[i + 1].split(",")
            fading = (int(parts[0]), float(parts[1]) if len(parts) > 1 else 0.0)
            assert len(parts) <= 2
        except (IndexError, ValueError, AssertionError):
            sys.exit("--fading takes BLOCK[,K]: symbols per fading block and the Rician factor")
        del argv[i:i + 2]
        if "--modulation" not in argv or "--interleaver" not in argv:
            sys.exit("--fading goes with --modulation and --interleaver")
    messages = None
    modulation = None
    interleaver = None
    if "--interleaver" in argv:
        i = argv.index("--interleaver")
        interleaver = argv[i + 1] if i + 1 < len(argv) else ""
        del argv[i:i + 2]
        if interleaver not in ("none", "block", "random") or "--modulation" not in argv:
            sys.exit("--interleaver takes one value: none, block or random, and goes with --modulation")
    if "--modulation" in argv:
        i = argv.index("--modulation")
        modulation = argv[i + 1] if i + 1 < len(argv) else ""
        del argv[i:i + 2]
        if modulation not in ("qpsk", "8psk", "table32", "grid64") + PRODUCT_BUILTINS:
            sys.exit("--modulation takes one value: qpsk, 8psk, table32, grid64, 64qam, 256qam, 1024qam or 4096qam")
    if "--messages" in argv:
        i = argv.index("--messages")
        messages = argv[i + 1] if i + 1 < len(argv) else ""
        del argv[i:i + 2]
        if messages != "caller":
            sys.exit("--messages takes one value: caller")
    args = [a for a in argv if not a.startswith("--")]
    B = int(args[0]) if args else 65536
    E.init(0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    if fading:
        fading_leg(modulation, interleaver, fading[0], fading[1], B, dev, st)
        return
    if modulation:
        modulation_leg(modulation, B, dev, st, interleaver)
        return
    if messages:
        caller_leg(B, dev, st)
        return
    if "--systematic-only" in sys.argv:
        systematic_leg(B, dev, st)
        return
    if "--sparse-only" in sys.argv:
        sparse_leg(B, dev, st)
        return
    for name in ("ldpc/hip-minsum/jpl.1024.4.5/50/4/5", "ldpc/hip-minsum/jpl.4096.4.5/50/4/5"):
        rows = {}
        for enc in ("qc", "dense"):
            if enc == "dense":
                os.environ["LDPC_SIM_ENCODER"] = "dense"
            else:
                os.environ.pop("LDPC_SIM_ENCODER", None)
            ecc = E.ECC(os.path.join(ROOT, "codes"), name, max_batch=B)
            k, n_tx, N = ecc.message_length, ecc.codeword_length, ecc.unpunctured_length
            assert ecc.sim.encoder == enc
            cw = torch.empty((B, n_tx), dtype=torch.uint8, device=dev)
            llr = torch.empty((B, N), dtype=torch.float32, device=dev)
            t_enc = timed(lambda: ecc.sim.encode_batch(1, 0, B, cw.data_ptr(), None, st.cuda_stream), st)
            t_gen = timed(lambda: ecc.sim.generate(1, 0, B, 2.0, llr.data_ptr(), None, st.cuda_stream), st)
            rows[enc] = (t_enc, t_gen, cw.cpu().numpy().copy())
            print(f"{name:42s} {enc:5s} encoder: {B} frames  encode_batch {t_enc:7.3f} ms = {B / t_enc / 1e3:8.2f} Mframes/s = {B * k / t_enc / 1e6:8.1f} Gbit/s info"
                  f" | generate (encode + AWGN + LLR) {t_gen:7.3f} ms", flush=True)
            ecc.close()
            del cw, llr
        assert (rows["qc"][2] == rows["dense"][2]).all(), "encoders disagree"
        print(f"{'':42s} codewords identical; qc/dense time: encode {rows['qc'][0] / rows['dense'][0]:.2f}, generate {rows['qc'][1] / rows['dense'][1]:.2f}")
    sparse_leg(B, dev, st)


if __name__ == "__main__":
    main()
