"""The BCH rule of include/ldpc_hip.h (ldpc_bch; csrc/bch.cc, csrc/bch.hip), restated with Python integers and numpy.  All integer
arithmetic, so everything that compares against this compares with equality.

  FIELD      GF(2^m), m = 3..16, from prim_poly (the x^m term included); alpha = x; N0 = 2^m - 1; x must have order N0.
  GENERATOR  g = the product of the distinct minimal polynomials of alpha^1 .. alpha^(2t), t = 1..16, 2t < N0; p = deg g; p < n <= N0; k = n - p.
  ROW        bit i, i = 0..n-1, is the coefficient of x^(n-1-i): bits 0..k-1 the message, bits k..n-1 the remainder of m(x) x^p mod g, MSB
             first.  Packed rows: bit i in byte i/8 at bit i%8, 4 * ceil(n/32) bytes a row.
  ENCODE     in place.  Bytes: bit 0 of a message byte is read, the byte is kept; the parity bytes are 0 / 1.  Packed: message bits kept,
             bits >= n written 0.
  DECODE     the codeword within Hamming distance e <= t of the row (unique if it exists) replaces it, nerr = e; otherwise the row stays
             exactly as it was, nerr = -1.  A correction flips bit 0 of a byte, or the one bit of a packed row.
A polynomial over GF(2) is a Python int here, bit b = the coefficient of x^b; a row is the int whose bit n-1-i is row bit i.  The decoder
is Berlekamp-Massey and a Chien search with the acceptance "L <= t, deg Lambda = L, exactly L roots, all at positions < n";
tests/test_bch_spec.py holds it to the definition above by brute force over every word of six small codes."""
import numpy as np

# kind (the integer of LDPC_BCH_*) -> (name, m, prim_poly, t).  Defined by formula; no claim that they are any standard's
BUILTINS = {0: ("m16t8", 16, 0x1002D, 8), 1: ("m16t10", 16, 0x1002D, 10), 2: ("m16t12", 16, 0x1002D, 12), 3: ("m14t12", 14, 0x402B, 12)}

# (prim_poly, m, t) -> p = deg g
PARITY_LENGTHS = {(0xB, 3, 1): 3, (0x13, 4, 2): 8, (0x13, 4, 3): 10, (0x25, 5, 2): 10, (0x11D, 8, 4): 32, (0x11D, 8, 16): 124, (0x805, 11, 4): 44,
                  (0x402B, 14, 12): 168, (0x1002D, 16, 12): 192, (0x1002D, 16, 16): 256}


def poly_mod(a, g):
    """a mod g over GF(2)"""
    dg = g.bit_length() - 1
    while a.bit_length() > dg:
        a ^= g << (a.bit_length() - 1 - dg)
    return a


def poly_mul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        b >>= 1
    return r


def row_bytes(n):
    return 4 * ((n + 31) // 32)


def pack(bits):
    """bits [B][n] (bit 0 of each) -> packed rows [B][4 * ceil(n/32)] uint8, bit i in byte i/8 at bit i%8, pad bits 0"""
    b = np.asarray(bits, np.uint8) & 1
    n = b.shape[-1]
    pad = np.zeros(b.shape[:-1] + (8 * row_bytes(n) - n,), np.uint8)
    return np.packbits(np.concatenate([b, pad], -1), axis=-1, bitorder="little")


def unpack(rows, n):
    """packed rows -> bits [B][n] uint8"""
    return np.unpackbits(np.asarray(rows, np.uint8), axis=-1, bitorder="little")[..., :n]


class Code:
    def __init__(self, m, prim_poly, t, n):
        if not 3 <= m <= 16:
            raise ValueError(f"m = {m} outside 3..16")
        if not 1 <= t <= 16:
            raise ValueError(f"t = {t} outside 1..16")
        if prim_poly >> m != 1:
            raise ValueError(f"prim_poly = {prim_poly:#x} is not of degree m = {m}")
        N0 = (1 << m) - 1
        exp, log, a = [], [0] * (N0 + 1), 1
        for i in range(N0):
            if i and a == 1:
                raise ValueError(f"prim_poly = {prim_poly:#x} is not primitive: x has order {i}")
            exp.append(a)
            log[a] = i
            a <<= 1
            if a >> m:
                a ^= prim_poly
        if a != 1:
            raise ValueError(f"prim_poly = {prim_poly:#x} is not primitive")
        if 2 * t >= N0:
            raise ValueError(f"t = {t}: 2t must be below 2^m - 1 = {N0}")
        self.m, self.prim_poly, self.t, self.n, self.N0 = m, prim_poly, t, n, N0
        self.exp, self.log = exp + exp, log
        self.exp_np, self.log_np = np.array(self.exp, np.int64), np.array(log, np.int64)
        g, seen = 1, set()
        for j in range(1, 2 * t + 1):
            if j in seen:
                continue
            mp, e = [1], j                                                   # the product of (x + alpha^e) over the coset of j, low coefficient first
            while e not in seen:
                seen.add(e)
                root = exp[e]
                mp = [self.mul(mp[0], root)] + [mp[d - 1] ^ (self.mul(mp[d], root) if d < len(mp) else 0) for d in range(1, len(mp) + 1)]
                e = e * 2 % N0
            assert all(c in (0, 1) for c in mp) and mp[-1] == 1              # a minimal polynomial is binary and monic
            g = poly_mul(g, sum(c << d for d, c in enumerate(mp)))
        self.g, self.p = g, g.bit_length() - 1
        if not self.p < n <= N0:
            raise ValueError(f"n = {n} outside p + 1 .. 2^m - 1 (p = {self.p})")
        self.k = n - self.p
        self._located = {0: ()}

    def mul(self, a, b):
        return self.exp[self.log[a] + self.log[b]] if a and b else 0

    def generator(self):
        """g [p + 1] uint8, g[j] = the coefficient of x^j"""
        return np.array([(self.g >> j) & 1 for j in range(self.p + 1)], np.uint8)

    # ---- rows as integers
    def row_int(self, bits):
        """bits [n] 0 / 1 -> the int whose bit n-1-i is bits[i]"""
        b = np.asarray(bits, np.uint8) & 1
        assert b.shape == (self.n,)
        return int.from_bytes(np.packbits(b, bitorder="big").tobytes(), "big") >> (-self.n % 8)

    def int_row(self, v):
        return np.array([(v >> (self.n - 1 - i)) & 1 for i in range(self.n)], np.uint8)

    def parity(self, msg_int):
        """the p-bit remainder of m(x) x^p mod g"""
        return poly_mod(msg_int << self.p, self.g)

    def syndromes(self, v):
        """[S_1 .. S_2t] of the polynomial v: S_j = v(alpha^j)"""
        out = []
        for j in range(1, 2 * self.t + 1):
            s, b, w = 0, 0, v
            while w:
                if w & 1:
                    s ^= self.exp[j * b % self.N0]
                w >>= 1
                b += 1
            out.append(s)
        return out

    def locate(self, rem):
        """rem = the row mod g -> the degrees d (row bit n-1-d) of the bits to flip, ascending; () for a codeword; None if no codeword
        lies within distance t.  The row and its remainder have the same syndromes: they differ by a multiple of g"""
        if rem in self._located:
            return self._located[rem]
        t, N0, n = self.t, self.N0, self.n
        S = self.syndromes(rem)
        C, B, L, shift, b = [1], [1], 0, 1, 1
        for r in range(2 * t):
            d = S[r]
            for i in range(1, L + 1):
                if i < len(C):
                    d ^= self.mul(C[i], S[r - i])
            if d == 0:
                shift += 1
                continue
            coef = self.mul(d, self.exp[N0 - self.log[b]])
            T = list(C)
            C = C + [0] * (len(B) + shift - len(C))
            for i, c in enumerate(B):
                C[i + shift] ^= self.mul(coef, c)
            if 2 * L <= r:
                L, B, b, shift = r + 1 - L, T, d, 1
            else:
                shift += 1
        while C and C[-1] == 0:
            C.pop()
        out = None
        if L <= t and len(C) - 1 == L:
            d = np.arange(n, dtype=np.int64)
            e = np.where(d > 0, N0 - d, 0)                                    # alpha^-d
            acc = np.full(n, C[0], np.int64)
            for j in range(1, L + 1):
                if C[j]:
                    acc ^= self.exp_np[self.log[C[j]] + (j * e) % N0]
            roots = np.flatnonzero(acc == 0)
            if len(roots) == L:
                out = tuple(int(x) for x in roots)
        self._located[rem] = out
        return out

    # ---- the two operations on arrays of rows
    def encode_bytes(self, rows):
        """rows [B][n] bytes: message bytes kept as they are (junk above bit 0 included), bytes k..n-1 become the parity bits, 0 or 1"""
        out = np.array(rows, np.uint8, copy=True)
        assert out.ndim == 2 and out.shape[1] == self.n
        for r in out:
            par = self.parity(self.row_int(r) >> self.p)
            r[self.k:] = [(par >> (self.p - 1 - j)) & 1 for j in range(self.p)]
        return out

    def encode_packed(self, rows):
        """packed rows: message bits kept, parity bits written, bits >= n of the last word 0 (whatever they were)"""
        assert np.asarray(rows).shape[-1] == row_bytes(self.n)
        return pack(self.encode_bytes(unpack(rows, self.n)))

    def flips(self, bits):
        """bits [B][n] (bit 0 of each) -> (mask [B][n] uint8 of the bits a decode flips, nerr [B] int32)"""
        b = np.asarray(bits, np.uint8) & 1
        assert b.ndim == 2 and b.shape[1] == self.n
        mask, nerr = np.zeros(b.shape, np.uint8), np.zeros(len(b), np.int32)
        for f, r in enumerate(b):
            at = self.locate(poly_mod(self.row_int(r), self.g))
            if at is None:
                nerr[f] = -1
            else:
                nerr[f] = len(at)
                mask[f, [self.n - 1 - d for d in at]] = 1
        return mask, nerr

    def decode_bytes(self, rows):
        """rows [B][n] bytes -> (rows with bit 0 of the corrected bytes flipped, nerr)"""
        mask, nerr = self.flips(rows)
        return np.asarray(rows, np.uint8) ^ mask, nerr

    def decode_packed(self, rows):
        """packed rows -> (rows with the corrected bits flipped and every other bit, pad bits included, as it was, nerr)"""
        rows = np.asarray(rows, np.uint8)
        assert rows.shape[-1] == row_bytes(self.n)
        mask, nerr = self.flips(unpack(rows, self.n))
        return rows ^ pack(mask), nerr

    def is_codeword(self, bits):
        return poly_mod(self.row_int(bits), self.g) == 0
