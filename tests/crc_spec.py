"""The CRC rule of include/ldpc_hip.h (ldpc_crc; csrc/crc.cc, csrc/crc.hip), restated in numpy: the bit-serial register, vectorised over
frames and serial over bits.  All integer arithmetic, so everything that compares against this compares with equality.

  width w in 1..32; poly = the generator without its x^w term (odd, below 2^w); init, xorout below 2^w; payload length L >= 1; k = L + w.
  r = init; for payload bit b_i, i = 0 .. L-1 (message order):  top = (r >> (w-1)) & 1;  r = (r << 1) & mask;  if top ^ b_i: r ^= poly
  crc = r ^ xorout;  message bit L + j = (crc >> (w-1-j)) & 1, j = 0 .. w-1 (MSB first).  No reflection, no byte notion.
  packed rows: bit i in byte i/8 at bit i%8, 4 * ceil(k/32) bytes a row, bits >= k zero.
  linear form: crc = C0 ^ XOR over the set bits i of T[i]; T[i] = the register after the unit vector e_i with init = xorout = 0;
  C0 = the CRC of L zero bits."""
import numpy as np

# kind (the integer of LDPC_CRC_*) -> (name, w, poly, init, xorout, check): check = the CRC of the 72 bits of ASCII "123456789", the MSB
# of each byte first.  Defined by formula; no claim that they are any standard's
BUILTINS = {
    0: ("crc6", 6, 0x21, 0, 0, 0x15),
    1: ("crc11", 11, 0x621, 0, 0, 0x5CA),
    2: ("crc16", 16, 0x1021, 0, 0, 0x31C3),
    3: ("crc24a", 24, 0x864CFB, 0, 0, 0xCDE703),
    4: ("crc24b", 24, 0x800063, 0, 0, 0x23EF52),
    5: ("crc24c", 24, 0xB2B117, 0, 0, 0xF48279),
    6: ("crc32", 32, 0x04C11DB7, 0xFFFFFFFF, 0xFFFFFFFF, 0xFC891918),
}
KIND = {v[0]: k for k, v in BUILTINS.items()}


def builtin(name):
    """-> (w, poly, init, xorout)"""
    return BUILTINS[KIND[name]][1:5]


def check_string_bits():
    """the 72 bits of b"123456789", the MSB of each byte first"""
    return np.unpackbits(np.frombuffer(b"123456789", np.uint8), bitorder="big")


def _mask(w):
    return (1 << w) - 1


def crc_bits(bits, w, poly, init=0, xorout=0):
    """bits [..., L] (bit 0 of each element is read) -> the CRC of every row, uint32 [...]"""
    b = (np.asarray(bits).astype(np.uint64)) & np.uint64(1)
    r = np.full(b.shape[:-1], init, np.uint64)
    mask, p, s = np.uint64(_mask(w)), np.uint64(poly), np.uint64(w - 1)
    for i in range(b.shape[-1]):
        top = (r >> s) & np.uint64(1)
        r = (r << np.uint64(1)) & mask
        r = np.where((top ^ b[..., i]) != 0, r ^ p, r)
    return (r ^ np.uint64(xorout)).astype(np.uint32)


def table(w, poly, L):
    """T [L] uint32 of the linear form, each entry by the rule itself: the register after e_i, init = xorout = 0"""
    return crc_bits(np.eye(L, dtype=np.uint8), w, poly, 0, 0)


def c0(w, poly, init, xorout, L):
    return int(crc_bits(np.zeros(L, np.uint8), w, poly, init, xorout))


def crc_linear(bits, w, poly, init, xorout):
    """the linear form on bits [..., L] -> uint32 [...]"""
    b = np.asarray(bits) & 1
    L = b.shape[-1]
    T = table(w, poly, L)
    acc = np.bitwise_xor.reduce(np.where(b != 0, T, np.uint32(0)).astype(np.uint32), axis=-1)
    return acc ^ np.uint32(c0(w, poly, init, xorout, L))


def crc_field(crc, w):
    """crc uint32 [...] -> its w bits, MSB first, uint8 [..., w]"""
    sh = np.arange(w - 1, -1, -1, dtype=np.uint32)
    return ((np.asarray(crc, np.uint32)[..., None] >> sh) & np.uint32(1)).astype(np.uint8)


def attach_bytes(msg, L, w, poly, init=0, xorout=0):
    """msg [B][k] bytes: the payload bytes are kept as they are (junk above bit 0 included), bytes L .. k-1 become the CRC bits, 0 or 1"""
    out = np.array(msg, np.uint8, copy=True)
    assert out.shape[-1] == L + w
    out[..., L:] = crc_field(crc_bits(out[..., :L], w, poly, init, xorout), w)
    return out


def check_bytes(msg, L, w, poly, init=0, xorout=0):
    """msg [B][k] bytes (bit 0 of each) -> uint8 [B]: 1 where the trailing w bits are the CRC of the first L"""
    m = np.asarray(msg, np.uint8) & 1
    assert m.shape[-1] == L + w
    return (m[..., L:] == crc_field(crc_bits(m[..., :L], w, poly, init, xorout), w)).all(-1).astype(np.uint8)


def row_bytes(k):
    return 4 * ((k + 31) // 32)


def pack(bits):
    """bits [B][k] (bit 0 of each) -> packed rows [B][4 * ceil(k/32)] uint8, bit i in byte i/8 at bit i%8, pad bits 0"""
    b = (np.asarray(bits, np.uint8) & 1)
    k = b.shape[-1]
    pad = np.zeros(b.shape[:-1] + (8 * row_bytes(k) - k,), np.uint8)
    return np.packbits(np.concatenate([b, pad], -1), axis=-1, bitorder="little")


def unpack(rows, k):
    """packed rows -> bits [B][k] uint8"""
    return np.unpackbits(np.asarray(rows, np.uint8), axis=-1, bitorder="little")[..., :k]


def attach_packed(rows, L, w, poly, init=0, xorout=0):
    """packed rows [B][4 * ceil(k/32)]: payload bits kept, CRC bits written, bits >= k of the last word 0 (whatever they were)"""
    k = L + w
    assert np.asarray(rows).shape[-1] == row_bytes(k)
    return pack(attach_bytes(unpack(rows, k), L, w, poly, init, xorout))


def check_packed(rows, L, w, poly, init=0, xorout=0):
    return check_bytes(unpack(rows, L + w), L, w, poly, init, xorout)


def bitrev32(x):
    x = int(x)
    return int(f"{x:032b}"[::-1], 2)
