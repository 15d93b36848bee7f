// bch.h -- the BCH outer code of include/ldpc_hip.h (ldpc_bch): a binary, narrow-sense, primitive BCH code over GF(2^m), m = 3 .. 16,
// correcting t = 1 .. 16 errors, shortened to n bits.  The rule (bch.cc; restated in tests/bch_spec.py):
//   FIELD      GF(2^m) from prim_poly (its x^m term included), alpha = x, N0 = 2^m - 1; x must have order N0.
//   GENERATOR  g = the product of the distinct minimal polynomials of alpha^1 .. alpha^(2t); p = deg g <= m t <= 256; p < n <= N0; 2t < N0.
//   ROW        bit i, i = 0 .. n - 1, is the coefficient of x^(n - 1 - i): k = n - p message bits, then the remainder of m(x) x^p mod g,
//              MSB first -- the CRC's order (crc.h).
//   DECODE     the codeword within Hamming distance t of the row if there is one (it is unique), else the row as it was.
// The kernels (bch.hip) use the LINEAR FORM of the remainder, R = XOR over the set bits i of T[i], T[i] = x^(n - 1 - i) mod g, a number of
// p bits (bit b = the coefficient of x^b) in W = ceil(p / 32) words.  Over the parity positions T is a unit vector, so R over the k message
// bits is the parity and R over all n bits is the row mod g: zero iff the row is a codeword.
// The part above `#ifdef __HIPCC__` is plain C++ with no device in it: tools/bch_host_main.cc builds it alone.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace ldpc {

constexpr int kBchMaxM = 16, kBchMaxT = 16, kBchMaxWords = 8;   // p <= 256 bits

// the remainder register: p <= 256 bits, bit b = the coefficient of x^b
struct BchRem {
    uint32_t w[kBchMaxWords] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool bit(int b) const { return (w[b >> 5] >> (b & 31)) & 1u; }
    bool zero() const { return !(w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]); }
};

struct BchCode {
    int m = 0, t = 0, n = 0, k = 0, p = 0, N0 = 0;
    uint32_t prim_poly = 0;
    std::vector<uint16_t> alog;   // [2 N0]: alpha^i, doubled so that the sum of two logs needs no modulo
    std::vector<uint16_t> log;    // [N0 + 1]: log[alpha^i] = i; log[0] is not used
    std::vector<uint8_t> g;       // [p + 1]: g[j] = the coefficient of x^j
    BchRem glow;                  // g without its x^p term

    // builds the field and the generator.  0, or -1 with `err` naming the argument: m, t or n out of range, a prim_poly under which x
    // does not have order N0, 2t >= N0, n <= p
    int init(const char *what, int m, uint32_t prim_poly, int t, int n, std::string &err);
    uint32_t mul(uint32_t a, uint32_t b) const { return a && b ? alog[(size_t)log[a] + log[b]] : 0u; }
    // one step of the division register with input bit b: r <- r x + b x^p mod g
    void step(BchRem &r, uint32_t b) const;
    // the serial rule on one row of n bytes (bit 0 of each read), in place
    void encode(uint8_t *row) const;
    int decode(uint8_t *row) const;   // -> the number of bits corrected, or -1 with the row untouched
    // T of the linear form as the kernels read it: W planes of n4 = n rounded up to 4 words, plane w holding word w of every T[i]
    void table(int W, std::vector<uint32_t> &planes) const;
};

}  // namespace ldpc

#ifdef __HIPCC__
#include "internal.h"

namespace ldpc {

// the tables as a kernel argument
struct BchTab {
    const uint32_t *T;       // [W][n4]: plane w = word w of T[0 .. n - 1], zeros behind; 16-byte aligned planes
    const uint16_t *alog;    // [2 N0]
    const uint16_t *log;     // [N0 + 1]
    int n, k, p, n4, m, t, N0;
    uint32_t prim_poly;
};

constexpr size_t kBchMaxItems = 0xffffff00ull;   // batch * n of one call: 2^32 - 256, the CRC's limit

// ldpc_bch_encode_dev: rows of n bytes (packed: 4 * ceil(n / 32) bytes), in place
int bch_encode_launch(hipStream_t st, const BchTab &t, int W, int batch, void *d_rows, bool packed);
// ldpc_bch_decode_dev, ldpc_sim_bch_decode: row bit i of frame f = bit 0 of rows[f * stride + q], or (packed) bit q % 8 of
// rows[f * stride + q / 8], q = pos ? pos[i] : i; stride in bytes.  Corrected in place; nerr[f] = bits corrected, or -1
int bch_decode_launch(hipStream_t st, const BchTab &t, int W, int batch, uint8_t *rows, size_t stride, bool packed, const int32_t *pos, int32_t *d_nerr);

}  // namespace ldpc

// (host) the object behind include/ldpc_hip.h ldpc_bch
struct ldpc_bch {
    ldpc::BchCode code;
    int device = -1, W = 0;   // device -1: a host-only object; W: the words of a table entry the kernels are instantiated for (1, 2, 4, 6, 8)
    uint32_t *d_T = nullptr;
    uint16_t *d_alog = nullptr, *d_log = nullptr;
    ldpc::BchTab tab{};
};
#endif
