// crc.h -- the CRC of include/ldpc_hip.h (ldpc_crc): a bit-serial, unreflected CRC of width w over the first L bits of a message of
// k = L + w bits, its w bits appended MSB first.  The rule (crc.cc crc_serial; restated in tests/crc_spec.py):
//   r = init;  for payload bit b_i, i = 0 .. L - 1:  top = (r >> (w - 1)) & 1;  r = (r << 1) & mask;  if (top ^ b_i) r ^= poly;
//   crc = r ^ xorout;  message bit L + j = (crc >> (w - 1 - j)) & 1.
// The kernels (crc.hip) use the LINEAR FORM  crc = C0 ^ XOR_{i : b_i = 1} T[i]:  T[i] = the register after the unit vector e_i with
// init = xorout = 0, C0 = the CRC of L zero bits.  The device table is T EXTENDED over the CRC bits, ext[L + j] = 1 << (w - 1 - j), so
// that the XOR over ALL set bits of a message is crc(payload) ^ (the w received bits as a number): a message passes iff that XOR is C0.
// Host side: crc.cc; the object is created in api.cc (ldpc_crc_create_on).
#pragma once
#include "internal.h"

namespace ldpc {

// the table as a kernel argument
struct CrcTab {
    const uint32_t *ext;   // [k rounded up to 4]: T[0 .. L - 1], then 1 << (w - 1 - j) for bit L + j, then zeros; 16-byte aligned
    int L, w, k;
    uint32_t c0;           // the CRC of L zero bits (init and xorout inside)
};

constexpr int kCrcMaxBits = 1 << 24;             // k = n_bits + width may be no larger
constexpr size_t kCrcMaxItems = 0xffffff00ull;   // batch * k of one call: 2^32 - 256

// LDPC_OK, or LDPC_EINVAL: width outside 1..32, an even poly, poly / init / xorout at or above 2^width, n_bits < 1, n_bits + width > 2^24
int crc_check_params(const char *what, int width, uint32_t poly, uint32_t init, uint32_t xorout, int n_bits);
// the rule, bit 0 of each byte
uint32_t crc_serial(int width, uint32_t poly, uint32_t init, uint32_t xorout, int n_bits, const uint8_t *bits);
// T [n_bits] of the linear form
void crc_table(int width, uint32_t poly, int n_bits, uint32_t *table);

// ldpc_crc_attach_dev: rows of k bytes (packed: 4 * ceil(k / 32) bytes), in place
int crc_attach_launch(hipStream_t st, const CrcTab &t, int batch, void *d_msg, bool packed);
// ldpc_crc_check_dev, ldpc_sim_crc_check: message bit i of frame f = bit 0 of src[f * stride + p], or (packed) bit p % 8 of
// src[f * stride + p / 8], p = pos ? pos[i] : i; stride in bytes
int crc_check_launch(hipStream_t st, const CrcTab &t, int batch, const uint8_t *src, size_t stride, bool packed, const int32_t *pos, uint8_t *d_ok);
// ldpc_sim_tally_crc: tally[0..3] += {frames, ok, frames with a message-bit error, ok and in error}; the message-bit comparison is
// sim_tally_kernel's (decoded byte msg_pos[i], or i, against bit i of msgw)
int crc_tally_launch(hipStream_t st, const int32_t *msg_pos, int N, int k, int kwords, const uint32_t *msgw, int batch, const uint8_t *d_bits, const uint8_t *d_ok,
                     unsigned long long *d_tally);

}  // namespace ldpc

// (host) the object behind include/ldpc_hip.h ldpc_crc
struct ldpc_crc {
    int width = 0, n_bits = 0, device = -1;
    uint32_t poly = 0, init = 0, xorout = 0;
    uint32_t *d_ext = nullptr;
    ldpc::CrcTab tab{};
};
