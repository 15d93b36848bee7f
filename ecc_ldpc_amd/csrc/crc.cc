// crc.cc -- the host side of the CRC (include/ldpc_hip.h ldpc_crc, csrc/crc.h): the parameter checks, the bit-serial rule, the table
// of its linear form and the built-in parameter sets.  Nothing here touches a device (ldpc_crc_create_on, which copies the table
// there, is in api.cc).  Restated in tests/crc_spec.py.
#include "crc.h"

using ldpc::set_error;

namespace ldpc {

static inline uint32_t crc_mask(int w) { return w == 32 ? 0xffffffffu : (1u << w) - 1u; }

// one step of the register with input bit b
static inline uint32_t crc_step(uint32_t r, uint32_t b, int w, uint32_t poly, uint32_t mask) {
    const uint32_t top = (r >> (w - 1)) & 1u;
    r = (r << 1) & mask;
    return (top ^ b) ? r ^ poly : r;
}

int crc_check_params(const char *what, int width, uint32_t poly, uint32_t init, uint32_t xorout, int n_bits) {
    if (width < 1 || width > 32) return set_error(LDPC_EINVAL, "%s: width = %d outside 1..32", what, width);
    if (!(poly & 1u)) return set_error(LDPC_EINVAL, "%s: poly = 0x%x is even (the generator needs its x^0 term)", what, poly);
    const uint32_t mask = crc_mask(width);
    if ((poly & ~mask) || (init & ~mask) || (xorout & ~mask))
        return set_error(LDPC_EINVAL, "%s: poly = 0x%x, init = 0x%x, xorout = 0x%x: all must be below 2^%d", what, poly, init, xorout, width);
    if (n_bits < 1) return set_error(LDPC_EINVAL, "%s: n_bits = %d (must be >= 1)", what, n_bits);
    if (n_bits > kCrcMaxBits - width) return set_error(LDPC_EINVAL, "%s: n_bits + width = %d + %d is more than 2^24", what, n_bits, width);
    return LDPC_OK;
}

uint32_t crc_serial(int width, uint32_t poly, uint32_t init, uint32_t xorout, int n_bits, const uint8_t *bits) {
    const uint32_t mask = crc_mask(width);
    uint32_t r = init;
    for (int i = 0; i < n_bits; i++) r = crc_step(r, bits ? bits[i] & 1u : 0u, width, poly, mask);
    return r ^ xorout;
}

// T[i] = the register after e_i = a one, then n_bits - 1 - i zeros, from register 0: T[n_bits - 1] = poly, T[i] = one zero step of T[i + 1]
void crc_table(int width, uint32_t poly, int n_bits, uint32_t *table) {
    const uint32_t mask = crc_mask(width);
    uint32_t r = poly;
    for (int i = n_bits - 1; i >= 0; i--) {
        table[i] = r;
        r = crc_step(r, 0u, width, poly, mask);
    }
}

}  // namespace ldpc

extern "C" {

int ldpc_crc_builtin(int kind, int *width, uint32_t *poly, uint32_t *init, uint32_t *xorout) {
    static const struct { int w; uint32_t poly, init, xorout; } k[] = {
        {6, 0x21u, 0u, 0u}, {11, 0x621u, 0u, 0u}, {16, 0x1021u, 0u, 0u}, {24, 0x864CFBu, 0u, 0u}, {24, 0x800063u, 0u, 0u}, {24, 0xB2B117u, 0u, 0u},
        {32, 0x04C11DB7u, 0xFFFFFFFFu, 0xFFFFFFFFu}};
    if (kind < LDPC_CRC_6 || kind > LDPC_CRC_32) return set_error(LDPC_EINVAL, "ldpc_crc_builtin: unknown kind %d", kind);
    if (width) *width = k[kind].w;
    if (poly) *poly = k[kind].poly;
    if (init) *init = k[kind].init;
    if (xorout) *xorout = k[kind].xorout;
    return LDPC_OK;
}

int ldpc_crc_bits_host(int width, uint32_t poly, uint32_t init, uint32_t xorout, int n_bits, const uint8_t *bits, uint32_t *crc) {
    const int rc = ldpc::crc_check_params("ldpc_crc_bits_host", width, poly, init, xorout, n_bits);
    if (rc != LDPC_OK) return rc;
    if (!bits || !crc) return set_error(LDPC_EINVAL, "ldpc_crc_bits_host: null argument");
    *crc = ldpc::crc_serial(width, poly, init, xorout, n_bits, bits);
    return LDPC_OK;
}

int ldpc_crc_table(int width, uint32_t poly, int n_bits, uint32_t *table) {
    const int rc = ldpc::crc_check_params("ldpc_crc_table", width, poly, 0u, 0u, n_bits);
    if (rc != LDPC_OK) return rc;
    if (!table) return set_error(LDPC_EINVAL, "ldpc_crc_table: null output");
    ldpc::crc_table(width, poly, n_bits, table);
    return LDPC_OK;
}

int ldpc_crc_params(const ldpc_crc *crc, int *width, uint32_t *poly, uint32_t *init, uint32_t *xorout, int *n_bits) {
    if (!crc) return set_error(LDPC_EINVAL, "null crc");
    if (width) *width = crc->width;
    if (poly) *poly = crc->poly;
    if (init) *init = crc->init;
    if (xorout) *xorout = crc->xorout;
    if (n_bits) *n_bits = crc->n_bits;
    return LDPC_OK;
}

}  // extern "C"
