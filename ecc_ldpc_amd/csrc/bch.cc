// bch.cc -- the host side of the BCH outer code (include/ldpc_hip.h ldpc_bch, csrc/bch.h): the field's log / antilog tables, the
// generator polynomial, the table of the linear form, and the serial rule -- LFSR division, syndromes, Berlekamp-Massey, Chien search.
// Nothing here touches a device (ldpc_bch_create_on, which copies the tables there, is in api.cc).  Restated in tests/bch_spec.py.
#include "bch.h"

#include <stdio.h>

namespace ldpc {

static int bch_refuse(std::string &err, const char *fmt, const char *what, long a, long b) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, what, a, b);
    err = buf;
    return -1;
}

int BchCode::init(const char *what, int m_, uint32_t prim, int t_, int n_, std::string &err) {
    if (m_ < 3 || m_ > kBchMaxM) return bch_refuse(err, "%s: m = %ld outside 3..%ld", what, m_, kBchMaxM);
    if (t_ < 1 || t_ > kBchMaxT) return bch_refuse(err, "%s: t = %ld outside 1..%ld", what, t_, kBchMaxT);
    if ((prim >> m_) != 1u) return bch_refuse(err, "%s: prim_poly = 0x%lx is not of degree m = %ld (the x^m term is part of it)", what, (long)prim, m_);
    m = m_; t = t_; n = n_; prim_poly = prim; N0 = (1 << m) - 1;
    alog.assign((size_t)2 * N0, 0);
    log.assign((size_t)N0 + 1, 0);
    uint32_t a = 1u;
    for (int i = 0; i < N0; i++) {
        if (i > 0 && a == 1u) return bch_refuse(err, "%s: prim_poly = 0x%lx is not primitive: x has order %ld", what, (long)prim, i);
        alog[i] = alog[(size_t)i + N0] = (uint16_t)a;
        log[a] = (uint16_t)i;
        a <<= 1;
        if (a >> m) a ^= prim;
    }
    if (a != 1u) return bch_refuse(err, "%s: prim_poly = 0x%lx is not primitive: x has no order dividing %ld", what, (long)prim, N0);
    if (2 * t >= N0) return bch_refuse(err, "%s: t = %ld: 2t must be below 2^m - 1 = %ld", what, t, N0);
    // g = the product of the minimal polynomials of the cyclotomic cosets that meet 1 .. 2t
    std::vector<uint8_t> covered((size_t)N0, 0);
    g.assign(1, 1);
    for (int j = 1; j <= 2 * t; j++) {
        if (covered[j]) continue;
        std::vector<uint32_t> mp(1, 1u);   // the product of (x + alpha^e) over the coset of j, coefficients in GF(2^m)
        int e = j;
        do {
            covered[e] = 1;
            const uint32_t root = alog[e];
            mp.push_back(0u);
            for (size_t d = mp.size() - 1; d >= 1; d--) mp[d] = mp[d - 1] ^ mul(mp[d], root);
            mp[0] = mul(mp[0], root);
            e = (int)(((long)e * 2) % N0);
        } while (e != j);
        std::vector<uint8_t> prod(g.size() + mp.size() - 1, 0);   // a minimal polynomial has coefficients 0 and 1
        for (size_t x = 0; x < g.size(); x++)
            if (g[x])
                for (size_t y = 0; y < mp.size(); y++) prod[x + y] ^= (uint8_t)(mp[y] & 1u);
        g.swap(prod);
    }
    p = (int)g.size() - 1;
    if (n <= p || n > N0) return bch_refuse(err, "%s: n = %ld outside p + 1 .. 2^m - 1 (p = deg g = %ld)", what, n, p);
    k = n - p;
    glow = BchRem();
    for (int b = 0; b < p; b++)
        if (g[b]) glow.w[b >> 5] |= 1u << (b & 31);
    return 0;
}

void BchCode::step(BchRem &r, uint32_t b) const {
    const uint32_t top = (r.w[(p - 1) >> 5] >> ((p - 1) & 31)) & 1u;
    for (int w = kBchMaxWords - 1; w >= 1; w--) r.w[w] = (r.w[w] << 1) | (r.w[w - 1] >> 31);
    r.w[0] <<= 1;
    if (p < 32 * kBchMaxWords) r.w[p >> 5] &= ~(1u << (p & 31));
    if (top ^ (b & 1u))
        for (int w = 0; w < kBchMaxWords; w++) r.w[w] ^= glow.w[w];
}

void BchCode::encode(uint8_t *row) const {
    BchRem r;
    for (int i = 0; i < k; i++) step(r, row[i]);
    for (int j = 0; j < p; j++) row[k + j] = (uint8_t)r.bit(p - 1 - j);
}

int BchCode::decode(uint8_t *row) const {
    BchRem r;
    for (int i = 0; i < k; i++) step(r, row[i]);
    for (int j = 0; j < p; j++)
        if (row[k + j] & 1u) r.w[(p - 1 - j) >> 5] ^= 1u << ((p - 1 - j) & 31);
    if (r.zero()) return 0;
    // S[j - 1] = R(alpha^j): the row and its remainder agree at every root of g
    uint32_t S[2 * kBchMaxT];
    for (int j = 1; j <= 2 * t; j++) {
        uint32_t s = 0;
        for (int b = 0; b < p; b++)
            if (r.bit(b)) s ^= alog[(size_t)(((long)j * b) % N0)];
        S[j - 1] = s;
    }
    // Berlekamp-Massey: the shortest LFSR C of length L that generates S
    constexpr int kLen = 2 * kBchMaxT + 2;
    uint32_t C[kLen] = {1u}, B[kLen] = {1u}, T[kLen];
    int L = 0, shift = 1;
    uint32_t bd = 1u;
    for (int s = 0; s < 2 * t; s++) {
        uint32_t d = S[s];
        for (int i = 1; i <= L; i++) d ^= mul(C[i], S[s - i]);
        if (!d) { shift++; continue; }
        const uint32_t coef = mul(d, alog[(size_t)N0 - log[bd]]);
        for (int i = 0; i < kLen; i++) T[i] = C[i];
        for (int i = 0; i + shift < kLen; i++) C[i + shift] ^= mul(coef, B[i]);
        if (2 * L <= s) {
            L = s + 1 - L;
            for (int i = 0; i < kLen; i++) B[i] = T[i];
            bd = d;
            shift = 1;
        } else {
            shift++;
        }
    }
    if (L > t) return -1;
    int deg = 0;
    for (int i = 0; i < kLen; i++)
        if (C[i]) deg = i;
    if (deg != L) return -1;
    // Chien: the bit of x^d is in error iff C(alpha^-d) = 0; exactly L such d below n, or the row stays as it was
    int roots[kBchMaxT], count = 0;
    for (int d = 0; d < n; d++) {
        const int e = d ? N0 - d : 0;
        uint32_t acc = C[0];
        int ej = 0;
        for (int j = 1; j <= L; j++) {
            ej += e;
            if (ej >= N0) ej -= N0;
            if (C[j]) acc ^= alog[(size_t)log[C[j]] + ej];
        }
        if (!acc) {
            if (count == L) return -1;
            roots[count++] = d;
        }
    }
    if (count != L) return -1;
    for (int i = 0; i < L; i++) row[n - 1 - roots[i]] ^= 1u;
    return L;
}

void BchCode::table(int W, std::vector<uint32_t> &planes) const {
    const size_t n4 = ((size_t)n + 3) / 4 * 4;
    planes.assign((size_t)W * n4, 0u);
    BchRem r;
    r.w[0] = 1u;   // p >= 3: x^0 is its own remainder
    for (int d = 0; d < n; d++) {
        for (int w = 0; w < W && w < kBchMaxWords; w++) planes[(size_t)w * n4 + (size_t)(n - 1 - d)] = r.w[w];
        step(r, 0u);
    }
}

}  // namespace ldpc

#ifdef __HIPCC__
using ldpc::set_error;

extern "C" {

int ldpc_bch_builtin(int kind, int *m, uint32_t *prim_poly, int *t) {
    static const struct { int m; uint32_t prim; int t; } k[] = {{16, 0x1002Du, 8}, {16, 0x1002Du, 10}, {16, 0x1002Du, 12}, {14, 0x402Bu, 12}};
    if (kind < LDPC_BCH_M16_T8 || kind > LDPC_BCH_M14_T12) return set_error(LDPC_EINVAL, "ldpc_bch_builtin: unknown kind %d", kind);
    if (m) *m = k[kind].m;
    if (prim_poly) *prim_poly = k[kind].prim;
    if (t) *t = k[kind].t;
    return LDPC_OK;
}

int ldpc_bch_params(const ldpc_bch *bch, int *m, uint32_t *prim_poly, int *t, int *n, int *k) {
    if (!bch) return set_error(LDPC_EINVAL, "ldpc_bch_params: null bch");
    if (m) *m = bch->code.m;
    if (prim_poly) *prim_poly = bch->code.prim_poly;
    if (t) *t = bch->code.t;
    if (n) *n = bch->code.n;
    if (k) *k = bch->code.k;
    return LDPC_OK;
}

int ldpc_bch_generator(const ldpc_bch *bch, uint8_t *g) {
    if (!bch) return set_error(LDPC_EINVAL, "ldpc_bch_generator: null bch");
    if (g)
        for (int j = 0; j <= bch->code.p; j++) g[j] = bch->code.g[j];
    return bch->code.p;
}

int ldpc_bch_encode_host(const ldpc_bch *bch, uint8_t *row) {
    if (!bch || !row) return set_error(LDPC_EINVAL, "ldpc_bch_encode_host: null %s", bch ? "row" : "bch");
    bch->code.encode(row);
    return LDPC_OK;
}

int ldpc_bch_decode_host(const ldpc_bch *bch, uint8_t *row, int *nerr) {
    if (!bch || !row || !nerr) return set_error(LDPC_EINVAL, "ldpc_bch_decode_host: null %s", !bch ? "bch" : !row ? "row" : "nerr");
    *nerr = bch->code.decode(row);
    return LDPC_OK;
}

}  // extern "C"
#endif
