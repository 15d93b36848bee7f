// Stand-alone driver of the host side of the BCH outer code (ecc_ldpc_amd/csrc/bch.cc), host code only: the way to run the field and
// generator construction, the table of the linear form and the serial encode / decode under a sanitizer without loading them into
// another process.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/bch_host_main.cc ecc_ldpc_amd/csrc/bch.cc -o bch_host_main
//   ./bch_host_main
// On each shape of tests/test_bch_spec.py SHAPES (and the full-length row of tests/test_bch_gpu.py) it builds the code, encodes random
// messages, checks the row against the table of the linear form, flips e = 0 .. t + 2 bits and decodes: for e <= t the row must come
// back as sent with nerr = e; above t a row is either left as it was (nerr = -1) or has become another codeword at distance nerr <= t.
// The refusals of BchCode::init run too.  Exit status 0 if all of it holds.
#include <stdio.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../ecc_ldpc_amd/csrc/bch.h"

static bool is_codeword(const ldpc::BchCode &c, const std::vector<uint32_t> &planes, int W, const std::vector<uint8_t> &row) {
    const size_t n4 = ((size_t)c.n + 3) / 4 * 4;
    for (int w = 0; w < W; w++) {
        uint32_t acc = 0;
        for (int i = 0; i < c.n; i++)
            if (row[i] & 1u) acc ^= planes[(size_t)w * n4 + i];
        if (acc) return false;
    }
    return true;
}

int main() {
    static const struct { uint32_t poly; int m, t, n; } shapes[] = {{0xB, 3, 1, 7}, {0x13, 4, 3, 13}, {0x11D, 8, 4, 100}, {0x11D, 8, 16, 255}, {0x402B, 14, 12, 601},
                                                                    {0x1002D, 16, 12, 700}, {0x1002D, 16, 16, 300}, {0x1002D, 16, 12, 32400}};
    std::mt19937 rng(2024);
    int bad = 0;
    for (const auto &s : shapes) {
        ldpc::BchCode c;
        std::string err;
        if (c.init("bch_host_main", s.m, s.poly, s.t, s.n, err) != 0) { printf("m %d t %d n %d: %s\n", s.m, s.t, s.n, err.c_str()); bad++; continue; }
        const int W = (c.p + 31) / 32;
        std::vector<uint32_t> planes;
        c.table(W, planes);
        int fails = 0, corrected = 0, left = 0, moved = 0;
        for (int e = 0; e <= c.t + 2; e++) {
            std::vector<uint8_t> row(c.n);
            for (auto &b : row) b = (uint8_t)(rng() & 0xFF);                 // junk above bit 0; the parity bytes are overwritten
            c.encode(row.data());
            if (!is_codeword(c, planes, W, row)) fails++;
            const std::vector<uint8_t> sent = row;
            std::vector<int> at(c.n);
            for (int i = 0; i < c.n; i++) at[i] = i;
            std::shuffle(at.begin(), at.end(), rng);
            if (e >= 1) std::swap(at[0], *std::find(at.begin(), at.end(), 0));             // the two ends of the row among the positions
            if (e >= 2) std::swap(at[1], *std::find(at.begin(), at.end(), c.n - 1));
            for (int i = 0; i < e; i++) row[at[i]] ^= 1u;
            const std::vector<uint8_t> got = row;
            const int nerr = c.decode(row.data());
            if (e <= c.t) {
                if (nerr != e || row != sent) fails++;
                corrected++;
            } else if (nerr < 0) {
                if (row != got) fails++;
                left++;
            } else {
                int dist = 0;
                for (int i = 0; i < c.n; i++) dist += (row[i] ^ got[i]) & 1u;
                if (dist != nerr || nerr > c.t || !is_codeword(c, planes, W, row)) fails++;
                moved++;
            }
        }
        printf("m %2d t %2d n %5d: p %3d k %5d  corrected %d, left %d, moved to another codeword %d, failures %d\n", c.m, c.t, c.n, c.p, c.k, corrected, left, moved, fails);
        bad += fails;
    }
    static const struct { int m; uint32_t poly; int t, n; } refused[] = {{2, 0x7, 1, 3}, {17, 0x20009, 1, 100}, {4, 0x13, 0, 15}, {16, 0x1002D, 17, 1000}, {4, 0x1F, 1, 15},
                                                                        {4, 0x12, 1, 15}, {8, 0x11B, 2, 255}, {3, 0xB, 4, 7}, {4, 0x13, 3, 10}, {4, 0x13, 2, 16}, {4, 0x13, 3, -1}};
    for (const auto &r : refused) {
        ldpc::BchCode c;
        std::string err;
        if (c.init("bch_host_main", r.m, r.poly, r.t, r.n, err) == 0 || err.empty()) { printf("m %d poly 0x%x t %d n %d was accepted\n", r.m, r.poly, r.t, r.n); bad++; }
    }
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
