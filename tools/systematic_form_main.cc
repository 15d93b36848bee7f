// Stand-alone driver of the GF(2) elimination behind ldpc_csr_systematic_form (ecc_ldpc_amd/csrc/systematic.cc), host code only:
// the way to run that elimination under a sanitizer without loading it into another process.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/systematic_form_main.cc
//       ecc_ldpc_amd/csrc/systematic.cc -o systematic_form_main
//   ./systematic_form_main H.csr [...]
// H.csr is text: "M N", then per row its number of columns followed by the columns, ascending.  For each file it prints K, rank and
// the first parity positions, and checks on its own that the codeword of every unit message satisfies every row of H.
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../ecc_ldpc_amd/csrc/systematic.h"

int main(int argc, char **argv) {
    int bad = 0;
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "r");
        int M = 0, N = 0;
        if (!f || fscanf(f, "%d %d", &M, &N) != 2 || M <= 0 || N <= 0) { fprintf(stderr, "%s: cannot read M N\n", argv[a]); return 2; }
        std::vector<int32_t> rp(1, 0), ci;
        for (int m = 0; m < M; m++) {
            int d = 0;
            if (fscanf(f, "%d", &d) != 1 || d < 0) { fprintf(stderr, "%s: row %d\n", argv[a], m); return 2; }
            for (int e = 0; e < d; e++) {
                int c = 0;
                if (fscanf(f, "%d", &c) != 1) { fprintf(stderr, "%s: row %d\n", argv[a], m); return 2; }
                ci.push_back(c);
            }
            rp.push_back((int32_t)ci.size());
        }
        fclose(f);
        ldpc::SystematicForm sf;
        std::string err;
        const int rc = ldpc::systematic_form("systematic_form", M, N, rp.data(), ci.data(), sf, err);
        if (rc != 0) { printf("%s: %d %s\n", argv[a], rc, err.c_str()); continue; }
        printf("%s: M %d N %d K %d rank %d par_pos", argv[a], M, N, sf.K, sf.rank);
        for (int j = 0; j < sf.rank && j < 10; j++) printf(" %d", sf.par_pos[j]);
        long ones = 0, fails = 0;
        std::vector<uint8_t> c((size_t)N);
        for (int i = 0; i < sf.K; i++) {
            std::fill(c.begin(), c.end(), 0);
            c[sf.msg_pos[i]] = 1;
            for (int j = 0; j < sf.rank; j++) {
                c[sf.par_pos[j]] = (uint8_t)((sf.P[(size_t)i * sf.pw64 + (j >> 6)] >> (j & 63)) & 1ull);
                ones += c[sf.par_pos[j]];
            }
            for (int m = 0; m < M; m++) {
                unsigned s = 0;
                for (int e = rp[m]; e < rp[m + 1]; e++) s ^= c[ci[e]];
                fails += s;
            }
        }
        printf(" ... density of P %.3f, failed checks %ld\n", (double)ones / ((double)sf.K * sf.rank), fails);
        bad += fails != 0;
    }
    return bad ? 1 : 0;
}
