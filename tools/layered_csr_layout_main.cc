// Stand-alone driver of the graph layout of the on-chip layered kernel for any H (ecc_ldpc_amd/csrc/layered_csr_layout.cc), host code
// only: the way to run the step builder and the packing of the column table under a sanitizer without loading them into another process.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/layered_csr_layout_main.cc ecc_ldpc_amd/csrc/layered_csr_layout.cc -o layered_csr_layout_main
//   ./layered_csr_layout_main GRAPH.txt
// GRAPH.txt holds integers separated by white space: N M L T, then the L + 1 entries of layer_ptr, the M + 1 of row_ptr and the row_ptr[M]
// of col_idx (a CSR parity-check matrix of M rows and N columns, its L layers, T threads per workgroup).  tests/test_layered_csr_layout.py
// writes such files.  Printed: one line per barrier step (its rows as the range lo..hi, its slabs, the rows of the last one), one per slab
// {offset, weight, rows} with the slab's wdeg words, and a checksum (FNV-1a, 64 bits) of cols.  The tables are then held to what
// layered_csr.hip's kernels assume of them, recomputed here from the rows:
//   every row is in exactly one step, a step is a run of consecutive rows that share no column, sorted heaviest first;
//   a slab's weight is that of its heaviest row, the slabs tile cols without a gap, and inside a slab entry [k * T + i] is column k of the
//   slab's row i where that row has one, kNoEdge everywhere else;
//   a wave's wdeg word is the largest weight of its 64 rows (lanes without a row count as 0), | 0x100 iff all 64 are equal;
//   step_ptr starts at 0, never decreases, gives step s its ceil(rows / T) slabs and ends at nslab.
// Exit status 0 if all of it holds, 1 on a violation (each is printed), 2 if the file is not a graph.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../ecc_ldpc_amd/csrc/layered_csr_layout.h"

static int bad = 0;
#define HOLD(cond, ...) do { if (!(cond)) { if (bad++ < 20) { printf("VIOLATION: " __VA_ARGS__); printf("\n"); } } } while (0)

static bool read_ints(FILE *f, std::vector<int32_t> &v, long n) {
    if (n < 0 || n > (1L << 28)) return false;
    v.resize((size_t)n);
    for (auto &x : v)
        if (fscanf(f, "%d", &x) != 1) return false;
    return true;
}

int main(int argc, char **argv) {
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) { fprintf(stderr, "usage: %s GRAPH.txt\n", argv[0]); return 2; }
    int N = 0, M = 0, L = 0, T = 0;
    std::vector<int32_t> lp, rp, ci;
    bool ok = fscanf(f, "%d %d %d %d", &N, &M, &L, &T) == 4 && N > 0 && N <= 65535 && M >= 0 && L >= 0 && T >= 64 && T % 64 == 0 && T <= 1024;
    ok = ok && read_ints(f, lp, L + 1L) && read_ints(f, rp, M + 1L) && rp[0] == 0 && lp[0] == 0 && lp[L] == M;
    for (int l = 0; ok && l < L; l++) ok = lp[l] <= lp[l + 1];
    for (int m = 0; ok && m < M; m++) ok = rp[m] <= rp[m + 1];
    ok = ok && read_ints(f, ci, rp[M]);
    for (size_t q = 0; ok && q < ci.size(); q++) ok = ci[q] >= 0 && ci[q] < N;
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: not a graph (N M L T, layer_ptr, row_ptr, col_idx)\n", argv[1]); return 2; }
    auto deg = [&](int m) { return rp[m + 1] - rp[m]; };

    const ldpc::CsrSteps steps = ldpc::csr_layout_steps(N, rp.data(), ci.data(), lp.data(), L);
    const ldpc::CsrLayout lay = ldpc::csr_layout_pack(steps, rp.data(), ci.data(), T);
    const int W = T / 64, nstep = (int)steps.rows.size();
    printf("graph N %d M %d layers %d T %d: steps %d rmax %zu nslab %d\n", N, M, L, T, nstep, steps.rmax, lay.nslab);

    // the steps
    std::vector<int> seen((size_t)M, 0);
    std::vector<int32_t> owner((size_t)N, -1);
    size_t rmax = 1;
    int next = 0;
    for (int s = 0; s < nstep; s++) {
        const auto &st = steps.rows[s];
        HOLD(!st.empty(), "step %d is empty", s);
        if (st.empty()) continue;
        const int lo = *std::min_element(st.begin(), st.end()), hi = *std::max_element(st.begin(), st.end());
        const int ns = (int)((st.size() + T - 1) / T);
        printf("step %d rows %zu lo %d hi %d slabs %d last %zu\n", s, st.size(), lo, hi, ns, st.size() - (size_t)(ns - 1) * T);
        HOLD(lo == next && hi - lo + 1 == (int)st.size(), "step %d is not the run of rows that follows step %d", s, s - 1);
        next = hi + 1;
        rmax = std::max(rmax, st.size());
        for (size_t i = 0; i < st.size(); i++) {
            const int m = st[i];
            HOLD(m >= 0 && m < M, "step %d holds row %d", s, m);
            if (m < 0 || m >= M) continue;
            seen[m]++;
            HOLD(i == 0 || deg(st[i - 1]) > deg(m) || (deg(st[i - 1]) == deg(m) && st[i - 1] < m), "step %d: row %d is out of order (heaviest first, stable)", s, m);
            for (int q = rp[m]; q < rp[m + 1]; q++) {
                HOLD(owner[ci[q]] != s, "step %d: column %d is in two of its rows", s, ci[q]);
                owner[ci[q]] = s;
            }
        }
    }
    for (int m = 0; m < M; m++) HOLD(seen[m] == 1, "row %d is in %d steps", m, seen[m]);
    HOLD(rmax == steps.rmax, "rmax %zu, the largest step has %zu rows", steps.rmax, rmax);

    // the tables
    HOLD((int)lay.step_ptr.size() == nstep + 1 && lay.step_ptr[0] == 0 && lay.step_ptr.back() == lay.nslab, "step_ptr does not run from 0 to nslab = %d", lay.nslab);
    HOLD(lay.slab.size() == 2 * (size_t)lay.nslab && lay.wdeg.size() == (size_t)lay.nslab * W, "%zu slab words and %zu wdeg words for %d slabs", lay.slab.size(), lay.wdeg.size(), lay.nslab);
    if (bad) { printf("FAILED\n"); return 1; }      // (what follows indexes by these)
    size_t at = 0;
    for (int s = 0; s < nstep; s++) {
        const auto &st = steps.rows[s];
        const int j0 = lay.step_ptr[s], j1 = lay.step_ptr[s + 1];
        HOLD(j1 >= j0 && (size_t)(j1 - j0) == (st.size() + T - 1) / T, "step %d of %zu rows has slabs %d..%d", s, st.size(), j0, j1);
        if (j1 < j0 || (size_t)(j1 - j0) != (st.size() + T - 1) / T) break;
        for (int j = j0; j < j1; j++) {
            const size_t r0 = (size_t)(j - j0) * T;
            const int nr = (int)std::min<size_t>(T, st.size() - r0), D = lay.slab[2 * j + 1];
            int dmax = 0;
            for (int i = 0; i < nr; i++) dmax = std::max(dmax, deg(st[r0 + i]));
            printf("slab %d offset %d weight %d rows %d wdeg", j, lay.slab[2 * j], D, nr);
            for (int w = 0; w < W; w++) printf(" 0x%03x", lay.wdeg[(size_t)j * W + w]);
            printf("\n");
            HOLD((size_t)lay.slab[2 * j] == at, "slab %d starts at %d, the slab before it ends at %zu", j, lay.slab[2 * j], at);
            HOLD(D == dmax, "slab %d has weight %d, its heaviest row %d", j, D, dmax);
            HOLD(at + (size_t)D * T <= lay.cols.size(), "slab %d ends past cols", j);
            if ((size_t)lay.slab[2 * j] != at || D != dmax || at + (size_t)D * T > lay.cols.size()) { at = lay.cols.size() + 1; break; }
            for (int k = 0; k < D; k++)
                for (int i = 0; i < T; i++) {
                    const bool edge = i < nr && k < deg(st[r0 + i]);
                    const int want = edge ? ci[rp[st[r0 + i]] + k] : (int)ldpc::kNoEdge;
                    HOLD(lay.cols[at + (size_t)k * T + i] == want, "slab %d edge %d thread %d: %d, not %d", j, k, i, lay.cols[at + (size_t)k * T + i], want);
                }
            for (int w = 0; w < W; w++) {
                int wd = 0, least = 1 << 30;
                for (int i = 64 * w; i < 64 * w + 64; i++) {
                    const int d = i < nr ? deg(st[r0 + i]) : 0;
                    wd = std::max(wd, d); least = std::min(least, d);
                }
                HOLD(lay.wdeg[(size_t)j * W + w] == (wd | (wd == least ? 0x100 : 0)), "slab %d wave %d: wdeg 0x%x, its rows give 0x%x", j, w, lay.wdeg[(size_t)j * W + w], wd | (wd == least ? 0x100 : 0));
            }
            at += (size_t)D * T;
        }
    }
    HOLD(at == lay.cols.size(), "the slabs hold %zu entries, cols %zu", at, lay.cols.size());
    uint64_t h = 1469598103934665603ull;
    for (uint16_t c : lay.cols) { h = (h ^ (c & 0xFFu)) * 1099511628211ull; h = (h ^ (c >> 8)) * 1099511628211ull; }
    printf("cols %zu entries fnv1a64 %016llx\n", lay.cols.size(), (unsigned long long)h);
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
