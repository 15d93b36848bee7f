// layered_csr_layout.cc -- steps, slabs and the column table of the on-chip layered kernel for any H (layered_csr_layout.h)
#include "layered_csr_layout.h"

#include <algorithm>

namespace ldpc {

CsrSteps csr_layout_steps(int N, const int32_t *row_ptr, const int32_t *col_idx, const int32_t *layer_ptr, int nlayers) {
    CsrSteps s;
    auto &steps = s.rows;
    std::vector<int32_t> stamp((size_t)N, -1);      // the last step that touched a column
    for (int l = 0; l < nlayers; l++) {
        bool clash = steps.empty();
        for (int m = layer_ptr[l]; m < layer_ptr[l + 1] && !clash; m++)
            for (int q = row_ptr[m]; q < row_ptr[m + 1] && !clash; q++) clash = stamp[col_idx[q]] == (int)steps.size() - 1;
        if (clash) steps.emplace_back();
        for (int m = layer_ptr[l]; m < layer_ptr[l + 1]; m++) {
            steps.back().push_back(m);
            for (int q = row_ptr[m]; q < row_ptr[m + 1]; q++) stamp[col_idx[q]] = (int)steps.size() - 1;
        }
    }
    auto deg = [&](int m) { return row_ptr[m + 1] - row_ptr[m]; };
    for (auto &st : steps) {
        std::stable_sort(st.begin(), st.end(), [&](int a, int b) { return deg(a) > deg(b); });   // heaviest first: uniform waves
        s.rmax = std::max(s.rmax, st.size());
    }
    return s;
}

CsrLayout csr_layout_pack(const CsrSteps &steps, const int32_t *row_ptr, const int32_t *col_idx, int T) {
    CsrLayout o;
    auto deg = [&](int m) { return row_ptr[m + 1] - row_ptr[m]; };
    const int W = T / 64;
    o.step_ptr.push_back(0);
    for (auto &st : steps.rows) {
        for (size_t r0 = 0; r0 < st.size(); r0 += T) {
            const int nr = (int)std::min<size_t>(T, st.size() - r0), D = deg(st[r0]);
            o.slab.push_back((int32_t)o.cols.size()); o.slab.push_back(D);
            const size_t base = o.cols.size();
            o.cols.resize(base + (size_t)D * T, kNoEdge);
            for (int i = 0; i < nr; i++) {
                const int m = st[r0 + i];
                for (int k = 0; k < deg(m); k++) o.cols[base + (size_t)k * T + i] = (uint16_t)col_idx[row_ptr[m] + k];
            }
            for (int w = 0; w < W; w++) {
                int wd = 0; bool uni = true;
                for (int i = 64 * w; i < 64 * w + 64; i++) {
                    const int d = i < nr ? deg(st[r0 + i]) : 0;
                    if (i == 64 * w) wd = d; else uni = uni && d == wd;
                    wd = std::max(wd, d);
                }
                o.wdeg.push_back(wd | (uni ? 0x100 : 0));
            }
        }
        o.step_ptr.push_back((int32_t)(o.slab.size() / 2));
    }
    o.nslab = (int)(o.slab.size() / 2);
    return o;
}

}  // namespace ldpc
