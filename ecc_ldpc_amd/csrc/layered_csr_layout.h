// layered_csr_layout.h -- the graph work of csrc/layered_csr.hip as host code of its own (plain C++, no HIP header: it compiles with any
// host compiler and runs under a sanitizer, tools/layered_csr_layout_main.cc).  A CSR matrix and its layers go in; out come the barrier
// STEPS, and -- once the caller has chosen T, the threads of a workgroup -- the tables the kernels read: the column table
// [slab][edge k][thread], the slabs, the per-wave weights and the slabs of each step.  layered_csr.hip's header says what they mean.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace ldpc {

constexpr uint16_t kNoEdge = 0xFFFF;    // a neutral entry of the column table: past the row's weight, or a lane without a row

// barrier steps: maximal runs of consecutive layers that share no column, each step's rows sorted by weight, heaviest first (stable)
struct CsrSteps {
    std::vector<std::vector<int>> rows;     // [step]: row indices
    size_t rmax = 1;                        // the rows of the largest step (1 when there is none)
};
CsrSteps csr_layout_steps(int N, const int32_t *row_ptr, const int32_t *col_idx, const int32_t *layer_ptr, int nlayers);

struct CsrLayout {
    std::vector<uint16_t> cols;     // per slab, [edge k < slab weight][thread]: column index, kNoEdge past the row's weight
    std::vector<int32_t> slab;      // [nslab][2]: {first entry in cols, slab weight (that of its first, heaviest row)}
    std::vector<int32_t> wdeg;      // [nslab][T / 64]: the heaviest row of each wave (0: idle), | 0x100 when all 64 rows of the wave have that weight
    std::vector<int32_t> step_ptr;  // [nstep + 1]: the slabs of each barrier step
    int nslab = 0;
};
// T: a multiple of 64.  Each step is cut into slabs of T rows, thread t taking row t of every slab of the step
CsrLayout csr_layout_pack(const CsrSteps &steps, const int32_t *row_ptr, const int32_t *col_idx, int T);

}  // namespace ldpc
