// cascade.h -- the two-stage decode of include/ldpc_hip.h (ldpc_cascade): the three kernels between the two contexts' own decodes.  The
// rule is restated in tests/cascade_spec.py.  Nothing is read back to the host: the number of frames that go on lives in stats[1], in device
// memory, and every kernel after `select` reads it there.  The object is created and driven in api.cc (ldpc_cascade_create,
// ldpc_cascade_decode_dev); the kernels are in cascade.hip.
#pragma once
#include "internal.h"

namespace ldpc {

constexpr int kCascadeSelectThreads = 1024;   // one workgroup: the running count never leaves it

// idx[0 .. min(n, capacity)) = the frames f < batch with conv[f] == 0, ascending (n of them); stage[f] = 1 for every f < batch (stage may be
// null); stats[0] = n, stats[1] = min(n, capacity), stats[2] = 0
int cascade_select_launch(hipStream_t st, int batch, int capacity, const uint8_t *conv, int32_t *idx, uint8_t *stage, uint32_t *stats);
// out [capacity][N] of es-byte elements (4, 2, 1): row j < stats[1] = row idx[j] of llr, every other row = the LLR -1 in that format
// (0xBF800000, 0xBC00, 0xFF).  llr and out aligned to es
int cascade_gather_launch(hipStream_t st, int N, int es, int capacity, const void *llr, const int32_t *idx, const uint32_t *stats, void *out);
// rows j < stats[1]: bits[idx[j]] = bits2[j] (N bytes), iters[idx[j]] = iters2[j], conv[idx[j]] = conv2[j], stage[idx[j]] = 2 (stage may
// be null), stats[2] += (conv2[j] == 0)
int cascade_scatter_launch(hipStream_t st, int N, int capacity, const int32_t *idx, const uint8_t *bits2, const int32_t *iters2, const uint8_t *conv2, uint8_t *bits,
                           int32_t *iters, uint8_t *conv, uint8_t *stage, uint32_t *stats);

}  // namespace ldpc
