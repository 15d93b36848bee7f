// cascade.hip -- the three kernels of the two-stage decode (ldpc_cascade_decode_dev; the rule: cascade.h, restated in tests/cascade_spec.py).
// Between stage 1's decode and stage 2's: `select` compacts the frames stage 1 did not converge on into idx, `gather` copies their channel
// LLRs into the dense buffer stage 2 decodes; after stage 2's decode `scatter` puts its results where those frames were.  All on one stream,
// nothing read back: gather and scatter read the count from stats[1].
//
// select: ONE workgroup of 1024 threads walks the flags in chunks of 1024 frames.  A lane's place inside its wave is the number of set
// ballot bits below it (mbcnt), the 16 wave totals go through LDS and every lane adds up the ones before its own wave, a running count is
// carried from chunk to chunk in a register (the same in every lane).  The order is the frame order by construction: no atomic takes part.
// gather / scatter: a workgroup per compact row.  Rows are dense, N * es bytes, so with N * es no multiple of 16 every row sits differently
// against a 16-byte boundary: where source and destination row sit ALIKE the row moves 16 bytes a lane between an element-wise head and
// tail, otherwise element by element throughout (the traffic is a few per cent of what stage 1 reads).  Padding rows (gather, j >= count)
// are the LLR -1 in the buffer's format, a frame every decoder stops on before its first sweep.  The one atomic is scatter's count of
// frames that failed again (stats[2], zeroed by select): it orders nothing.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cascade.h"

namespace ldpc {

__global__ __launch_bounds__(kCascadeSelectThreads) void cascade_select_kernel(const uint8_t *__restrict__ conv, int32_t *__restrict__ idx, uint8_t *__restrict__ stage,
                                                                               uint32_t *__restrict__ stats, int batch, int capacity) {
    __shared__ uint32_t wcount[kCascadeSelectThreads / 64];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int chunks = (int)(((unsigned)batch + (unsigned)kCascadeSelectThreads - 1u) / (unsigned)kCascadeSelectThreads);
    uint32_t running = 0u;
    for (int c = 0; c < chunks; c++) {
        const size_t f = (size_t)c * kCascadeSelectThreads + tid;
        const bool live = f < (size_t)batch;
        const bool fail = live && conv[f] == 0;
        const unsigned long long m = __ballot(fail);
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if ((tid & 63) == 0) wcount[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0u, total = 0u;
#pragma unroll
        for (int w = 0; w < kCascadeSelectThreads / 64; w++) {
            const uint32_t n = wcount[w];
            before += w < wave ? n : 0u;
            total += n;
        }
        const uint32_t pos = running + before + below;
        if (fail && pos < (uint32_t)capacity) idx[pos] = (int32_t)f;
        if (stage && live) stage[f] = 1;
        running += total;
        __syncthreads();   // wcount is written again in the next chunk
    }
    if (tid == 0) {
        stats[0] = running;
        stats[1] = running < (uint32_t)capacity ? running : (uint32_t)capacity;
        stats[2] = 0u;
    }
}

// n elements from src to dst, both aligned to T, by the nt threads of a workgroup
template <typename T>
static __device__ __forceinline__ void row_copy(T *dst, const T *src, int n, int tid, int nt) {
    constexpr int PER = 16 / (int)sizeof(T);
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15u) == 0u) {
        const int head = min(n, (int)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) / sizeof(T)));
        const int nvec = (n - head) / PER;
        for (int i = tid; i < head; i += nt) dst[i] = src[i];
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src + head);   // 16-byte aligned, nvec * 16 bytes inside the row
        uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
        for (int v = tid; v < nvec; v += nt) d4[v] = s4[v];
        for (int i = head + nvec * PER + tid; i < n; i += nt) dst[i] = src[i];
    } else {
        for (int i = tid; i < n; i += nt) dst[i] = src[i];
    }
}

// n elements `pad` (pad4: the same pattern over 16 bytes)
template <typename T>
static __device__ __forceinline__ void row_fill(T *dst, T pad, uint32_t pad4, int n, int tid, int nt) {
    constexpr int PER = 16 / (int)sizeof(T);
    const int head = min(n, (int)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) / sizeof(T)));
    const int nvec = (n - head) / PER;
    for (int i = tid; i < head; i += nt) dst[i] = pad;
    uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
    for (int v = tid; v < nvec; v += nt) d4[v] = make_uint4(pad4, pad4, pad4, pad4);
    for (int i = head + nvec * PER + tid; i < n; i += nt) dst[i] = pad;
}

template <typename T>
__global__ __launch_bounds__(256) void cascade_gather_kernel(const T *llr, const int32_t *__restrict__ idx, const uint32_t *__restrict__ stats, T *out, int N, T pad,
                                                             uint32_t pad4) {
    const uint32_t j = blockIdx.x;                    // < capacity: the grid
    T *dst = out + (size_t)j * N;
    if (j < stats[1]) row_copy<T>(dst, llr + (size_t)idx[j] * N, N, threadIdx.x, 256);
    else row_fill<T>(dst, pad, pad4, N, threadIdx.x, 256);
}

__global__ __launch_bounds__(256) void cascade_scatter_kernel(const int32_t *__restrict__ idx, const uint8_t *bits2, const int32_t *__restrict__ iters2,
                                                              const uint8_t *__restrict__ conv2, uint8_t *bits, int32_t *iters, uint8_t *conv, uint8_t *stage, uint32_t *stats,
                                                              int N) {
    const uint32_t j = blockIdx.x;
    if (j >= stats[1]) return;
    const size_t f = (size_t)idx[j];
    row_copy<uint8_t>(bits + f * N, bits2 + (size_t)j * N, N, threadIdx.x, 256);
    if (threadIdx.x == 0) {
        const uint8_t cv = conv2[j];
        iters[f] = iters2[j];
        conv[f] = cv;
        if (stage) stage[f] = 2;
        if (cv == 0) atomicAdd(&stats[2], 1u);
    }
}

static int cascade_launched(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(LDPC_EHIP, "%s: %s", what, hipGetErrorString(e));
    return LDPC_OK;
}

int cascade_select_launch(hipStream_t st, int batch, int capacity, const uint8_t *conv, int32_t *idx, uint8_t *stage, uint32_t *stats) {
    hipLaunchKernelGGL(cascade_select_kernel, dim3(1), dim3(kCascadeSelectThreads), 0, st, conv, idx, stage, stats, batch, capacity);
    return cascade_launched("ldpc_cascade_decode_dev (select)");
}

int cascade_gather_launch(hipStream_t st, int N, int es, int capacity, const void *llr, const int32_t *idx, const uint32_t *stats, void *out) {
    const dim3 grid((unsigned)capacity), block(256);
    if (es == 4) hipLaunchKernelGGL(cascade_gather_kernel<uint32_t>, grid, block, 0, st, (const uint32_t *)llr, idx, stats, (uint32_t *)out, N, 0xBF800000u, 0xBF800000u);
    else if (es == 2) hipLaunchKernelGGL(cascade_gather_kernel<uint16_t>, grid, block, 0, st, (const uint16_t *)llr, idx, stats, (uint16_t *)out, N, (uint16_t)0xBC00u, 0xBC00BC00u);
    else hipLaunchKernelGGL(cascade_gather_kernel<uint8_t>, grid, block, 0, st, (const uint8_t *)llr, idx, stats, (uint8_t *)out, N, (uint8_t)0xFFu, 0xFFFFFFFFu);
    return cascade_launched("ldpc_cascade_decode_dev (gather)");
}

int cascade_scatter_launch(hipStream_t st, int N, int capacity, const int32_t *idx, const uint8_t *bits2, const int32_t *iters2, const uint8_t *conv2, uint8_t *bits,
                           int32_t *iters, uint8_t *conv, uint8_t *stage, uint32_t *stats) {
    hipLaunchKernelGGL(cascade_scatter_kernel, dim3((unsigned)capacity), dim3(256), 0, st, idx, bits2, iters2, conv2, bits, iters, conv, stage, stats, N);
    return cascade_launched("ldpc_cascade_decode_dev (scatter)");
}

}  // namespace ldpc
