// api.cc -- the C ABI of include/ldpc_hip.h: graph objects, decoder replicas, host<->device plumbing.
// No C++ exception leaves this file; every failure becomes an LDPC_E* code + thread-local message.
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <set>

#include "backend.h"
#include "demap.h"
#include "interleaver.h"
#include "fading.h"
#include "ratematch.h"
#include "bch.h"
#include "cascade.h"
#include "crc.h"
#include "jit.h"
#include "sim.h"
#include "systematic.h"

namespace ldpc {
static thread_local char g_err[512] = "";
static thread_local int g_err_code = 0;
int set_error(int code, const char *fmt, ...) {
    g_err_code = code;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    // messages may quote bytes of a damaged input file: keep the text printable ASCII
    for (char *q = g_err; *q; q++)
        if ((unsigned char)*q < 0x20 || (unsigned char)*q > 0x7e) *q = '?';
    return code;
}
}  // namespace ldpc
using ldpc::set_error;

#define HIPCHK(x)                                                                                \
    do {                                                                                         \
        hipError_t e_ = (x);                                                                     \
        if (e_ != hipSuccess) return set_error(LDPC_EHIP, "%s: %s", #x, hipGetErrorString(e_)); \
    } while (0)
#define HIPCHK_NULL(x)                                                               \
    do {                                                                             \
        hipError_t e_ = (x);                                                         \
        if (e_ != hipSuccess) {                                                      \
            set_error(LDPC_EHIP, "%s: %s", #x, hipGetErrorString(e_));               \
            return nullptr;                                                          \
        }                                                                            \
    } while (0)

struct ldpc_ctx {
    const ldpc_code *code = nullptr;
    int max_batch = 0, device = 0, schedule = LDPC_SCHED_FLOODING, dtype = LDPC_F32;
    float llr_qscale = 0.f;             // LDPC_I8: the quantiser's scale (0 for every other dtype)
    int cn_rule = LDPC_CN_MINSUM;           // LDPC_CN_AMINSTAR: the A-min* row of csrc/layered_csr.hip (then cn_scale = cn_offset = 0)
    float cn_scale = 0.f, cn_offset = 0.f;  // the min-sum check-node rule the kernel computes with (0.75, 0 unless configured; 0, 0: tanh)
    hipStream_t stream = nullptr;
    ldpc::Backend *backend = nullptr;   // the context's decoder (select.cc make_backend)
    // staging of the host-pointer entry points, allocated on first use.  kSlots slots, each with its own stream
    // running H2D -> decode -> D2H for one chunk, so that the copies of one chunk overlap the decode of another.
    // The decodes themselves never overlap: each waits for `decoded`, recorded after the previous chunk's decode
    // (backend.h: a backend's decode may keep device state across launches; the flood path uses slot 0 with the
    // whole batch).  Measured on MI355X: a third slot changes nothing (65 536 jpl.4096 frames, pinned fp16
    // LLRs: 44.7 ms with 2 and with 3) -- the copies of both directions together run at ~25-32 GB/s, which is the
    // bound, not the pipeline depth.
    static constexpr int kSlots = 2;
    hipStream_t pstream[kSlots] = {};   // [0] aliases `stream`
    hipEvent_t decoded = nullptr;       // (slots > 1) recorded after each chunk's decode; the next chunk's decode waits for it
    int slots = 0, chunk = 0;
    void *d_in[kSlots] = {};            // [chunk][N] float, double, half or int8
    uint8_t *d_bits[kSlots] = {};       // [chunk][N]
    int32_t *d_iters[kSlots] = {};
    uint8_t *d_conv[kSlots] = {};
    double *d_final[kSlots] = {};       // [chunk][N], only when final LLRs are requested
    // latency path of the host-pointer entry points (<= kSmallFrames frames, e.g. ldpc_decode_one): page-locked
    // bounce buffers and ONE device block for bits|iters|converged, so a call costs one H2D copy, one launch and
    // one D2H copy instead of four pageable copies
    static constexpr int kSmallFrames = 16;
    void *h_small_in = nullptr, *d_small_in = nullptr;   // its own 16-frame device input: no full-size staging
    uint8_t *h_small_out = nullptr, *d_small_out = nullptr;
    // zero-copy path: outputs the caller gave as pageable memory while llr/bits are page-locked
    uint8_t *d_unpacked = nullptr;   // packed-result entry points: one byte per bit [max_batch][N], then packed (sim.hip pack_bits)
    uint8_t *d_packed = nullptr;     // ... and the packed image the host-pointer flavour copies back [max_batch][ceil(N/8)]
    int32_t *d_zc_iters = nullptr;
    uint8_t *d_zc_conv = nullptr;
    ldpc::KernelTimer timer;
    // what a decode state remembers of the context it was made for: never reused, unlike the context's address
    uint64_t serial = 0;
};
// the serials of the live contexts (under g_ctx_mu): a decode state asks here before it touches its context
static std::mutex g_ctx_mu;
static std::set<uint64_t> g_live_ctx;
static uint64_t g_next_serial = 1;
static bool ctx_alive(uint64_t serial) {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    return g_live_ctx.count(serial) != 0;
}

// Device selection.  ldpc_init(d) validates device d and makes it the CALLING THREAD's device (thread-local); the first
// device any thread initialised is the process default for threads that never called ldpc_init.  Objects remember
// the device they were created on, so several threads can drive several GPUs from one process
// (Utils.hs:53,63-69: maxThreadCount replicas, chosen by thread).  ldpc_ctx_create_on names the device explicitly.
static std::mutex g_mu;
static int g_default_device = -1;
static uint64_t g_checked_mask = 0;          // devices that passed check_device (bit d)
static thread_local int t_device = -1;

static int check_device(int device) {
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (device >= 0 && device < 64 && ((g_checked_mask >> device) & 1u)) return LDPC_OK;
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return set_error(LDPC_ENODEVICE, "no HIP device visible (%s); the HIP path has no CPU fallback",
                         e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device < 0 || device >= n || device >= 64) return set_error(LDPC_EINVAL, "device %d out of range [0,%d)", device, n);
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, device));
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0)
        return set_error(LDPC_ENODEVICE, "device %d is %s; libldpc_hip.so carries gfx950 code objects only", device, p.gcnArchName);
    std::lock_guard<std::mutex> lk(g_mu);
    g_checked_mask |= 1ull << device;
    return LDPC_OK;
}
static int current_device() {   // the calling thread's device, else the process default, else -1
    if (t_device >= 0) return t_device;
    std::lock_guard<std::mutex> lk(g_mu);
    return g_default_device;
}

extern "C" {

const char *ldpc_last_error(void) { return ldpc::g_err; }
int ldpc_last_error_code(void) { return ldpc::g_err_code; }
int ldpc_abi_version(void) { return 3; }

int ldpc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ldpc_init(int device) {
    int rc = check_device(device);
    if (rc != LDPC_OK) return rc;
    HIPCHK(hipSetDevice(device));
    t_device = device;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_default_device < 0) g_default_device = device;
    return LDPC_OK;
}

int ldpc_shutdown(void) {
    t_device = -1;
    std::lock_guard<std::mutex> lk(g_mu);
    g_default_device = -1;
    return LDPC_OK;
}

int ldpc_current_device(void) { return current_device(); }

// ------------------------------------------------------------------------------- graph
static int finish_code(ldpc_code *c) {
    c->E = c->row_ptr[c->M];
    c->col_ptr.assign((size_t)c->N + 1, 0);
    c->max_row_deg = 0;
    c->min_row_deg = c->M > 0 ? (1 << 30) : 0;
    for (int m = 0; m < c->M; m++) {
        int b = c->row_ptr[m], e = c->row_ptr[m + 1];
        if (e < b) return set_error(LDPC_EINVAL, "row_ptr not monotone at row %d", m);
        c->max_row_deg = std::max(c->max_row_deg, e - b);
        c->min_row_deg = std::min(c->min_row_deg, e - b);
        for (int q = b; q < e; q++) {
            int col = c->col_idx[q];
            if (col < 0 || col >= c->N) return set_error(LDPC_EINVAL, "column %d out of range in row %d", col, m);
            if (q > b && c->col_idx[q - 1] >= col) return set_error(LDPC_EINVAL, "columns of row %d not strictly ascending", m);
            c->col_ptr[col + 1]++;
        }
    }
    c->max_col_deg = 0;
    for (int j = 0; j < c->N; j++) {
        c->max_col_deg = std::max(c->max_col_deg, c->col_ptr[j + 1]);
        c->col_ptr[j + 1] += c->col_ptr[j];
    }
    // default layers: block rows of a QC code (column-disjoint: one circulant per block), single rows otherwise
    c->layer_ptr.clear();
    if (c->sz > 0) for (int br = 0; br <= c->block_rows; br++) c->layer_ptr.push_back(br * c->sz);
    else for (int m = 0; m <= c->M; m++) c->layer_ptr.push_back(m);
    c->csc_edge.assign((size_t)c->E, 0);
    std::vector<int32_t> fill(c->col_ptr.begin(), c->col_ptr.end() - 1);
    for (int m = 0; m < c->M; m++)
        for (int q = c->row_ptr[m]; q < c->row_ptr[m + 1]; q++) c->csc_edge[fill[c->col_idx[q]]++] = q;
    return LDPC_OK;
}

ldpc_code *ldpc_code_create_csr(int M, int N, const int32_t *row_ptr, const int32_t *col_idx) {
    if (M <= 0 || N <= 0 || M > (1 << 24) || N > (1 << 24) || !row_ptr || !col_idx || row_ptr[0] != 0 || row_ptr[M] < 0 ||
        row_ptr[M] > (1 << 30)) {
        set_error(LDPC_EINVAL, "ldpc_code_create_csr: bad arguments (M=%d N=%d)", M, N);
        return nullptr;
    }
    ldpc_code *c = new (std::nothrow) ldpc_code();
    if (!c) { set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    try {
        c->M = M; c->N = N;
        c->row_ptr.assign(row_ptr, row_ptr + M + 1);
        c->col_idx.assign(col_idx, col_idx + row_ptr[M]);
        if (finish_code(c) != LDPC_OK) { delete c; return nullptr; }
    } catch (...) { delete c; set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    return c;
}

ldpc_code *ldpc_code_create_qc(int sz, int block_rows, int block_cols, const int32_t *offsets) {
    if (sz <= 0 || block_rows <= 0 || block_cols <= 0 || !offsets) {
        set_error(LDPC_EINVAL, "ldpc_code_create_qc: bad arguments (sz=%d %dx%d)", sz, block_rows, block_cols);
        return nullptr;
    }
    // expanded sizes must stay well inside int32 (edge ids are int32): M, N <= 2^24, E <= 2^30
    const long long kMaxDim = 1ll << 24;
    if ((long long)sz * block_rows > kMaxDim || (long long)sz * block_cols > kMaxDim ||
        (long long)block_rows * block_cols > (1ll << 24)) {
        set_error(LDPC_EUNSUPPORTED, "ldpc_code_create_qc: %d x %d blocks of size %d expand beyond 2^24 rows/columns", block_rows, block_cols, sz);
        return nullptr;
    }
    long long nnz_blocks = 0;
    for (int i = 0; i < block_rows * block_cols; i++) nnz_blocks += offsets[i] >= 0;
    if (nnz_blocks * sz > (1ll << 30)) {
        set_error(LDPC_EUNSUPPORTED, "ldpc_code_create_qc: %lld edges exceed 2^30", nnz_blocks * sz);
        return nullptr;
    }
    for (int i = 0; i < block_rows * block_cols; i++)
        if (offsets[i] < -1 || offsets[i] >= sz) {
            set_error(LDPC_EINVAL, "offset %d at block %d outside [-1,%d)", offsets[i], i, sz);
            return nullptr;
        }
    ldpc_code *c = new (std::nothrow) ldpc_code();
    if (!c) { set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    try {
        c->sz = sz; c->block_rows = block_rows; c->block_cols = block_cols;
        c->offsets.assign(offsets, offsets + (size_t)block_rows * block_cols);
        c->M = sz * block_rows; c->N = sz * block_cols;
        c->row_ptr.assign((size_t)c->M + 1, 0);
        // row r of block-row br: one entry per non-empty block, column bc*sz + (r+off) mod sz
        // (QuasiCyclic.hs:19-25); block columns ascend, so columns ascend.
        for (int br = 0; br < block_rows; br++)
            for (int r = 0; r < sz; r++) {
                int m = br * sz + r;
                for (int bc = 0; bc < block_cols; bc++) {
                    int off = offsets[(size_t)br * block_cols + bc];
                    if (off >= 0) c->col_idx.push_back(bc * sz + (r + off) % sz);
                }
                c->row_ptr[m + 1] = (int32_t)c->col_idx.size();
            }
        if (finish_code(c) != LDPC_OK) { delete c; return nullptr; }
    } catch (...) { delete c; set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    return c;
}

static void code_free_device(ldpc_code *c) {
    std::lock_guard<std::mutex> lk(c->dev_mu);
    int prev = -1;
    (void)hipGetDevice(&prev);
    for (auto &kv : c->dev) {
        if (hipSetDevice(kv.first) != hipSuccess) continue;
        (void)hipFree(kv.second.row_ptr); (void)hipFree(kv.second.col_idx); (void)hipFree(kv.second.col_ptr); (void)hipFree(kv.second.csc_edge);
    }
    c->dev.clear();
    if (prev >= 0) (void)hipSetDevice(prev);
}

void ldpc_code_destroy(ldpc_code *code) {
    if (!code) return;
    code_free_device(code);
    delete code;
}

int ldpc_code_dims(const ldpc_code *code, int *M, int *N, int *E) {
    if (!code) return set_error(LDPC_EINVAL, "null code");
    if (M) *M = code->M;
    if (N) *N = code->N;
    if (E) *E = code->E;
    return LDPC_OK;
}

int ldpc_qc_layer_order(int block_rows, int block_cols, const int32_t *offsets, int run, int32_t *perm) {
    if (block_rows <= 0 || block_cols <= 0 || !offsets || !perm || run < 1 || run > 8) return set_error(LDPC_EINVAL, "ldpc_qc_layer_order: bad arguments");
    try {
        const int Q = block_rows;
        auto hit = [&](int br, int bc) { return offsets[(size_t)br * block_cols + bc] >= 0; };
        std::vector<char> ok((size_t)Q * Q, 0);          // ok[i][j]: block rows i and j share no block column
        for (int i = 0; i < Q; i++)
            for (int j = i + 1; j < Q; j++) {
                bool share = false;
                for (int bc = 0; bc < block_cols && !share; bc++) share = hit(i, bc) && hit(j, bc);
                ok[(size_t)i * Q + j] = ok[(size_t)j * Q + i] = share ? 0 : 1;
            }
        std::vector<char> free_((size_t)Q, 1);
        std::vector<std::vector<int>> runs;
        int left = Q;
        while (left > 0) {
            // compatible rows still free, per free row; the run starts with the row that has the fewest, ties to the lower index
            std::vector<int> deg((size_t)Q, 0);
            for (int i = 0; i < Q; i++) if (free_[i]) for (int j = 0; j < Q; j++) if (free_[j] && ok[(size_t)i * Q + j]) deg[i]++;
            int first = -1;
            for (int i = 0; i < Q; i++) if (free_[i] && (first < 0 || deg[i] < deg[first])) first = i;
            std::vector<int> r{first};
            free_[first] = 0; left--;
            while ((int)r.size() < run) {
                int best = -1;
                for (int j = 0; j < Q; j++) {
                    if (!free_[j]) continue;
                    bool all = true;
                    for (int i : r) all = all && ok[(size_t)i * Q + j];
                    if (all && (best < 0 || deg[j] < deg[best])) best = j;
                }
                if (best < 0) break;
                r.push_back(best); free_[best] = 0; left--;
            }
            std::sort(r.begin(), r.end());
            runs.push_back(r);
        }
        std::stable_sort(runs.begin(), runs.end(), [](const std::vector<int> &a, const std::vector<int> &b) {
            return a.size() != b.size() ? a.size() > b.size() : a < b; });
        int n = 0, full = 0;
        for (auto &r : runs) { if ((int)r.size() == run) full++; for (int br : r) perm[n++] = br; }
        return full;
    } catch (...) { return set_error(LDPC_ENOMEM, "out of host memory"); }
}

int ldpc_csr_layer_order(int M, int N, const int32_t *row_ptr, const int32_t *col_idx, int max_rows, int32_t *perm, int32_t *layer_ptr) {
    if (M <= 0 || N <= 0 || !row_ptr || !col_idx || max_rows < 0 || !perm || !layer_ptr || row_ptr[0] != 0)
        return set_error(LDPC_EINVAL, "ldpc_csr_layer_order: bad arguments (M=%d N=%d max_rows=%d)", M, N, max_rows);
    for (int m = 0; m < M; m++) {
        if (row_ptr[m + 1] < row_ptr[m]) return set_error(LDPC_EINVAL, "ldpc_csr_layer_order: row_ptr decreases at row %d", m);
        for (int q = row_ptr[m]; q < row_ptr[m + 1]; q++)
            if (col_idx[q] < 0 || col_idx[q] >= N || (q > row_ptr[m] && col_idx[q] <= col_idx[q - 1]))
                return set_error(LDPC_EINVAL, "ldpc_csr_layer_order: row %d: columns not strictly ascending inside [0, %d)", m, N);
    }
    try {
        // first fit in file order: each row joins the lowest layer that holds none of its columns and has room
        std::vector<std::vector<int32_t>> col_layers((size_t)N);   // per column: the layers that already hold it
        std::vector<int32_t> layer_of((size_t)M), size, stamp;
        std::set<int> open;                                       // layers with room (all of them when max_rows = 0)
        for (int m = 0; m < M; m++) {
            for (int q = row_ptr[m]; q < row_ptr[m + 1]; q++)
                for (int l : col_layers[col_idx[q]]) stamp[l] = m;
            int l = (int)size.size();
            for (int o : open) if (stamp[o] != m) { l = o; break; }
            if (l == (int)size.size()) { size.push_back(0); stamp.push_back(-1); open.insert(l); }
            layer_of[m] = l;
            if (++size[l] == max_rows) open.erase(l);
            for (int q = row_ptr[m]; q < row_ptr[m + 1]; q++) col_layers[col_idx[q]].push_back(l);
        }
        const int n = (int)size.size();
        layer_ptr[0] = 0;
        for (int l = 0; l < n; l++) layer_ptr[l + 1] = layer_ptr[l] + size[l];
        std::vector<int32_t> at(layer_ptr, layer_ptr + n);
        for (int m = 0; m < M; m++) perm[at[layer_of[m]]++] = m;   // rows of a layer in file order
        return n;
    } catch (...) { return set_error(LDPC_ENOMEM, "out of host memory"); }
}

// the rule of the encoder from H (include/ldpc_hip.h): order[j] = the row whose largest column is K + j
static int triangular_order(const char *who, int M, int N, const int32_t *row_ptr, const int32_t *col_idx, int32_t *order) {
    const int K = N - M;
    if (K <= 0) return set_error(LDPC_EUNSUPPORTED, "%s: M = %d >= N = %d leaves no message columns", who, M, N);
    try {
        std::vector<int32_t> owner((size_t)M, -1);
        for (int m = 0; m < M; m++) {
            if (row_ptr[m + 1] == row_ptr[m]) return set_error(LDPC_EUNSUPPORTED, "%s: row %d is empty", who, m);
            const int last = col_idx[row_ptr[m + 1] - 1];   // (columns ascend inside a row)
            if (last < K) return set_error(LDPC_EUNSUPPORTED, "%s: row %d ends in column %d, inside the message part (K = %d)", who, m, last, K);
            if (owner[last - K] >= 0) return set_error(LDPC_EUNSUPPORTED, "%s: rows %d and %d end in column %d", who, owner[last - K], m, last);
            owner[last - K] = m;
        }
        memcpy(order, owner.data(), sizeof(int32_t) * (size_t)M);   // M rows into M places without a collision: a bijection
    } catch (...) { return set_error(LDPC_ENOMEM, "out of host memory"); }
    return LDPC_OK;
}

int ldpc_csr_triangular_order(int M, int N, const int32_t *row_ptr, const int32_t *col_idx, int32_t *order) {
    if (M <= 0 || N <= 0 || !row_ptr || !col_idx || !order || row_ptr[0] != 0)
        return set_error(LDPC_EINVAL, "ldpc_csr_triangular_order: bad arguments (M=%d N=%d)", M, N);
    for (int m = 0; m < M; m++) {
        if (row_ptr[m + 1] < row_ptr[m]) return set_error(LDPC_EINVAL, "ldpc_csr_triangular_order: row_ptr decreases at row %d", m);
        for (int q = row_ptr[m]; q < row_ptr[m + 1]; q++)
            if (col_idx[q] < 0 || col_idx[q] >= N || (q > row_ptr[m] && col_idx[q] <= col_idx[q - 1]))
                return set_error(LDPC_EINVAL, "ldpc_csr_triangular_order: row %d: columns not strictly ascending inside [0, %d)", m, N);
    }
    return triangular_order("ldpc_csr_triangular_order", M, N, row_ptr, col_idx, order);
}

int ldpc_csr_systematic_form(int M, int N, const int32_t *row_ptr, const int32_t *col_idx, int32_t *msg_pos, int32_t *par_pos, int *K, int *rank, uint8_t *P) {
    if (!msg_pos || !par_pos || !K || !rank) return set_error(LDPC_EINVAL, "ldpc_csr_systematic_form: bad arguments (M=%d N=%d)", M, N);
    ldpc::SystematicForm sf;
    std::string err;
    const int rc = ldpc::systematic_form("ldpc_csr_systematic_form", M, N, row_ptr, col_idx, sf, err);
    if (rc != LDPC_OK) return set_error(rc, "%s", err.c_str());
    *K = sf.K; *rank = sf.rank;
    memcpy(msg_pos, sf.msg_pos.data(), sizeof(int32_t) * (size_t)sf.K);
    memcpy(par_pos, sf.par_pos.data(), sizeof(int32_t) * (size_t)sf.rank);
    if (P)
        for (int i = 0; i < sf.K; i++)
            for (int j = 0; j < sf.rank; j++) P[(size_t)i * sf.rank + j] = (uint8_t)((sf.P[(size_t)i * sf.pw64 + (j >> 6)] >> (j & 63)) & 1ull);
    return LDPC_OK;
}

int ldpc_code_set_layers(ldpc_code *code, int n_layers, const int32_t *layer_ptr) {
    if (!code || n_layers <= 0 || !layer_ptr) return set_error(LDPC_EINVAL, "ldpc_code_set_layers: bad arguments");
    {
        std::lock_guard<std::mutex> lk(code->dev_mu);
        if (!code->dev.empty()) return set_error(LDPC_EINVAL, "ldpc_code_set_layers: the code already has decoder contexts");
    }
    if (layer_ptr[0] != 0 || layer_ptr[n_layers] != code->M) return set_error(LDPC_EINVAL, "layers must cover rows 0..%d", code->M);
    try {
        std::vector<int32_t> seen((size_t)code->N, -1);
        for (int l = 0; l < n_layers; l++) {
            if (layer_ptr[l + 1] <= layer_ptr[l]) return set_error(LDPC_EINVAL, "layer %d is empty or out of order", l);
            for (int m = layer_ptr[l]; m < layer_ptr[l + 1]; m++)
                for (int q = code->row_ptr[m]; q < code->row_ptr[m + 1]; q++) {
                    if (seen[code->col_idx[q]] == l) return set_error(LDPC_EINVAL, "rows of layer %d share column %d", l, code->col_idx[q]);
                    seen[code->col_idx[q]] = l;
                }
        }
        code->layer_ptr.assign(layer_ptr, layer_ptr + n_layers + 1);
    } catch (...) { return set_error(LDPC_ENOMEM, "out of host memory"); }
    return LDPC_OK;
}

int ldpc_code_layers(const ldpc_code *code, int *n_layers, int32_t *layer_ptr) {
    if (!code) return set_error(LDPC_EINVAL, "null code");
    if (n_layers) *n_layers = (int)code->layer_ptr.size() - 1;
    if (layer_ptr) memcpy(layer_ptr, code->layer_ptr.data(), sizeof(int32_t) * code->layer_ptr.size());
    return LDPC_OK;
}

int ldpc_code_csr(const ldpc_code *code, int32_t *row_ptr, int32_t *col_idx) {
    if (!code || !row_ptr || !col_idx) return set_error(LDPC_EINVAL, "null argument");
    memcpy(row_ptr, code->row_ptr.data(), sizeof(int32_t) * ((size_t)code->M + 1));
    memcpy(col_idx, code->col_idx.data(), sizeof(int32_t) * (size_t)code->E);
    return LDPC_OK;
}

// the graph tables on `device` (uploaded by the first caller); the calling thread's current device must be `device`
static int code_upload(ldpc_code *c, int device, ldpc_code_dev *out) {
    std::lock_guard<std::mutex> lk(c->dev_mu);
    auto it = c->dev.find(device);
    if (it != c->dev.end()) { *out = it->second; return LDPC_OK; }
    ldpc_code_dev t;
    auto up = [&](int32_t **dst, const std::vector<int32_t> &v) -> int {
        size_t bytes = sizeof(int32_t) * std::max<size_t>(v.size(), 1);
        HIPCHK(hipMalloc((void **)dst, bytes));
        if (!v.empty()) HIPCHK(hipMemcpy(*dst, v.data(), sizeof(int32_t) * v.size(), hipMemcpyHostToDevice));
        return LDPC_OK;
    };
    int rc;
    if ((rc = up(&t.row_ptr, c->row_ptr)) || (rc = up(&t.col_idx, c->col_idx)) ||
        (rc = up(&t.col_ptr, c->col_ptr)) || (rc = up(&t.csc_edge, c->csc_edge))) {
        (void)hipFree(t.row_ptr); (void)hipFree(t.col_idx); (void)hipFree(t.col_ptr); (void)hipFree(t.csc_edge);   // a half-uploaded graph is not kept
        return rc;
    }
    c->dev[device] = t;
    *out = t;
    return LDPC_OK;
}

// ------------------------------------------------------------------------------- contexts
void ldpc_ctx_destroy(ldpc_ctx *ctx) {
    if (!ctx) return;
    {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        g_live_ctx.erase(ctx->serial);
    }
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    for (int i = 1; i < ldpc_ctx::kSlots; i++) if (ctx->pstream[i]) hipStreamSynchronize(ctx->pstream[i]);
    for (int i = 0; i < ldpc_ctx::kSlots; i++) { hipFree(ctx->d_in[i]); hipFree(ctx->d_bits[i]); hipFree(ctx->d_iters[i]); hipFree(ctx->d_conv[i]); hipFree(ctx->d_final[i]); }
    for (int i = 1; i < ldpc_ctx::kSlots; i++) if (ctx->pstream[i]) hipStreamDestroy(ctx->pstream[i]);
    if (ctx->decoded) (void)hipEventDestroy(ctx->decoded);
    if (ctx->h_small_in) (void)hipHostFree(ctx->h_small_in);
    if (ctx->h_small_out) (void)hipHostFree(ctx->h_small_out);
    (void)hipFree(ctx->d_small_out); (void)hipFree(ctx->d_small_in);
    (void)hipFree(ctx->d_zc_iters); (void)hipFree(ctx->d_zc_conv); (void)hipFree(ctx->d_unpacked); (void)hipFree(ctx->d_packed);
    delete ctx->backend;
    ctx->timer.destroy();
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

ldpc_ctx *ldpc_ctx_create_ex(const ldpc_code *code, int variant, int dtype, int max_batch, int path) {
    return ldpc_ctx_create_on(code, -1, variant, dtype, max_batch, path);   // -1: the calling thread's device
}

ldpc_ctx *ldpc_ctx_create_on(const ldpc_code *code, int device, int variant, int dtype, int max_batch, int path) {
    ldpc_ctx_config cfg{};
    cfg.struct_size = sizeof(cfg); cfg.device = device; cfg.variant = variant; cfg.dtype = dtype; cfg.max_batch = max_batch; cfg.path = path;
    cfg.schedule = LDPC_SCHED_FLOODING;
    return ldpc_ctx_create_cfg(code, &cfg);
}

const ldpc_code *ldpc_ctx_code(const ldpc_ctx *ctx) { return ctx ? ctx->code : nullptr; }
int ldpc_ctx_max_batch(const ldpc_ctx *ctx) { return ctx ? ctx->max_batch : set_error(LDPC_EINVAL, "null ctx"); }
int ldpc_ctx_device(const ldpc_ctx *ctx) { return ctx ? ctx->device : set_error(LDPC_EINVAL, "null ctx"); }
int ldpc_ctx_schedule(const ldpc_ctx *ctx) { return ctx ? ctx->schedule : set_error(LDPC_EINVAL, "null ctx"); }
float ldpc_ctx_llr_qscale(const ldpc_ctx *ctx) { return ctx ? ctx->llr_qscale : 0.f; }
float ldpc_ctx_cn_scale(const ldpc_ctx *ctx) { return ctx ? ctx->cn_scale : 0.f; }
float ldpc_ctx_cn_offset(const ldpc_ctx *ctx) { return ctx ? ctx->cn_offset : 0.f; }
int ldpc_ctx_cn_rule(const ldpc_ctx *ctx) { return ctx ? ctx->cn_rule : set_error(LDPC_EINVAL, "null ctx"); }

ldpc_ctx *ldpc_ctx_create_cfg(const ldpc_code *code_c, const ldpc_ctx_config *cfg) {
    if (!cfg || cfg->struct_size < offsetof(ldpc_ctx_config, schedule)) { set_error(LDPC_EINVAL, "ldpc_ctx_create_cfg: bad config"); return nullptr; }
    ldpc_code *code = const_cast<ldpc_code *>(code_c);
    const int variant = cfg->variant, dtype = cfg->dtype, max_batch = cfg->max_batch, path = cfg->path;
    // every field added after `path` is read when struct_size covers THAT field (a caller built against an older header passes the
    // size its structure had: 32 bytes with `schedule` as its last member before `sum_order` was added)
    const int schedule = cfg->struct_size >= offsetof(ldpc_ctx_config, schedule) + sizeof(int) ? cfg->schedule : LDPC_SCHED_FLOODING;
    if (schedule != LDPC_SCHED_FLOODING && schedule != LDPC_SCHED_LAYERED) { set_error(LDPC_EINVAL, "unknown schedule %d", schedule); return nullptr; }
    const int sum_order = cfg->struct_size >= offsetof(ldpc_ctx_config, sum_order) + sizeof(int) ? cfg->sum_order : LDPC_SUM_REFERENCE;
    if (sum_order != LDPC_SUM_REFERENCE && sum_order != LDPC_SUM_ARRAYLET && sum_order != LDPC_SUM_SPARSE) { set_error(LDPC_EINVAL, "unknown sum order %d", sum_order); return nullptr; }
    // llr_qscale sits where the structure ended in padding before it was added: it is looked at for LDPC_I8 alone, a dtype no caller
    // built against the older header can name
    float llr_qscale = dtype == LDPC_I8 && cfg->struct_size >= offsetof(ldpc_ctx_config, llr_qscale) + sizeof(float) ? cfg->llr_qscale : 0.f;
    if (!(llr_qscale >= 0.f) || llr_qscale > 3.4028234e38f) { set_error(LDPC_EINVAL, "llr_qscale %g: the quantiser's scale must be finite and > 0 (0: the default, 4)", (double)cfg->llr_qscale); return nullptr; }
    if (llr_qscale == 0.f) llr_qscale = 4.f;
    // the check-node rule: |msg'| = max(cn_scale * min - cn_offset, 0).  0 / absent, or an explicit (0.75, 0): the 3/4 of every kernel,
    // and the context is selected exactly as without the fields.  Anything else is a rule of its own (csrc/layered_csr.hip
    // layered_csr_kernel<D, Ruled<LT>>); an LDPC_I8 context computes with a / 16 and b quantiser steps, and one whose integers are (12, 0) is
    // the default context
    float cn_scale = cfg->struct_size >= offsetof(ldpc_ctx_config, cn_scale) + sizeof(float) ? cfg->cn_scale : 0.f;
    float cn_offset = cfg->struct_size >= offsetof(ldpc_ctx_config, cn_offset) + sizeof(float) ? cfg->cn_offset : 0.f;
    if (!(cn_scale >= 0.f && cn_scale <= 1.f)) { set_error(LDPC_EINVAL, "cn_scale %g: the check-node rule's scale must be finite and in (0, 1] (0: the default, 3/4)", (double)cn_scale); return nullptr; }
    if (!(cn_offset >= 0.f) || cn_offset > 3.4028234e38f) { set_error(LDPC_EINVAL, "cn_offset %g: the check-node rule's offset must be finite and >= 0", (double)cn_offset); return nullptr; }
    // cn_rule: LDPC_CN_AMINSTAR is the A-min* row (csrc/layered_csr.hip layered_csr_kernel<D, MinStar<LT>>), which has no scale and no offset
    const int cn_rule = cfg->struct_size >= offsetof(ldpc_ctx_config, cn_rule) + sizeof(int) ? cfg->cn_rule : LDPC_CN_MINSUM;
    if (cn_rule != LDPC_CN_MINSUM && cn_rule != LDPC_CN_AMINSTAR) { set_error(LDPC_EINVAL, "unknown cn_rule %d (LDPC_CN_MINSUM or LDPC_CN_AMINSTAR)", cn_rule); return nullptr; }
    const bool aminstar = cn_rule == LDPC_CN_AMINSTAR;
    if (aminstar && (cn_scale != 0.f || cn_offset != 0.f)) {
        set_error(LDPC_EINVAL, "cn_rule LDPC_CN_AMINSTAR has no scale and no offset: cn_scale %g and cn_offset %g must be 0", (double)cn_scale, (double)cn_offset);
        return nullptr;
    }
    if (cn_scale == 0.f) cn_scale = 0.75f;
    ldpc::CnRule rule{cn_scale, cn_offset, 12, 0};
    rule.kind = cn_rule;
    if (dtype == LDPC_I8 && !aminstar) {
        const float a = rintf(cn_scale * 16.f), b = rintf(cn_offset * llr_qscale);       // (ties to even; 16 alpha is exact)
        if (a < 1.f) { set_error(LDPC_EINVAL, "cn_scale %g: LDPC_I8 computes with rint(16 cn_scale) sixteenths, which is 0", (double)cn_scale); return nullptr; }
        if (!(b <= 127.f)) { set_error(LDPC_EINVAL, "cn_offset %g: LDPC_I8 computes with rint(cn_offset * llr_qscale) = %g quantiser steps, above 127", (double)cn_offset, (double)b); return nullptr; }
        rule.a = (int)a; rule.b = (int)b;
        rule.scale = (float)rule.a / 16.f; rule.offset = (float)rule.b / llr_qscale;
    }
    const bool has_rule = aminstar ? true : dtype == LDPC_I8 ? (rule.a != 12 || rule.b != 0) : (cn_scale != 0.75f || cn_offset != 0.f);
    // (a context with a rule of its own is refused by make_backend, whose message names the rule, not by the parity-mode checks below)
    if (!has_rule && sum_order != LDPC_SUM_REFERENCE && (schedule != LDPC_SCHED_FLOODING || path == LDPC_PATH_FUSED || cfg->dtype == LDPC_F16 || cfg->dtype == LDPC_F16PK)) {
        set_error(LDPC_EUNSUPPORTED, "LDPC_SUM_ARRAYLET / LDPC_SUM_SPARSE are parity modes: flooding schedule, flood path, f32 or f64");
        return nullptr;
    }
    if (!has_rule && variant == LDPC_TANH_CM && (dtype != LDPC_F64 || schedule != LDPC_SCHED_FLOODING || path == LDPC_PATH_FUSED)) {
        set_error(LDPC_EUNSUPPORTED, "LDPC_TANH_CM (arraylet-cm numerics) is a parity mode: f64, flooding schedule, flood path (an f32 kernel is 1e-5 away from either tanh flavour)");
        return nullptr;
    }
    if (!has_rule && variant == LDPC_TANH_CUDA32 && (dtype != LDPC_F32 || schedule != LDPC_SCHED_FLOODING || path == LDPC_PATH_FUSED || sum_order != LDPC_SUM_REFERENCE ||
                                        (code && code->max_row_deg > 32))) {
        set_error(LDPC_EUNSUPPORTED, "LDPC_TANH_CUDA32 (cuda-arraylet2 numerics) is a parity mode: f32, flooding schedule, flood path, rows up to weight 32");
        return nullptr;
    }
    if (!code || max_batch <= 0 || (variant != LDPC_TANH && variant != LDPC_MINSUM && variant != LDPC_TANH_CM && variant != LDPC_TANH_CUDA32) ||
        (dtype != LDPC_F32 && dtype != LDPC_F64 && dtype != LDPC_F16 && dtype != LDPC_F16PK && dtype != LDPC_I8) ||
        (path != LDPC_PATH_AUTO && path != LDPC_PATH_FLOOD && path != LDPC_PATH_FUSED)) {
        set_error(LDPC_EINVAL, "ldpc_ctx_create: bad arguments (variant=%d dtype=%d max_batch=%d path=%d)", variant, dtype, max_batch, path);
        return nullptr;
    }
    if (variant == LDPC_MINSUM && code->min_row_deg == 1) {
        set_error(LDPC_EDEGREE, "min-sum on a check row of degree 1 (the reference's foldr1 min' fails on [], Min.hs:79)");
        return nullptr;
    }
    int device = cfg->device;
    if (device < 0) device = current_device();
    if (device < 0) { set_error(LDPC_ENODEVICE, "ldpc_init() has not succeeded: no GPU bound (there is no CPU fallback)"); return nullptr; }
    if (check_device(device) != LDPC_OK) return nullptr;
    HIPCHK_NULL(hipSetDevice(device));
    ldpc_code_dev tabs;
    if (code_upload(code, device, &tabs) != LDPC_OK) return nullptr;

    ldpc::Backend *backend = ldpc::make_backend(*code, tabs, variant, dtype, schedule, sum_order, path, max_batch, llr_qscale, has_rule ? &rule : nullptr);
    if (!backend) return nullptr;
    ldpc_ctx *ctx = new (std::nothrow) ldpc_ctx();
    if (!ctx) { delete backend; set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    ctx->code = code; ctx->max_batch = max_batch; ctx->device = device; ctx->schedule = schedule; ctx->backend = backend;
    ctx->dtype = dtype; ctx->llr_qscale = dtype == LDPC_I8 ? llr_qscale : 0.f;
    const bool minsum = variant == LDPC_MINSUM;
    ctx->cn_scale = minsum && !aminstar ? rule.scale : 0.f; ctx->cn_offset = minsum && !aminstar ? rule.offset : 0.f; ctx->cn_rule = cn_rule;
    backend->timer = &ctx->timer;
    {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        ctx->serial = g_next_serial++;
        g_live_ctx.insert(ctx->serial);
    }
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        set_error(e == hipErrorOutOfMemory ? LDPC_ENOMEM : LDPC_EHIP, "hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking): %s", hipGetErrorString(e));
        ldpc_ctx_destroy(ctx);
        return nullptr;
    }
    // (the staging buffers of the host-pointer entry points are allocated on first use: a context driven
    //  through ldpc_decode_batch_dev with 65 536 frames would otherwise park 3 GB of HBM)
    return ctx;
}

ldpc_ctx *ldpc_ctx_create(const ldpc_code *code, int variant, int dtype, int max_batch) {
    return ldpc_ctx_create_ex(code, variant, dtype, max_batch, LDPC_PATH_AUTO);
}

int ldpc_ctx_path(const ldpc_ctx *ctx) { return ctx ? ctx->backend->path : set_error(LDPC_EINVAL, "null ctx"); }

void *ldpc_host_alloc(size_t bytes) {
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) { set_error(LDPC_ENOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e)); return nullptr; }
    return p;
}
void ldpc_host_free(void *p) { if (p) (void)hipHostFree(p); }

int ldpc_ctx_synchronize(ldpc_ctx *ctx) {
    if (!ctx) return set_error(LDPC_EINVAL, "null ctx");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return LDPC_OK;
}

// ------------------------------------------------------------------------------- decode
static int check_call(ldpc_ctx *ctx, int max_iters, int batch) {
    if (!ctx) return set_error(LDPC_EINVAL, "null ctx");
    if (max_iters < 0) return set_error(LDPC_EINVAL, "max_iters %d < 0", max_iters);
    if (batch < 0 || batch > ctx->max_batch) return set_error(LDPC_EINVAL, "batch %d outside [0,%d]", batch, ctx->max_batch);
    HIPCHK(hipSetDevice(ctx->device));
    return LDPC_OK;
}

// int8 LLRs (ldpc::LLR_I8) are the input of the fixed-point decoder alone
static int check_format(const ldpc_ctx *ctx, int fmt) {
    if (fmt == ldpc::LLR_I8 && ctx->dtype != LDPC_I8)
        return set_error(LDPC_EUNSUPPORTED, "int8 LLRs are accepted by LDPC_I8 contexts only (this context's dtype is %d)", ctx->dtype);
    return LDPC_OK;
}
static size_t llr_bytes(int fmt) { return fmt == ldpc::LLR_F64 ? 8 : fmt == ldpc::LLR_F16 ? 2 : fmt == ldpc::LLR_I8 ? 1 : 4; }
// the packed entry points' llr_f16 argument: 0 float32, 1 binary16 patterns, 2 int8
static int packed_format(int llr_f16) { return llr_f16 == 2 ? ldpc::LLR_I8 : llr_f16 ? ldpc::LLR_F16 : ldpc::LLR_F32; }

// device-side core: d_llr is [batch][N] of element type fmt (ldpc::LLR_F32 / LLR_F64 / LLR_F16 / LLR_I8); outputs device pointers (may be null)
static int decode_dev(ldpc_ctx *ctx, hipStream_t st, int max_iters, int batch, const void *d_llr, int fmt,
                      uint8_t *d_bits, int32_t *d_iters, uint8_t *d_conv, double *d_final, double *d_trace) {
    if (batch == 0) return LDPC_OK;
    return ctx->backend->decode(st, max_iters, batch, d_llr, fmt, d_bits, d_iters, d_conv, d_final, d_trace);
}

// frames per pipelined chunk of the host-pointer entry points (fused paths)
static constexpr int kHostChunk = 8192;

static int ensure_staging(ldpc_ctx *ctx, bool want_final) {
    const size_t N = (size_t)ctx->code->N;
    if (!ctx->d_in[0]) {
        const bool pipelined = ctx->backend->path == LDPC_PATH_FUSED && ctx->max_batch > kHostChunk;
        ctx->chunk = pipelined ? kHostChunk : ctx->max_batch;
        ctx->slots = pipelined ? std::min(ldpc_ctx::kSlots, (ctx->max_batch + kHostChunk - 1) / kHostChunk) : 1;
        ctx->pstream[0] = ctx->stream;
        hipError_t e = hipSuccess;
        for (int i = 1; i < ctx->slots && e == hipSuccess; i++) e = hipStreamCreateWithFlags(&ctx->pstream[i], hipStreamNonBlocking);
        if (ctx->slots > 1 && e == hipSuccess) e = hipEventCreateWithFlags(&ctx->decoded, hipEventDisableTiming);
        for (int i = 0; i < ctx->slots && e == hipSuccess; i++) {
            const size_t c = (size_t)ctx->chunk;
            e = hipMalloc(&ctx->d_in[i], c * N * sizeof(double));
            if (e == hipSuccess) e = hipMalloc((void **)&ctx->d_bits[i], c * N);
            if (e == hipSuccess) e = hipMalloc((void **)&ctx->d_iters[i], sizeof(int32_t) * c);
            if (e == hipSuccess) e = hipMalloc((void **)&ctx->d_conv[i], c);
        }
        if (e != hipSuccess) {
            for (int i = 0; i < ldpc_ctx::kSlots; i++) {
                (void)hipFree(ctx->d_in[i]); (void)hipFree(ctx->d_bits[i]); (void)hipFree(ctx->d_iters[i]); (void)hipFree(ctx->d_conv[i]);
                ctx->d_in[i] = nullptr; ctx->d_bits[i] = nullptr; ctx->d_iters[i] = nullptr; ctx->d_conv[i] = nullptr;
                if (i > 0 && ctx->pstream[i]) { (void)hipStreamDestroy(ctx->pstream[i]); ctx->pstream[i] = nullptr; }
            }
            if (ctx->decoded) { (void)hipEventDestroy(ctx->decoded); ctx->decoded = nullptr; }
            ctx->slots = 0;
            return set_error(LDPC_ENOMEM, "staging buffers for %d frames: %s", ctx->chunk, hipGetErrorString(e));
        }
    }
    if (want_final)
        for (int i = 0; i < ctx->slots; i++)
            if (!ctx->d_final[i]) HIPCHK(hipMalloc((void **)&ctx->d_final[i], (size_t)ctx->chunk * N * sizeof(double)));
    return LDPC_OK;
}

// device-visible address of page-locked host memory (hipHostMalloc / hipHostRegister), or nullptr for pageable memory
static void *pinned_device_ptr(const void *p) {
    if (!p) return nullptr;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (at.type != hipMemoryTypeHost || !at.devicePointer) return nullptr;
    return at.devicePointer;
}

// one chunk's decode on slot stream `st`, enqueued after its H2D copy: it starts when the previous chunk's decode (on the other
// slot's stream) has ended, so one context's decodes never run at once while copies still overlap them
static int decode_chunk(ldpc_ctx *ctx, hipStream_t st, int max_iters, int batch, const void *d_llr, int fmt, uint8_t *d_bits,
                        int32_t *d_iters, uint8_t *d_conv, double *d_final, double *d_trace) {
    if (ctx->decoded) {
        hipError_t e = hipStreamWaitEvent(st, ctx->decoded, 0);
        if (e != hipSuccess) return set_error(LDPC_EHIP, "hipStreamWaitEvent: %s", hipGetErrorString(e));
    }
    int rc = decode_dev(ctx, st, max_iters, batch, d_llr, fmt, d_bits, d_iters, d_conv, d_final, d_trace);
    if (rc == LDPC_OK && ctx->decoded) {
        hipError_t e = hipEventRecord(ctx->decoded, st);
        if (e != hipSuccess) return set_error(LDPC_EHIP, "hipEventRecord: %s", hipGetErrorString(e));
    }
    return rc;
}

static int decode_host(ldpc_ctx *ctx, int max_iters, int batch, const void *llr, int fmt, uint8_t *bits,
                       int32_t *iters, uint8_t *converged, double *final_lam, double *trace_lam) {
    int rc = check_call(ctx, max_iters, batch);
    if (rc == LDPC_OK) rc = check_format(ctx, fmt);
    if (rc != LDPC_OK) return rc;
    if (batch == 0) return LDPC_OK;
    if (!llr || !bits) return set_error(LDPC_EINVAL, "null llr/bits");
    // Zero-copy: with page-locked llr and bits (ldpc_host_alloc) and a kernel that reads every LLR once, the decode
    // kernel itself reads the LLRs and writes the bits over PCIe -- no staging copies, the transfer hides under the
    // compute of the other workgroups.  Measured (65 536 jpl.4096 frames, min-sum): f32 26.9 ms vs 57.9 ms through
    // the chunked copy pipeline, fp16 LLRs 24.6 vs 44.7 ms (copies issued next to the decode kernel did not overlap
    // with it on this platform: pipeline time = copy time + kernel time).
    if (!final_lam && !trace_lam && batch > ldpc_ctx::kSmallFrames && ctx->backend->reads_llr_once(max_iters)) {
        void *z_llr = pinned_device_ptr(llr), *z_bits = pinned_device_ptr(bits);
        if (z_llr && z_bits) {
            int32_t *z_it = (int32_t *)pinned_device_ptr(iters);
            uint8_t *z_cv = (uint8_t *)pinned_device_ptr(converged);
            if (iters && !z_it) {
                if (!ctx->d_zc_iters) HIPCHK(hipMalloc((void **)&ctx->d_zc_iters, sizeof(int32_t) * (size_t)ctx->max_batch));
                z_it = ctx->d_zc_iters;
            }
            if (converged && !z_cv) {
                if (!ctx->d_zc_conv) HIPCHK(hipMalloc((void **)&ctx->d_zc_conv, (size_t)ctx->max_batch));
                z_cv = ctx->d_zc_conv;
            }
            hipStream_t st = ctx->stream;
            rc = decode_dev(ctx, st, max_iters, batch, z_llr, fmt, (uint8_t *)z_bits, z_it, z_cv, nullptr, nullptr);
            hipError_t e = hipSuccess;
            if (rc == LDPC_OK && iters && z_it == ctx->d_zc_iters) e = hipMemcpyAsync(iters, z_it, sizeof(int32_t) * (size_t)batch, hipMemcpyDeviceToHost, st);
            if (rc == LDPC_OK && e == hipSuccess && converged && z_cv == ctx->d_zc_conv) e = hipMemcpyAsync(converged, z_cv, (size_t)batch, hipMemcpyDeviceToHost, st);
            hipError_t es2 = hipStreamSynchronize(st);
            if (e == hipSuccess) e = es2;
            if (rc == LDPC_OK && e != hipSuccess) rc = set_error(LDPC_EHIP, "decode (zero-copy): %s", hipGetErrorString(e));
            return rc;
        }
    }
    const size_t N = (size_t)ctx->code->N, es = llr_bytes(fmt);
    if (batch <= ldpc_ctx::kSmallFrames && !final_lam && !trace_lam) {   // latency path (allocates 16 frames, never the full-size staging)
        const size_t cap = (size_t)ldpc_ctx::kSmallFrames;
        const size_t out_cap = cap * N + cap * sizeof(int32_t) + cap + 16;
        if (!ctx->h_small_in) {
            hipError_t e = hipHostMalloc(&ctx->h_small_in, cap * N * sizeof(double), hipHostMallocDefault);
            if (e == hipSuccess) e = hipHostMalloc((void **)&ctx->h_small_out, out_cap, hipHostMallocDefault);
            if (e == hipSuccess) e = hipMalloc((void **)&ctx->d_small_out, out_cap);
            if (e == hipSuccess) e = hipMalloc(&ctx->d_small_in, cap * N * sizeof(double));
            if (e != hipSuccess) {
                if (ctx->h_small_in) (void)hipHostFree(ctx->h_small_in);
                if (ctx->h_small_out) (void)hipHostFree(ctx->h_small_out);
                (void)hipFree(ctx->d_small_out); (void)hipFree(ctx->d_small_in);
                ctx->h_small_in = nullptr; ctx->h_small_out = nullptr; ctx->d_small_out = nullptr; ctx->d_small_in = nullptr;
                return set_error(LDPC_ENOMEM, "latency-path buffers: %s", hipGetErrorString(e));
            }
        }
        const size_t nb = (size_t)batch, in_bytes = nb * N * es;
        const size_t off_it = (nb * N + 3) / 4 * 4, off_cv = off_it + nb * sizeof(int32_t), out_bytes = off_cv + nb;
        memcpy(ctx->h_small_in, llr, in_bytes);
        hipStream_t st = ctx->stream;
        hipError_t e = hipMemcpyAsync(ctx->d_small_in, ctx->h_small_in, in_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            rc = decode_dev(ctx, st, max_iters, batch, ctx->d_small_in, fmt, ctx->d_small_out, (int32_t *)(ctx->d_small_out + off_it),
                            ctx->d_small_out + off_cv, nullptr, nullptr);
            if (rc == LDPC_OK) e = hipMemcpyAsync(ctx->h_small_out, ctx->d_small_out, out_bytes, hipMemcpyDeviceToHost, st);
        }
        hipError_t es2 = hipStreamSynchronize(st);   // also after an error: nothing may still be in flight
        if (e == hipSuccess) e = es2;
        if (rc == LDPC_OK && e != hipSuccess) rc = set_error(LDPC_EHIP, "decode: %s", hipGetErrorString(e));
        if (rc != LDPC_OK) return rc;
        memcpy(bits, ctx->h_small_out, nb * N);
        if (iters) memcpy(iters, ctx->h_small_out + off_it, nb * sizeof(int32_t));
        if (converged) memcpy(converged, ctx->h_small_out + off_cv, nb);
        return LDPC_OK;
    }
    if ((rc = ensure_staging(ctx, final_lam != nullptr)) != LDPC_OK) return rc;
    double *d_trace = nullptr;
    const size_t turns = (size_t)max_iters + 1;
    if (trace_lam) {  // verification path: one device buffer for the whole batch
        size_t tb = (size_t)batch * turns * N * sizeof(double);
        hipError_t e = hipMalloc((void **)&d_trace, tb);
        if (e != hipSuccess) return set_error(LDPC_ENOMEM, "trace buffer of %zu bytes: %s", tb, hipGetErrorString(e));
        (void)hipMemsetAsync(d_trace, 0, tb, ctx->stream);
        (void)hipStreamSynchronize(ctx->stream);
    }
    hipError_t e = hipSuccess;
    int slot = 0;
    for (int f0 = 0; f0 < batch && rc == LDPC_OK && e == hipSuccess; f0 += ctx->chunk, slot = (slot + 1) % ctx->slots) {
        const int nb = std::min(ctx->chunk, batch - f0);
        hipStream_t st = ctx->pstream[slot];
        // stream order protects the slot: this copy is queued behind the slot's previous D2H
        e = hipMemcpyAsync(ctx->d_in[slot], (const char *)llr + (size_t)f0 * N * es, (size_t)nb * N * es, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) break;
        rc = decode_chunk(ctx, st, max_iters, nb, ctx->d_in[slot], fmt, ctx->d_bits[slot], ctx->d_iters[slot], ctx->d_conv[slot],
                          final_lam ? ctx->d_final[slot] : nullptr, d_trace ? d_trace + (size_t)f0 * turns * N : nullptr);
        if (rc != LDPC_OK) break;
        e = hipMemcpyAsync(bits + (size_t)f0 * N, ctx->d_bits[slot], (size_t)nb * N, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && iters) e = hipMemcpyAsync(iters + f0, ctx->d_iters[slot], sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && converged) e = hipMemcpyAsync(converged + f0, ctx->d_conv[slot], (size_t)nb, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && final_lam) e = hipMemcpyAsync(final_lam + (size_t)f0 * N, ctx->d_final[slot], (size_t)nb * N * sizeof(double), hipMemcpyDeviceToHost, st);
    }
    for (int i = 0; i < ctx->slots; i++) {   // every slot, also after an error: nothing may still be writing to the caller's buffers
        hipError_t es = hipStreamSynchronize(ctx->pstream[i]);
        if (e == hipSuccess) e = es;
    }
    if (rc == LDPC_OK && e == hipSuccess && trace_lam)
        e = hipMemcpy(trace_lam, d_trace, (size_t)batch * turns * N * sizeof(double), hipMemcpyDeviceToHost);
    if (rc == LDPC_OK && e != hipSuccess) rc = set_error(LDPC_EHIP, "decode: %s", hipGetErrorString(e));
    (void)hipFree(d_trace);
    return rc;
}

int ldpc_decode_batch(ldpc_ctx *ctx, int max_iters, int batch, const float *llr, uint8_t *bits, int32_t *iters,
                      uint8_t *converged) {
    return decode_host(ctx, max_iters, batch, llr, ldpc::LLR_F32, bits, iters, converged, nullptr, nullptr);
}

int ldpc_decode_batch_f16(ldpc_ctx *ctx, int max_iters, int batch, const uint16_t *llr, uint8_t *bits, int32_t *iters,
                          uint8_t *converged) {
    return decode_host(ctx, max_iters, batch, llr, ldpc::LLR_F16, bits, iters, converged, nullptr, nullptr);
}

int ldpc_decode_batch_f64(ldpc_ctx *ctx, int max_iters, int batch, const double *llr, uint8_t *bits, int32_t *iters,
                          uint8_t *converged, double *final_lam) {
    return decode_host(ctx, max_iters, batch, llr, ldpc::LLR_F64, bits, iters, converged, final_lam, nullptr);
}

int ldpc_decode_trace(ldpc_ctx *ctx, int max_iters, int batch, const double *llr, uint8_t *bits, int32_t *iters,
                      uint8_t *converged, double *trace_lam) {
    if (!trace_lam) return set_error(LDPC_EINVAL, "null trace_lam");
    return decode_host(ctx, max_iters, batch, llr, ldpc::LLR_F64, bits, iters, converged, nullptr, trace_lam);
}

int ldpc_decode_one(ldpc_ctx *ctx, int max_iters, const double *llr, uint8_t *bits, int *iters, int *converged) {
    int32_t it = 0;
    uint8_t cv = 0;
    int rc = decode_host(ctx, max_iters, 1, llr, ldpc::LLR_F64, bits, &it, &cv, nullptr, nullptr);
    if (rc != LDPC_OK) return rc;
    if (iters) *iters = it;
    if (converged) *converged = cv;
    return LDPC_OK;
}

static int decode_dev_checked(ldpc_ctx *ctx, int max_iters, int batch, const void *d_llr, int fmt, uint8_t *d_bits,
                              int32_t *d_iters, uint8_t *d_converged, void *stream) {
    int rc = check_call(ctx, max_iters, batch);
    if (rc == LDPC_OK) rc = check_format(ctx, fmt);
    if (rc != LDPC_OK) return rc;
    if (batch == 0) return LDPC_OK;
    if (!d_llr || !d_bits) return set_error(LDPC_EINVAL, "null d_llr/d_bits");
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    return decode_dev(ctx, st, max_iters, batch, d_llr, fmt, d_bits, d_iters, d_converged, nullptr, nullptr);
}

int ldpc_decode_batch_dev(ldpc_ctx *ctx, int max_iters, int batch, const float *d_llr, uint8_t *d_bits,
                          int32_t *d_iters, uint8_t *d_converged, void *stream) {
    return decode_dev_checked(ctx, max_iters, batch, d_llr, ldpc::LLR_F32, d_bits, d_iters, d_converged, stream);
}

int ldpc_decode_batch_dev_f16(ldpc_ctx *ctx, int max_iters, int batch, const uint16_t *d_llr, uint8_t *d_bits,
                              int32_t *d_iters, uint8_t *d_converged, void *stream) {
    return decode_dev_checked(ctx, max_iters, batch, d_llr, ldpc::LLR_F16, d_bits, d_iters, d_converged, stream);
}

int ldpc_decode_batch_i8(ldpc_ctx *ctx, int max_iters, int batch, const int8_t *llr, uint8_t *bits, int32_t *iters,
                         uint8_t *converged) {
    return decode_host(ctx, max_iters, batch, llr, ldpc::LLR_I8, bits, iters, converged, nullptr, nullptr);
}

int ldpc_decode_batch_dev_i8(ldpc_ctx *ctx, int max_iters, int batch, const int8_t *d_llr, uint8_t *d_bits,
                             int32_t *d_iters, uint8_t *d_converged, void *stream) {
    return decode_dev_checked(ctx, max_iters, batch, d_llr, ldpc::LLR_I8, d_bits, d_iters, d_converged, stream);
}

// the argument checks ldpc_decode_batch_dev_soft and ldpc_decode_batch_dev_continue share: the formats, the kind and the scale (*fmt: the
// kernels' format of llr_fmt), then -- for a call with frames -- the pointers, where d_soft may be null only if `soft_optional`
static int check_soft_formats(ldpc_ctx *ctx, int llr_fmt, int soft_fmt, float soft_qscale, int soft_kind, int *fmt) {
    if (llr_fmt != LDPC_LLR_F32 && llr_fmt != LDPC_LLR_F16 && llr_fmt != LDPC_LLR_I8) return set_error(LDPC_EINVAL, "llr_fmt %d is not one of LDPC_LLR_F32, LDPC_LLR_F16, LDPC_LLR_I8", llr_fmt);
    if (soft_fmt != LDPC_LLR_F32 && soft_fmt != LDPC_LLR_F16 && soft_fmt != LDPC_LLR_I8) return set_error(LDPC_EINVAL, "soft_fmt %d is not one of LDPC_LLR_F32, LDPC_LLR_F16, LDPC_LLR_I8", soft_fmt);
    if (soft_kind != LDPC_SOFT_POSTERIOR && soft_kind != LDPC_SOFT_EXTRINSIC) return set_error(LDPC_EINVAL, "soft_kind %d is neither LDPC_SOFT_POSTERIOR nor LDPC_SOFT_EXTRINSIC", soft_kind);
    *fmt = packed_format(llr_fmt);
    int rc = check_format(ctx, *fmt);
    if (rc != LDPC_OK) return rc;
    if (!(soft_qscale >= 0.f) || !std::isfinite(soft_qscale)) return set_error(LDPC_EINVAL, "soft_qscale %g is negative or not finite (0 = 4.0)", (double)soft_qscale);
    // an int8 cell's soft output in int8 is the cell's own integer: no other scale can be asked for
    if (ctx->dtype == LDPC_I8 && soft_fmt == LDPC_LLR_I8 && soft_qscale != 0.f && soft_qscale != ldpc_ctx_llr_qscale(ctx))
        return set_error(LDPC_EINVAL, "soft_qscale %g: the int8 soft output of an LDPC_I8 context has the context's scale %g (pass that, or 0)", (double)soft_qscale,
                         (double)ldpc_ctx_llr_qscale(ctx));
    return LDPC_OK;
}
static int check_soft_pointers(const void *d_llr, int fmt, const uint8_t *d_bits, const void *d_soft, int soft_fmt, bool soft_optional) {
    if (!d_llr || !d_bits) return set_error(LDPC_EINVAL, "null d_llr/d_bits");
    if (!d_soft && !soft_optional) return set_error(LDPC_EINVAL, "null d_soft");
    const size_t es = soft_fmt == LDPC_LLR_F32 ? 4 : soft_fmt == LDPC_LLR_F16 ? 2 : 1;
    if ((uintptr_t)d_soft % es) return set_error(LDPC_EINVAL, "d_soft is not aligned to its %zu-byte elements", es);
    if ((uintptr_t)d_llr % llr_bytes(fmt)) return set_error(LDPC_EINVAL, "d_llr is not aligned to its %zu-byte elements", llr_bytes(fmt));
    return LDPC_OK;
}

int ldpc_decode_batch_dev_soft(ldpc_ctx *ctx, int max_iters, int batch, const void *d_llr, int llr_fmt, uint8_t *d_bits, int32_t *d_iters,
                               uint8_t *d_converged, void *d_soft, int soft_fmt, float soft_qscale, int soft_kind, void *stream) {
    int rc = check_call(ctx, max_iters, batch), fmt = 0;
    if (rc != LDPC_OK) return rc;
    if ((rc = check_soft_formats(ctx, llr_fmt, soft_fmt, soft_qscale, soft_kind, &fmt)) != LDPC_OK) return rc;
    if (batch == 0) return LDPC_OK;
    if ((rc = check_soft_pointers(d_llr, fmt, d_bits, d_soft, soft_fmt, false)) != LDPC_OK) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    return ctx->backend->decode_soft(st, max_iters, batch, d_llr, fmt, d_bits, d_iters, d_converged, d_soft, soft_fmt, soft_qscale == 0.f ? 4.0f : soft_qscale, soft_kind);
}

// ---- a decode state: the check messages of `frames` frame slots, kept between calls (csrc/backend.h decode_state_bytes / decode_continue)
struct ldpc_decode_state {
    ldpc_ctx *ctx = nullptr;            // the context it was made for: its records are laid out in that context's geometry
    uint64_t ctx_serial = 0;            // ... and that context's serial: an address can be a later context's, a serial cannot
    int frames = 0, device = 0;
    size_t rec_bytes = 0, sum_bytes = 0;   // per slot
    void *rec = nullptr, *sum = nullptr;   // [frames] x each
};

ldpc_decode_state *ldpc_decode_state_create(ldpc_ctx *ctx, int max_frames) {
    if (!ctx) { set_error(LDPC_EINVAL, "null ctx"); return nullptr; }
    if (max_frames < 1) { set_error(LDPC_EINVAL, "max_frames %d < 1", max_frames); return nullptr; }
    size_t rb = 0, sb = 0;
    if (ctx->backend->decode_state_bytes(&rb, &sb) != LDPC_OK) return nullptr;
    HIPCHK_NULL(hipSetDevice(ctx->device));
    ldpc_decode_state *s = new (std::nothrow) ldpc_decode_state();
    if (!s) { set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    s->ctx = ctx; s->ctx_serial = ctx->serial; s->frames = max_frames; s->device = ctx->device; s->rec_bytes = rb; s->sum_bytes = sb;
    const size_t total = (rb + sb) * (size_t)max_frames;
    hipError_t e = hipMalloc(&s->rec, rb * (size_t)max_frames);
    if (e == hipSuccess) e = hipMalloc(&s->sum, sb * (size_t)max_frames);
    // all slots reset when this returns: the fills go to the context's own stream, where the decodes run by default, and are waited for
    if (e == hipSuccess) e = hipMemsetAsync(s->rec, 0, rb * (size_t)max_frames, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s->sum, 0, sb * (size_t)max_frames, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error(e == hipErrorOutOfMemory ? LDPC_ENOMEM : LDPC_EHIP, "ldpc_decode_state_create: %zu bytes of device memory for %d frames (%zu + %zu per frame): %s", total,
                  max_frames, rb, sb, hipGetErrorString(e));
        (void)hipFree(s->rec); (void)hipFree(s->sum);
        delete s;
        return nullptr;
    }
    return s;
}

void ldpc_decode_state_destroy(ldpc_decode_state *st) {
    if (!st) return;
    (void)hipSetDevice(st->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(st->rec); (void)hipFree(st->sum);
    delete st;
}

int ldpc_decode_state_frames(const ldpc_decode_state *st) { return st ? st->frames : set_error(LDPC_EINVAL, "null state"); }
size_t ldpc_decode_state_bytes(const ldpc_decode_state *st) { return st ? (st->rec_bytes + st->sum_bytes) * (size_t)st->frames : 0; }

static int check_state_range(const ldpc_decode_state *st, int first, int count) {
    if (!st) return set_error(LDPC_EINVAL, "null state");
    if (first < 0 || count < 0 || (long long)first + count > st->frames)
        return set_error(LDPC_EINVAL, "slots [%d, %d + %d) outside the state's %d frames", first, first, count, st->frames);
    return LDPC_OK;
}

int ldpc_decode_state_reset(ldpc_decode_state *st, int first, int count, void *stream) {
    int rc = check_state_range(st, first, count);
    if (rc != LDPC_OK) return rc;
    if (count == 0) return LDPC_OK;
    if (!stream && !ctx_alive(st->ctx_serial)) return set_error(LDPC_EINVAL, "the state's context was destroyed: no stream of its own to reset on (pass one)");
    HIPCHK(hipSetDevice(st->device));
    hipStream_t s = stream ? (hipStream_t)stream : st->ctx->stream;
    HIPCHK(hipMemsetAsync((char *)st->rec + st->rec_bytes * (size_t)first, 0, st->rec_bytes * (size_t)count, s));
    HIPCHK(hipMemsetAsync((char *)st->sum + st->sum_bytes * (size_t)first, 0, st->sum_bytes * (size_t)count, s));
    return LDPC_OK;
}

int ldpc_decode_batch_dev_continue(ldpc_ctx *ctx, ldpc_decode_state *state, int first, int max_iters, int batch, const void *d_llr, int llr_fmt,
                                   uint8_t *d_bits, int32_t *d_iters, uint8_t *d_converged, void *d_soft, int soft_fmt, float soft_qscale, int soft_kind,
                                   void *stream) {
    if (!ctx) return set_error(LDPC_EINVAL, "null ctx");
    size_t rb = 0, sb = 0;
    int rc = ctx->backend->decode_state_bytes(&rb, &sb), fmt = 0;      // (another kernel family: LDPC_EUNSUPPORTED with its name)
    if (rc != LDPC_OK) return rc;
    if (!state) return set_error(LDPC_EINVAL, "null state");
    if (state->ctx != ctx || state->ctx_serial != ctx->serial) return set_error(LDPC_EINVAL, "the state was made for another context (its records are laid out in that context's geometry)");
    if ((rc = check_state_range(state, first, batch)) != LDPC_OK) return rc;
    if ((rc = check_call(ctx, max_iters, batch)) != LDPC_OK) return rc;
    if ((rc = check_soft_formats(ctx, llr_fmt, soft_fmt, soft_qscale, soft_kind, &fmt)) != LDPC_OK) return rc;
    if (batch == 0) return LDPC_OK;
    if ((rc = check_soft_pointers(d_llr, fmt, d_bits, d_soft, soft_fmt, true)) != LDPC_OK) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    return ctx->backend->decode_continue(st, state->rec, state->sum, first, max_iters, batch, d_llr, fmt, d_bits, d_iters, d_converged, d_soft, soft_fmt,
                                         soft_qscale == 0.f ? 4.0f : soft_qscale, soft_kind);
}

// ---- a cascade: two contexts in a row, the frames the first does not converge on decoded again by the second (csrc/cascade.h)
struct ldpc_cascade {
    ldpc_ctx *ctx1 = nullptr, *ctx2 = nullptr;
    uint64_t serial1 = 0, serial2 = 0;   // the contexts' serials: a destroyed context is refused, not touched
    int capacity = 0, device = 0, N = 0;
    size_t bytes = 0;
    char *block = nullptr;               // one device allocation, cut into:
    void *llr2 = nullptr;                // [capacity][N] of up to 4-byte elements: the compact channel LLRs stage 2 decodes
    uint8_t *bits2 = nullptr;            // [capacity][N]
    int32_t *iters2 = nullptr;           // [capacity]
    uint8_t *conv2 = nullptr;            // [capacity]
    int32_t *idx = nullptr;              // [capacity]
    uint32_t *stats = nullptr;           // [3], when the caller passes none
    int32_t *iters1 = nullptr;           // [ctx1's max_batch], when the caller passes no d_iters
    uint8_t *conv1 = nullptr;            // [ctx1's max_batch], when the caller passes no d_converged
};

ldpc_cascade *ldpc_cascade_create(ldpc_ctx *ctx1, ldpc_ctx *ctx2, int capacity) {
    if (!ctx1 || !ctx2) { set_error(LDPC_EINVAL, "null %s", !ctx1 ? "ctx1" : "ctx2"); return nullptr; }
    if (ctx1->code->N != ctx2->code->N) { set_error(LDPC_EINVAL, "ctx1 decodes frames of N = %d, ctx2 of N = %d: not one code", ctx1->code->N, ctx2->code->N); return nullptr; }
    if (ctx1->device != ctx2->device) { set_error(LDPC_EINVAL, "ctx1 is on device %d, ctx2 on device %d", ctx1->device, ctx2->device); return nullptr; }
    if (capacity < 1 || capacity > ctx2->max_batch) { set_error(LDPC_EINVAL, "capacity %d outside [1,%d] (ctx2's max_batch)", capacity, ctx2->max_batch); return nullptr; }
    HIPCHK_NULL(hipSetDevice(ctx1->device));
    ldpc_cascade *c = new (std::nothrow) ldpc_cascade();
    if (!c) { set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    c->ctx1 = ctx1; c->ctx2 = ctx2; c->serial1 = ctx1->serial; c->serial2 = ctx2->serial;
    c->capacity = capacity; c->device = ctx1->device; c->N = ctx1->code->N;
    const size_t cap = (size_t)capacity, N = (size_t)c->N, mb = (size_t)ctx1->max_batch;
    const size_t part[8] = {cap * N * 4, cap * N, cap * 4, cap, cap * 4, 3 * sizeof(uint32_t), mb * 4, mb};
    size_t off[8], total = 0;
    for (int i = 0; i < 8; i++) { off[i] = total; total += (part[i] + 255) & ~(size_t)255; }
    hipError_t e = hipMalloc((void **)&c->block, total);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error(e == hipErrorOutOfMemory ? LDPC_ENOMEM : LDPC_EHIP, "ldpc_cascade_create: %zu bytes of device memory for capacity %d (N = %d, ctx1's max_batch %d): %s", total,
                  capacity, c->N, ctx1->max_batch, hipGetErrorString(e));
        delete c;
        return nullptr;
    }
    c->bytes = total;
    c->llr2 = c->block + off[0]; c->bits2 = (uint8_t *)(c->block + off[1]); c->iters2 = (int32_t *)(c->block + off[2]); c->conv2 = (uint8_t *)(c->block + off[3]);
    c->idx = (int32_t *)(c->block + off[4]); c->stats = (uint32_t *)(c->block + off[5]); c->iters1 = (int32_t *)(c->block + off[6]); c->conv1 = (uint8_t *)(c->block + off[7]);
    return c;
}

void ldpc_cascade_destroy(ldpc_cascade *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(c->block);
    delete c;
}

int ldpc_cascade_capacity(const ldpc_cascade *c) { return c ? c->capacity : set_error(LDPC_EINVAL, "null cascade"); }
size_t ldpc_cascade_bytes(const ldpc_cascade *c) { return c ? c->bytes : 0; }

int ldpc_cascade_decode_dev(ldpc_cascade *c, int max_iters1, int max_iters2, int batch, const void *d_llr, int llr_fmt, uint8_t *d_bits, int32_t *d_iters,
                            uint8_t *d_converged, uint8_t *d_stage, uint32_t *d_stats, void *stream) {
    if (!c) return set_error(LDPC_EINVAL, "null cascade");
    if (!ctx_alive(c->serial1) || !ctx_alive(c->serial2)) return set_error(LDPC_EINVAL, "%s of the cascade was destroyed", !ctx_alive(c->serial1) ? "ctx1" : "ctx2");
    ldpc_ctx *ctx1 = c->ctx1, *ctx2 = c->ctx2;
    if (max_iters1 < 0 || max_iters2 < 0) return set_error(LDPC_EINVAL, "%s %d < 0", max_iters1 < 0 ? "max_iters1" : "max_iters2", max_iters1 < 0 ? max_iters1 : max_iters2);
    if (batch < 0 || batch > ctx1->max_batch) return set_error(LDPC_EINVAL, "batch %d outside [0,%d] (ctx1's max_batch)", batch, ctx1->max_batch);
    if (llr_fmt != LDPC_LLR_F32 && llr_fmt != LDPC_LLR_F16 && llr_fmt != LDPC_LLR_I8) return set_error(LDPC_EINVAL, "llr_fmt %d is not one of LDPC_LLR_F32, LDPC_LLR_F16, LDPC_LLR_I8", llr_fmt);
    // both stages read the caller's format: refused here, so that no call stops between its stages
    if (llr_fmt == LDPC_LLR_I8 && (ctx1->dtype != LDPC_I8 || ctx2->dtype != LDPC_I8))
        return set_error(LDPC_EUNSUPPORTED, "llr_fmt LDPC_LLR_I8: int8 LLRs are accepted by LDPC_I8 contexts only (ctx1's dtype is %d, ctx2's is %d)", ctx1->dtype, ctx2->dtype);
    if (batch == 0) return LDPC_OK;
    if (!d_llr || !d_bits) return set_error(LDPC_EINVAL, "null %s", !d_llr ? "d_llr" : "d_bits");
    const int fmt = packed_format(llr_fmt), es = (int)llr_bytes(fmt);
    if ((uintptr_t)d_llr % (size_t)es) return set_error(LDPC_EINVAL, "d_llr is not aligned to its %d-byte elements", es);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx1->stream;
    int32_t *iters = d_iters ? d_iters : c->iters1;
    uint8_t *conv = d_converged ? d_converged : c->conv1;
    uint32_t *stats = d_stats ? d_stats : c->stats;
    int rc = decode_dev(ctx1, st, max_iters1, batch, d_llr, fmt, d_bits, iters, conv, nullptr, nullptr);
    if (rc == LDPC_OK) rc = ldpc::cascade_select_launch(st, batch, c->capacity, conv, c->idx, d_stage, stats);
    if (rc == LDPC_OK) rc = ldpc::cascade_gather_launch(st, c->N, es, c->capacity, d_llr, c->idx, stats, c->llr2);
    // stage 2 always decodes `capacity` rows: how many of them are frames is known on the device only
    if (rc == LDPC_OK) rc = decode_dev(ctx2, st, max_iters2, c->capacity, c->llr2, fmt, c->bits2, c->iters2, c->conv2, nullptr, nullptr);
    if (rc == LDPC_OK) rc = ldpc::cascade_scatter_launch(st, c->N, c->capacity, c->idx, c->bits2, c->iters2, c->conv2, d_bits, iters, conv, d_stage, stats);
    return rc;
}

int ldpc_decode_batch_dev_packed(ldpc_ctx *ctx, int max_iters, int batch, const void *d_llr, int llr_f16, uint8_t *d_packed, int32_t *d_iters,
                                 uint8_t *d_converged, void *stream) {
    int rc = check_call(ctx, max_iters, batch);
    if (rc == LDPC_OK) rc = check_format(ctx, packed_format(llr_f16));
    if (rc != LDPC_OK) return rc;
    if (batch == 0) return LDPC_OK;
    if (!d_llr || !d_packed) return set_error(LDPC_EINVAL, "null d_llr/d_packed");
    if (!ctx->d_unpacked) HIPCHK(hipMalloc((void **)&ctx->d_unpacked, (size_t)ctx->max_batch * ctx->code->N));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    rc = decode_dev(ctx, st, max_iters, batch, d_llr, packed_format(llr_f16), ctx->d_unpacked, d_iters, d_converged, nullptr, nullptr);
    if (rc != LDPC_OK) return rc;
    return ldpc::pack_bits(st, ctx->d_unpacked, d_packed, batch, ctx->code->N);
}

int ldpc_decode_batch_packed(ldpc_ctx *ctx, int max_iters, int batch, const void *llr, int llr_f16, uint8_t *packed, int32_t *iters, uint8_t *converged) {
    int rc = check_call(ctx, max_iters, batch);
    if (rc == LDPC_OK) rc = check_format(ctx, packed_format(llr_f16));
    if (rc != LDPC_OK) return rc;
    if (batch == 0) return LDPC_OK;
    if (!llr || !packed) return set_error(LDPC_EINVAL, "null llr/packed");
    const size_t N = (size_t)ctx->code->N, PB = (N + 7) / 8, es = llr_bytes(packed_format(llr_f16));
    if ((rc = ensure_staging(ctx, false)) != LDPC_OK) return rc;       // (d_in / d_iters / d_conv of the chunked pipeline; its d_bits slots are not used here)
    if (!ctx->d_packed) HIPCHK(hipMalloc((void **)&ctx->d_packed, (size_t)ctx->max_batch * PB));
    hipError_t e = hipSuccess;
    int slot = 0;
    // LLRs in chunk by chunk as the byte-per-bit entry point does; an eighth of the bytes back
    for (int f0 = 0; f0 < batch && rc == LDPC_OK && e == hipSuccess; f0 += ctx->chunk, slot = (slot + 1) % ctx->slots) {
        const int nb = std::min(ctx->chunk, batch - f0);
        hipStream_t st = ctx->pstream[slot];
        e = hipMemcpyAsync(ctx->d_in[slot], (const char *)llr + (size_t)f0 * N * es, (size_t)nb * N * es, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) break;
        rc = decode_chunk(ctx, st, max_iters, nb, ctx->d_in[slot], packed_format(llr_f16), ctx->d_bits[slot], ctx->d_iters[slot], ctx->d_conv[slot], nullptr, nullptr);
        if (rc == LDPC_OK) rc = ldpc::pack_bits(st, ctx->d_bits[slot], ctx->d_packed + (size_t)f0 * PB, nb, (int)N);
        if (rc != LDPC_OK) break;
        e = hipMemcpyAsync(packed + (size_t)f0 * PB, ctx->d_packed + (size_t)f0 * PB, (size_t)nb * PB, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && iters) e = hipMemcpyAsync(iters + f0, ctx->d_iters[slot], sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && converged) e = hipMemcpyAsync(converged + f0, ctx->d_conv[slot], (size_t)nb, hipMemcpyDeviceToHost, st);
    }
    for (int i = 0; i < ctx->slots; i++) {
        hipError_t es2 = hipStreamSynchronize(ctx->pstream[i]);
        if (e == hipSuccess) e = es2;
    }
    if (rc == LDPC_OK && e != hipSuccess) rc = set_error(LDPC_EHIP, "decode (packed): %s", hipGetErrorString(e));
    return rc;
}

int ldpc_debug_step(ldpc_ctx *ctx, int batch, const double *orig, const double *lam, const double *ne, double *ne_out,
                    double *lam_out, uint8_t *syndrome_zero) {
    int rc = check_call(ctx, 0, batch);
    if (rc != LDPC_OK) return rc;
    if (batch == 0) return LDPC_OK;
    if (!orig || !lam || !ne || !ne_out || !lam_out) return set_error(LDPC_EINVAL, "null argument");
    const size_t N = (size_t)ctx->code->N, E = (size_t)ctx->code->E, B = (size_t)batch;
    double *buf = nullptr;
    uint8_t *d_syn = nullptr;
    const size_t total = B * (3 * N + 2 * E);
    HIPCHK(hipMalloc((void **)&buf, total * sizeof(double)));
    if (hipMalloc((void **)&d_syn, B) != hipSuccess) { hipFree(buf); return set_error(LDPC_ENOMEM, "hipMalloc"); }
    double *d_orig = buf, *d_lam = buf + B * N, *d_lam_out = buf + 2 * B * N, *d_ne = buf + 3 * B * N, *d_ne_out = d_ne + B * E;
    hipStream_t st = ctx->stream;
    hipError_t ce = hipMemcpyAsync(d_orig, orig, B * N * 8, hipMemcpyHostToDevice, st);
    if (ce == hipSuccess) ce = hipMemcpyAsync(d_lam, lam, B * N * 8, hipMemcpyHostToDevice, st);
    if (ce == hipSuccess) ce = hipMemcpyAsync(d_ne, ne, B * E * 8, hipMemcpyHostToDevice, st);
    if (ce != hipSuccess) rc = set_error(LDPC_EHIP, "debug_step upload: %s", hipGetErrorString(ce));
    else rc = ctx->backend->step(st, batch, d_orig, d_lam, d_ne, d_ne_out, d_lam_out, d_syn);
    if (rc == LDPC_OK) {
        ce = hipMemcpyAsync(ne_out, d_ne_out, B * E * 8, hipMemcpyDeviceToHost, st);
        if (ce == hipSuccess) ce = hipMemcpyAsync(lam_out, d_lam_out, B * N * 8, hipMemcpyDeviceToHost, st);
        if (ce == hipSuccess && syndrome_zero) ce = hipMemcpyAsync(syndrome_zero, d_syn, B, hipMemcpyDeviceToHost, st);
        if (ce != hipSuccess) rc = set_error(LDPC_EHIP, "debug_step download: %s", hipGetErrorString(ce));
    }
    hipError_t e = hipStreamSynchronize(st);
    if (rc == LDPC_OK && e != hipSuccess) rc = set_error(LDPC_EHIP, "debug_step: %s", hipGetErrorString(e));
    hipFree(buf);
    hipFree(d_syn);
    return rc;
}


// ------------------------------------------------------------------------------- timing
int ldpc_ctx_set_timing(ldpc_ctx *ctx, int enabled) {
    if (!ctx) return set_error(LDPC_EINVAL, "null ctx");
    ctx->timer.enabled = enabled != 0;
    ctx->timer.used = 0;
    return LDPC_OK;
}

int ldpc_ctx_kernel_time(ldpc_ctx *ctx, int *launches, double *total_ms) {
    if (!ctx) return set_error(LDPC_EINVAL, "null ctx");
    if (ctx->timer.drain(launches, total_ms) != 0) return set_error(LDPC_EHIP, "event query failed");
    return LDPC_OK;
}

const char *ldpc_ctx_kernel_name(const ldpc_ctx *ctx) {
    return ctx ? ctx->backend->kernel_name() : "";
}

int ldpc_ctx_kernel_geometry(const ldpc_ctx *ctx, int *threads_per_workgroup, int *frames_per_workgroup) {
    if (!ctx) return set_error(LDPC_EINVAL, "null ctx");
    const ldpc::LaunchInfo &li = ctx->backend->info;
    if (threads_per_workgroup) *threads_per_workgroup = li.threads;
    if (frames_per_workgroup) *frames_per_workgroup = li.frames_per_wg;
    return LDPC_OK;
}

// ------------------------------------------------------------------------------- run-time specialised kernels
const char *ldpc_jit_cache_dir(void) { return ldpc::jit_cache_dir(); }

long ldpc_jit_source_for(const ldpc_code *code, int variant, int dtype, int schedule, char *buf, size_t cap) {
    if (!code) return set_error(LDPC_EINVAL, "null code");
    if (schedule != LDPC_SCHED_FLOODING && schedule != LDPC_SCHED_LAYERED) return set_error(LDPC_EINVAL, "unknown schedule %d", schedule);
    try {
        const int kind = ldpc::jit_kind_of(dtype, schedule);
        const char *why = ldpc::jit_split_why_not(*code, variant, dtype, kind);
        if (why) return set_error(LDPC_EUNSUPPORTED, "%s", why);
        const std::string src = ldpc::jit_split_source(*code, variant, dtype, nullptr, kind);
        if (buf && cap) { size_t n = std::min(cap - 1, src.size()); memcpy(buf, src.data(), n); buf[n] = 0; }
        return (long)src.size();
    } catch (...) { return set_error(LDPC_ENOMEM, "out of host memory"); }
}

int ldpc_jit_prepare_for(const ldpc_code *code, int variant, int dtype, int schedule, char *kernel_name, size_t cap, int *from_cache, double *seconds) {
    if (!code) return set_error(LDPC_EINVAL, "null code");
    if (schedule != LDPC_SCHED_FLOODING && schedule != LDPC_SCHED_LAYERED) return set_error(LDPC_EINVAL, "unknown schedule %d", schedule);
    try {
        const int kind = ldpc::jit_kind_of(dtype, schedule);
        const char *why = ldpc::jit_split_why_not(*code, variant, dtype, kind);
        if (why) return set_error(LDPC_EUNSUPPORTED, "%s", why);
        ldpc::JitKernel g;
        const std::string src = ldpc::jit_split_source(*code, variant, dtype, &g, kind);
        std::vector<char> co;
        bool fc = false;
        double sec = 0;
        int rc = ldpc::jit_compile_cached(src, g.name, co, &fc, &sec);
        if (rc != LDPC_OK) return rc;
        if (kernel_name && cap) snprintf(kernel_name, cap, "%s", g.name.c_str());
        if (from_cache) *from_cache = fc ? 1 : 0;
        if (seconds) *seconds = sec;
        return LDPC_OK;
    } catch (...) { return set_error(LDPC_ENOMEM, "out of host memory"); }
}

long ldpc_jit_source(const ldpc_code *code, int variant, int dtype, char *buf, size_t cap) {
    return ldpc_jit_source_for(code, variant, dtype, LDPC_SCHED_FLOODING, buf, cap);
}
int ldpc_jit_prepare(const ldpc_code *code, int variant, int dtype, char *kernel_name, size_t cap, int *from_cache, double *seconds) {
    return ldpc_jit_prepare_for(code, variant, dtype, LDPC_SCHED_FLOODING, kernel_name, cap, from_cache, seconds);
}

// ------------------------------------------------------------------------------- frame source
}  // extern "C"
struct ldpc_sim {
    ldpc::SimDev dev{};
    int p = 0, max_batch = 0, device = 0;
    std::vector<uint32_t> gt_host;     // dense generator, packed columns (host encode)
    std::vector<uint32_t> qc_host;     // quasi-cyclic generator: [brows][bcols][W] first-row words
    uint32_t *d_gt = nullptr, *d_msgw = nullptr, *d_rot = nullptr, *d_parw = nullptr;
    // encoder from H: row order[j] of H without its last column K + j, as [sp_ptr[j], sp_ptr[j+1]) of sp_col (host encode);
    // the device tables of sim_sparse.hip in one allocation, and its bit-sliced scratch
    bool sparse = false;
    ldpc::SimSparse sp{};
    std::vector<int32_t> sp_ptr, sp_col;
    int32_t *d_sp = nullptr;
    uint32_t *d_x = nullptr;
    // systematic form of any H (csrc/systematic.cc, csrc/sim_systematic.hip): positions and P (host encode), the window generator and
    // msg_pos on the device; d_parw holds the packed codewords
    bool systematic = false;
    ldpc::SimSys sy{};
    ldpc::SystematicForm sf;
    uint32_t *d_gwin = nullptr;
    int32_t *d_msg_pos = nullptr;
    // dense source, packed codewords (ldpc_sim_encode_messages): codeword bytes [max_batch][n_tx] for pack_bits, allocated on first use
    uint8_t *d_stage = nullptr;
    // modulated path (ldpc_sim_transmit, ldpc_sim_generate_mod): packed codewords [max_batch][ceil(n_tx / 8)], allocated on first use
    uint8_t *d_cw = nullptr;
};
extern "C" {

void ldpc_sim_destroy(ldpc_sim *sim) {
    if (!sim) return;
    (void)hipSetDevice(sim->device);
    hipFree(sim->d_gt);
    hipFree(sim->d_rot);
    hipFree(sim->d_parw);
    hipFree(sim->d_msgw);
    hipFree(sim->d_sp);
    hipFree(sim->d_x);
    hipFree(sim->d_gwin);
    hipFree(sim->d_msg_pos);
    hipFree(sim->d_stage);
    hipFree(sim->d_cw);
    delete sim;
}

ldpc_sim *ldpc_sim_create(const ldpc_code *code, int k, int n_tx, int p, const uint8_t *G, int max_batch) {
    const int device = current_device();
    if (device < 0) { set_error(LDPC_ENODEVICE, "ldpc_init() has not succeeded"); return nullptr; }
    return ldpc_sim_create_on(code, device, k, n_tx, p, G, max_batch);
}

static ldpc_sim *sim_new(const ldpc_code *code, int device, int k, int n_tx, int max_batch) {
    if (check_device(device) != LDPC_OK) return nullptr;
    ldpc_sim *s = new (std::nothrow) ldpc_sim();
    if (!s) { set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    s->device = device; s->max_batch = max_batch;
    s->dev.N = code->N; s->dev.k = k; s->dev.n_tx = n_tx; s->dev.kwords = (k + 31) / 32; s->dev.gt = nullptr; s->dev.qc_rot = nullptr;
    return s;
}

ldpc_sim *ldpc_sim_create_on(const ldpc_code *code, int device, int k, int n_tx, int p, const uint8_t *G, int max_batch) {
    if (!code || k <= 0 || n_tx < k || n_tx > code->N || max_batch <= 0 || (G && (p <= 0 || k + p < n_tx))) {
        set_error(LDPC_EINVAL, "ldpc_sim_create: bad arguments (k=%d n_tx=%d p=%d N=%d)", k, n_tx, p, code ? code->N : -1);
        return nullptr;
    }
    ldpc_sim *s = sim_new(code, device, k, n_tx, max_batch);
    if (!s) return nullptr;
    s->p = G ? p : 0;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess && G) {
        s->gt_host.assign((size_t)p * s->dev.kwords, 0u);
        for (int r = 0; r < k; r++)
            for (int j = 0; j < p; j++)
                if (G[(size_t)r * p + j]) s->gt_host[(size_t)j * s->dev.kwords + (r >> 5)] |= 1u << (r & 31);
        // device copy transposed and padded: [kwords][pp], parity position fastest, so that the lanes of a wave
        // (consecutive parity positions, four per lane) read consecutive words
        const int pp = (p + 3) / 4 * 4;
        std::vector<uint32_t> gtt((size_t)s->dev.kwords * pp, 0u);
        for (int j = 0; j < p; j++)
            for (int w = 0; w < s->dev.kwords; w++) gtt[(size_t)w * pp + j] = s->gt_host[(size_t)j * s->dev.kwords + w];
        e = hipMalloc((void **)&s->d_gt, gtt.size() * 4);
        if (e == hipSuccess) e = hipMemcpy(s->d_gt, gtt.data(), gtt.size() * 4, hipMemcpyHostToDevice);
        s->dev.gt = s->d_gt;
        s->dev.pp = pp;
    }
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_msgw, (size_t)max_batch * s->dev.kwords * 4);
    if (e != hipSuccess) { set_error(LDPC_EHIP, "ldpc_sim_create: %s", hipGetErrorString(e)); ldpc_sim_destroy(s); return nullptr; }
    return s;
}

// The generator in the reference's quasi-cyclic form (Fast/Encoder.hs:26-40: sz in {32, 64, 128, 256}, one machine word
// of sz bits per circulant = the integer of the .q file, bit b = first-row entry of column b).
ldpc_sim *ldpc_sim_create_qc_on(const ldpc_code *code, int device, int k, int n_tx, int sz, int block_rows, int block_cols,
                                const uint32_t *circ, int max_batch) {
    if (!code || !circ || sz <= 0 || block_rows <= 0 || block_cols <= 0 || max_batch <= 0 || k != sz * block_rows || n_tx < k || n_tx > code->N ||
        (long)k + (long)sz * block_cols < n_tx) {
        set_error(LDPC_EINVAL, "ldpc_sim_create_qc: bad arguments (k=%d n_tx=%d sz=%d blocks %dx%d N=%d)", k, n_tx, sz, block_rows, block_cols, code ? code->N : -1);
        return nullptr;
    }
    if (sz != 32 && sz != 64 && sz != 128 && sz != 256) {   // Fast/Encoder.hs:33 "unsupported size for fast encoder"
        set_error(LDPC_EUNSUPPORTED, "unsupported size for fast encoder : %d (32, 64, 128, 256; give the dense generator to ldpc_sim_create instead)", sz);
        return nullptr;
    }
    ldpc_sim *s = sim_new(code, device, k, n_tx, max_batch);
    if (!s) return nullptr;
    const int W = sz / 32, CB = 16 / W, ncg = (block_cols + CB - 1) / CB;
    s->p = sz * block_cols;
    s->qc_host.assign(circ, circ + (size_t)block_rows * block_cols * W);
    s->dev.qc_w = W; s->dev.qc_brows = block_rows; s->dev.qc_bcols = block_cols; s->dev.qc_ncg = ncg; s->dev.pwords = block_cols * W;
    // rot[cg][r][b][c in group][w] = word w of rotateL(g[r][c], b)
    std::vector<uint32_t> rot((size_t)ncg * block_rows * 32 * 16, 0u);
    for (int bc = 0; bc < block_cols; bc++)
        for (int r = 0; r < block_rows; r++) {
            const uint32_t *g = &circ[((size_t)r * block_cols + bc) * W];
            for (int b = 0; b < 32; b++)
                for (int w = 0; w < W; w++) {
                    const uint32_t lo = g[w], hi = g[(w + W - 1) % W];
                    rot[(((size_t)(bc / CB) * block_rows + r) * 32 + b) * 16 + (bc % CB) * W + w] = b ? ((lo << b) | (hi >> (32 - b))) : lo;
                }
        }
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_rot, rot.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(s->d_rot, rot.data(), rot.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_parw, (size_t)max_batch * s->dev.pwords * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_msgw, (size_t)max_batch * s->dev.kwords * 4);
    s->dev.qc_rot = s->d_rot;
    if (e != hipSuccess) { set_error(LDPC_EHIP, "ldpc_sim_create_qc: %s", hipGetErrorString(e)); ldpc_sim_destroy(s); return nullptr; }
    return s;
}

// The encoder from H (csrc/sim_sparse.hip).  Scratch: 4 N min(ceil(max_batch / 32), kSparseFwCap) bytes; a larger batch goes
// through it in chunks of 32 * kSparseFwCap frames.
static const int kSparseFwCap = 512;
ldpc_sim *ldpc_sim_create_sparse_on(const ldpc_code *code, int device, int n_tx, int max_batch) {
    if (!code || max_batch <= 0) {
        set_error(LDPC_EINVAL, "ldpc_sim_create_sparse: bad arguments (n_tx=%d max_batch=%d N=%d)", n_tx, max_batch, code ? code->N : -1);
        return nullptr;
    }
    const int M = code->M, N = code->N, K = N - M;
    std::vector<int32_t> order((size_t)M);
    if (triangular_order("ldpc_sim_create_sparse", M, N, code->row_ptr.data(), code->col_idx.data(), order.data()) != LDPC_OK) return nullptr;
    if (n_tx < K || n_tx > N) {
        set_error(LDPC_EINVAL, "ldpc_sim_create_sparse: bad arguments (k=%d n_tx=%d N=%d)", K, n_tx, N);
        return nullptr;
    }
    ldpc_sim *s = sim_new(code, device, K, n_tx, max_batch);
    if (!s) return nullptr;
    s->p = M;
    s->sparse = true;
    s->dev.pwords = (M + 31) / 32;
    // device tables, one allocation: a_ptr [M+1] | b_meta [M+1] | a_col [na] | b_far [nb]
    std::vector<int32_t> a_ptr((size_t)M + 1, 0), b_meta((size_t)M + 1, 0), a_col, b_far;
    s->sp_ptr.assign((size_t)M + 1, 0);
    for (int j = 0; j < M; j++) {
        const int m = order[j];
        bool prev = false;
        for (int q = code->row_ptr[m]; q < code->row_ptr[m + 1] - 1; q++) {   // (the last column is K + j itself)
            const int c = code->col_idx[q];
            s->sp_col.push_back(c);
            if (c < K) a_col.push_back(c);
            else if (c == K + j - 1) prev = true;
            else b_far.push_back(c - K);
        }
        s->sp_ptr[j + 1] = (int32_t)s->sp_col.size();
        a_ptr[j + 1] = (int32_t)a_col.size();
        b_meta[j] |= prev ? (int32_t)0x80000000u : 0;
        b_meta[j + 1] = (int32_t)b_far.size();
    }
    std::vector<int32_t> tab;
    tab.insert(tab.end(), a_ptr.begin(), a_ptr.end());
    tab.insert(tab.end(), b_meta.begin(), b_meta.end());
    tab.insert(tab.end(), a_col.begin(), a_col.end());
    tab.insert(tab.end(), b_far.begin(), b_far.end());
    const int fw_cap = std::min((max_batch + 31) / 32, kSparseFwCap);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_sp, tab.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(s->d_sp, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_x, (size_t)N * fw_cap * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_parw, (size_t)max_batch * s->dev.pwords * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_msgw, (size_t)max_batch * s->dev.kwords * 4);
    if (e != hipSuccess) { set_error(LDPC_EHIP, "ldpc_sim_create_sparse: %s", hipGetErrorString(e)); ldpc_sim_destroy(s); return nullptr; }
    s->sp.M = M; s->sp.K = K; s->sp.x = s->d_x; s->sp.fw_cap = fw_cap;
    s->sp.a_ptr = s->d_sp; s->sp.b_meta = s->d_sp + (M + 1);
    s->sp.a_col = s->d_sp + 2 * (size_t)(M + 1); s->sp.b_far = s->sp.a_col + a_col.size();
    return s;
}

// The encoder from any H (csrc/sim_systematic.hip).  Device memory: the window generator, 64 * 32 * ceil(K / 32) bytes per 512
// codeword positions from the first parity position on, and 4 * ceil(N / 32) * max_batch bytes of packed codewords.
ldpc_sim *ldpc_sim_create_systematic_on(const ldpc_code *code, int device, int n_tx, int max_batch) {
    if (!code || max_batch <= 0) {
        set_error(LDPC_EINVAL, "ldpc_sim_create_systematic: bad arguments (n_tx=%d max_batch=%d N=%d)", n_tx, max_batch, code ? code->N : -1);
        return nullptr;
    }
    const int N = code->N;
    ldpc::SystematicForm sf;
    std::string err;
    const int rc = ldpc::systematic_form("ldpc_sim_create_systematic", code->M, N, code->row_ptr.data(), code->col_idx.data(), sf, err);
    if (rc != LDPC_OK) { set_error(rc, "%s", err.c_str()); return nullptr; }
    const int K = sf.K, r = sf.rank;
    if (n_tx < K || n_tx > N) {
        set_error(LDPC_EINVAL, "ldpc_sim_create_systematic: bad arguments (k=%d n_tx=%d N=%d)", K, n_tx, N);
        return nullptr;
    }
    ldpc_sim *s = sim_new(code, device, K, n_tx, max_batch);
    if (!s) return nullptr;
    s->p = r;
    s->systematic = true;
    const int kwords = s->dev.kwords, cww = (N + 31) / 32;
    const int w0 = std::min(r ? sf.par_pos[0] / 32 : cww - 1, cww - 1), ncg = (cww - w0 + 15) / 16;
    s->dev.pwords = cww;
    // gwin[cg][i][c]: word w0 + 16 cg + c of the codeword of the unit message e_i
    std::vector<uint32_t> gwin((size_t)ncg * kwords * 32 * 16, 0u);
    auto put = [&](int i, int n) {
        const int w = n / 32 - w0;
        if (w >= 0) gwin[((size_t)(w / 16) * kwords * 32 + i) * 16 + w % 16] |= 1u << (n & 31);
    };
    for (int i = 0; i < K; i++) {
        put(i, sf.msg_pos[i]);
        for (int j = 0; j < r; j++)
            if ((sf.P[(size_t)i * sf.pw64 + (j >> 6)] >> (j & 63)) & 1ull) put(i, sf.par_pos[j]);
    }
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_gwin, gwin.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(s->d_gwin, gwin.data(), gwin.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_msg_pos, (size_t)K * 4);
    if (e == hipSuccess) e = hipMemcpy(s->d_msg_pos, sf.msg_pos.data(), (size_t)K * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_parw, (size_t)max_batch * cww * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_msgw, (size_t)max_batch * kwords * 4);
    if (e != hipSuccess) { set_error(LDPC_EHIP, "ldpc_sim_create_systematic: %s", hipGetErrorString(e)); ldpc_sim_destroy(s); return nullptr; }
    s->sy.gwin = s->d_gwin; s->sy.ncg = ncg; s->sy.w0 = w0; s->sy.cww = cww; s->sy.msg_pos = s->d_msg_pos;
    s->sf = std::move(sf);
    return s;
}

int ldpc_sim_message_length(const ldpc_sim *sim) {
    if (!sim) return set_error(LDPC_EINVAL, "null sim");
    return sim->dev.k;
}

int ldpc_sim_positions(const ldpc_sim *sim, int32_t *msg_pos, int32_t *par_pos) {
    if (!sim) return set_error(LDPC_EINVAL, "null sim");
    const int k = sim->dev.k, np = sim->systematic ? sim->p : std::max(0, std::min(sim->p, sim->dev.N - k));
    for (int i = 0; msg_pos && i < k; i++) msg_pos[i] = sim->systematic ? sim->sf.msg_pos[i] : i;
    for (int j = 0; par_pos && j < np; j++) par_pos[j] = sim->systematic ? sim->sf.par_pos[j] : k + j;
    return np;
}

int ldpc_sim_encoder(const ldpc_sim *sim) {
    if (!sim) return set_error(LDPC_EINVAL, "null sim");
    if (sim->systematic) return LDPC_ENCODER_SYSTEMATIC;
    if (sim->sparse) return LDPC_ENCODER_SPARSE;
    return sim->dev.qc_rot ? LDPC_ENCODER_QC : (sim->dev.gt ? LDPC_ENCODER_DENSE : LDPC_ENCODER_NONE);
}

static int sim_generate_any(ldpc_sim *sim, uint64_t seed, uint64_t first_frame, int batch, double ebn0_db, void *d_out,
                            int out_fmt, uint8_t *d_msg, void *stream) {
    if (!sim || !d_out || batch < 0 || batch > sim->max_batch) return set_error(LDPC_EINVAL, "ldpc_sim_generate: bad arguments");
    if (batch == 0) return LDPC_OK;
    HIPCHK(hipSetDevice(sim->device));
    return ldpc::sim_generate(sim->dev, sim->sparse ? &sim->sp : nullptr, sim->systematic ? &sim->sy : nullptr, sim->d_msgw, sim->d_parw, (hipStream_t)stream, seed, first_frame, batch, ebn0_db, d_out, out_fmt, d_msg);
}

int ldpc_sim_generate(ldpc_sim *sim, uint64_t seed, uint64_t first_frame, int batch, double ebn0_db, float *d_llr,
                      uint8_t *d_msg, void *stream) {
    return sim_generate_any(sim, seed, first_frame, batch, ebn0_db, d_llr, 0, d_msg, stream);
}

int ldpc_sim_generate_f16(ldpc_sim *sim, uint64_t seed, uint64_t first_frame, int batch, double ebn0_db, uint16_t *d_llr,
                          uint8_t *d_msg, void *stream) {
    return sim_generate_any(sim, seed, first_frame, batch, ebn0_db, d_llr, 1, d_msg, stream);
}

int ldpc_sim_encode_batch(ldpc_sim *sim, uint64_t seed, uint64_t first_frame, int batch, uint8_t *d_codewords, uint8_t *d_msg, void *stream) {
    return sim_generate_any(sim, seed, first_frame, batch, 0.0, d_codewords, 2, d_msg, stream);
}

// caller-supplied messages: the checks the three entry points share, then the message words
static int sim_check_messages(const char *what, const ldpc_sim *sim, int batch, const void *a, const void *b, int fmt_a, int fmt_b, bool encodes) {
    if (!sim || !a || !b) return set_error(LDPC_EINVAL, "%s: null argument", what);
    if (batch <= 0 || batch > sim->max_batch) return set_error(LDPC_EINVAL, "%s: batch %d outside 1..%d", what, batch, sim->max_batch);
    if ((fmt_a != LDPC_BITS_BYTES && fmt_a != LDPC_BITS_PACKED) || (fmt_b != LDPC_BITS_BYTES && fmt_b != LDPC_BITS_PACKED))
        return set_error(LDPC_EINVAL, "%s: unknown bit format (LDPC_BITS_BYTES = 0, LDPC_BITS_PACKED = 1)", what);
    if (encodes && ldpc_sim_encoder(sim) == LDPC_ENCODER_NONE)
        return set_error(LDPC_EUNSUPPORTED, "%s: this frame source has no encoder (msg ++ zeros is not a codeword); create it with a generator or from H", what);
    return LDPC_OK;
}

static int sim_load(const char *what, ldpc_sim *sim, int batch, const void *d_msg, int msg_fmt, void *stream) {
    if (msg_fmt == LDPC_BITS_PACKED && (uintptr_t)d_msg % 4 != 0) return set_error(LDPC_EINVAL, "%s: packed message rows must be 4-byte aligned", what);
    return ldpc::sim_load_messages((hipStream_t)stream, d_msg, msg_fmt, sim->d_msgw, sim->dev.kwords, sim->dev.k, batch);
}

int ldpc_sim_encode_messages(ldpc_sim *sim, int batch, const void *d_msg, int msg_fmt, void *d_codewords, int cw_fmt, void *stream) {
    int rc = sim_check_messages("ldpc_sim_encode_messages", sim, batch, d_msg, d_codewords, msg_fmt, cw_fmt, true);
    if (rc != LDPC_OK) return rc;
    HIPCHK(hipSetDevice(sim->device));
    hipStream_t st = (hipStream_t)stream;
    if ((rc = sim_load("ldpc_sim_encode_messages", sim, batch, d_msg, msg_fmt, stream)) != LDPC_OK) return rc;
    const ldpc::SimSparse *sp = sim->sparse ? &sim->sp : nullptr;
    const ldpc::SimSys *sy = sim->systematic ? &sim->sy : nullptr;
    if (cw_fmt == LDPC_BITS_BYTES || sim->d_parw)
        return ldpc::sim_generate(sim->dev, sp, sy, sim->d_msgw, sim->d_parw, st, 0, 0, batch, 0.0, d_codewords, cw_fmt == LDPC_BITS_BYTES ? 2 : 3, nullptr, true);
    // dense generator: the product lives inside the frame kernel, which writes bytes; pack those
    if (!sim->d_stage) {
        hipError_t e = hipMalloc((void **)&sim->d_stage, (size_t)sim->max_batch * sim->dev.n_tx);
        if (e != hipSuccess) { sim->d_stage = nullptr; return set_error(LDPC_EHIP, "ldpc_sim_encode_messages: staging buffer: %s", hipGetErrorString(e)); }
    }
    rc = ldpc::sim_generate(sim->dev, sp, sy, sim->d_msgw, sim->d_parw, st, 0, 0, batch, 0.0, sim->d_stage, 2, nullptr, true);
    if (rc != LDPC_OK) return rc;
    return ldpc::pack_bits(st, sim->d_stage, (uint8_t *)d_codewords, batch, sim->dev.n_tx);
}

int ldpc_sim_generate_from(ldpc_sim *sim, uint64_t seed, uint64_t first_frame, int batch, double ebn0_db, const void *d_msg, int msg_fmt, void *d_llr,
                           int llr_f16, void *stream) {
    int rc = sim_check_messages("ldpc_sim_generate_from", sim, batch, d_msg, d_llr, msg_fmt, LDPC_BITS_BYTES, true);
    if (rc != LDPC_OK) return rc;
    if (llr_f16 != 0 && llr_f16 != 1) return set_error(LDPC_EINVAL, "ldpc_sim_generate_from: llr_f16 must be 0 (float32) or 1 (fp16)");
    HIPCHK(hipSetDevice(sim->device));
    if ((rc = sim_load("ldpc_sim_generate_from", sim, batch, d_msg, msg_fmt, stream)) != LDPC_OK) return rc;
    return ldpc::sim_generate(sim->dev, sim->sparse ? &sim->sp : nullptr, sim->systematic ? &sim->sy : nullptr, sim->d_msgw, sim->d_parw, (hipStream_t)stream, seed,
                              first_frame, batch, ebn0_db, d_llr, llr_f16, nullptr, true);
}

// ---- higher-order modulation: the stand-alone demapper and the frame source's modulated path (csrc/demap.hip, csrc/sim_mod.hip)
static int check_llr_out(const char *what, int llr_fmt, float qscale) {
    if (llr_fmt != LDPC_LLR_F32 && llr_fmt != LDPC_LLR_F16 && llr_fmt != LDPC_LLR_I8)
        return set_error(LDPC_EINVAL, "%s: unknown LLR format %d (LDPC_LLR_F32 = 0, LDPC_LLR_F16 = 1, LDPC_LLR_I8 = 2)", what, llr_fmt);
    if (!(qscale >= 0.f) || !std::isfinite(qscale)) return set_error(LDPC_EINVAL, "%s: qscale must be finite and >= 0 (0 = 4.0)", what);
    return LDPC_OK;
}

static int llr_elem(int llr_fmt) { return llr_fmt == LDPC_LLR_F32 ? 4 : llr_fmt == LDPC_LLR_F16 ? 2 : 1; }

// what every demapper entry point checks after its null pointers, in the one order they all have: batch, accumulate (0 where there is
// none), noise_var, the output format, `misaligned` (the entry point's own complaint about its buffers, null if it has none), and
// 1 / (2 noise_var) as a float32.  Gives the kernels' two scales: inv, and qs = the int8 scale with its default
static int demap_args(const char *what, int batch, int accumulate, double noise_var, int llr_fmt, float qscale, const char *misaligned, float &inv, float &qs) {
    if (batch <= 0) return set_error(LDPC_EINVAL, "%s: bad dimensions (batch=%d)", what, batch);
    if (accumulate != 0 && accumulate != 1) return set_error(LDPC_EINVAL, "%s: accumulate must be 0 or 1", what);
    if (!(noise_var > 0.0) || !std::isfinite(noise_var)) return set_error(LDPC_EINVAL, "%s: noise_var must be finite and > 0", what);
    const int rc = check_llr_out(what, llr_fmt, qscale);
    if (rc != LDPC_OK) return rc;
    if (misaligned) return set_error(LDPC_EINVAL, "%s: %s", what, misaligned);
    inv = (float)(1.0 / (2.0 * noise_var));
    if (!std::isfinite(inv)) return set_error(LDPC_EINVAL, "%s: 1 / (2 noise_var) does not fit a float32 (noise_var %g)", what, noise_var);
    qs = qscale == 0.f ? 4.0f : qscale;
    return LDPC_OK;
}

int ldpc_demap_dev(const ldpc_modulation *mod, int batch, int n_tx, int N, const float *d_sym, double noise_var, void *d_llr, int llr_fmt, float qscale, void *stream) {
    if (!mod || !d_sym || !d_llr) return set_error(LDPC_EINVAL, "ldpc_demap_dev: null argument");
    if (batch <= 0 || n_tx <= 0 || n_tx > N) return set_error(LDPC_EINVAL, "ldpc_demap_dev: bad dimensions (batch=%d n_tx=%d N=%d)", batch, n_tx, N);
    const bool bad = (uintptr_t)d_sym % 8 != 0 || (uintptr_t)d_llr % llr_elem(llr_fmt) != 0;
    float inv, qs;
    const int rc = demap_args("ldpc_demap_dev", batch, 0, noise_var, llr_fmt, qscale, bad ? "samples must be 8-byte aligned and LLRs aligned to their element" : nullptr, inv, qs);
    if (rc != LDPC_OK) return rc;
    const int device = current_device();
    if (device < 0) return set_error(LDPC_ENODEVICE, "ldpc_init() has not succeeded");
    HIPCHK(hipSetDevice(device));
    if (mod->b) return ldpc::demap_product_launch((hipStream_t)stream, mod->ax, mod->b, mod->rule, batch, n_tx, N, d_sym, inv, d_llr, llr_fmt, qs);
    return ldpc::demap_launch((hipStream_t)stream, mod->tab, mod->m, mod->rule, batch, n_tx, N, d_sym, inv, d_llr, llr_fmt, qs);
}

double ldpc_sim_noise_var(const ldpc_sim *sim, const ldpc_modulation *mod, double ebn0_db) {
    if (!sim || !mod) { set_error(LDPC_EINVAL, "ldpc_sim_noise_var: null argument"); return 0.0; }
    const double R = (double)sim->dev.k / (double)sim->dev.n_tx;
    return mod->es / (2.0 * R * (double)mod->m * pow(10.0, ebn0_db / 10.0));
}

// the codewords of the batch, packed, in sim->d_cw: the drawn messages (d_msg_in null) or the caller's
static int sim_mod_codewords(const char *what, ldpc_sim *sim, uint64_t seed, uint64_t first_frame, int batch, const void *d_msg_in, int msg_fmt, uint8_t *d_msg, hipStream_t st) {
    const int n_tx = sim->dev.n_tx, PB = (n_tx + 7) / 8;
    if (!sim->d_cw) {
        hipError_t e = hipMalloc((void **)&sim->d_cw, (size_t)sim->max_batch * PB);
        if (e != hipSuccess) { sim->d_cw = nullptr; return set_error(LDPC_EHIP, "%s: codeword buffer: %s", what, hipGetErrorString(e)); }
    }
    int rc;
    if (d_msg_in && (rc = sim_load(what, sim, batch, d_msg_in, msg_fmt, st)) != LDPC_OK) return rc;
    const ldpc::SimSparse *sp = sim->sparse ? &sim->sp : nullptr;
    const ldpc::SimSys *sy = sim->systematic ? &sim->sy : nullptr;
    if (sim->d_parw) {   // quasi-cyclic, from H, systematic form: packed straight from the message and parity words
        rc = ldpc::sim_generate(sim->dev, sp, sy, sim->d_msgw, sim->d_parw, st, seed, first_frame, batch, 0.0, sim->d_cw, 3, d_msg, d_msg_in != nullptr);
        if (rc == LDPC_OK && d_msg && !sy) rc = ldpc::sim_systematic_msg_bytes(sim->d_msgw, sim->dev.kwords, sim->dev.k, d_msg, st, batch);   // (the message words unpacked)
        return rc;
    }
    // dense generator, or none (all-zero codewords): the frame kernel writes bytes; pack those
    if (!sim->d_stage) {
        hipError_t e = hipMalloc((void **)&sim->d_stage, (size_t)sim->max_batch * n_tx);
        if (e != hipSuccess) { sim->d_stage = nullptr; return set_error(LDPC_EHIP, "%s: staging buffer: %s", what, hipGetErrorString(e)); }
    }
    rc = ldpc::sim_generate(sim->dev, sp, sy, sim->d_msgw, sim->d_parw, st, seed, first_frame, batch, 0.0, sim->d_stage, 2, d_msg, d_msg_in != nullptr);
    if (rc != LDPC_OK) return rc;
    return ldpc::pack_bits(st, sim->d_stage, sim->d_cw, batch, n_tx);
}

// fused: the entry point's kernel maps, adds noise and demaps in one; those hold the max-log rule only (include/ldpc_hip.h, THE LLR RULE)
static int sim_mod_check(const char *what, const ldpc_sim *sim, const ldpc_modulation *mod, int batch, const void *d_msg_in, int msg_fmt, const void *d_out, bool fused = false) {
    if (!sim || !mod || !d_out) return set_error(LDPC_EINVAL, "%s: null argument", what);
    if (batch <= 0 || batch > sim->max_batch) return set_error(LDPC_EINVAL, "%s: batch %d outside 1..%d", what, batch, sim->max_batch);
    if (d_msg_in) {
        if (msg_fmt != LDPC_BITS_BYTES && msg_fmt != LDPC_BITS_PACKED) return set_error(LDPC_EINVAL, "%s: unknown bit format (LDPC_BITS_BYTES = 0, LDPC_BITS_PACKED = 1)", what);
        if (ldpc_sim_encoder(sim) == LDPC_ENCODER_NONE)
            return set_error(LDPC_EUNSUPPORTED, "%s: this frame source has no encoder (msg ++ zeros is not a codeword); create it with a generator or from H", what);
    }
    if (fused && mod->rule != LDPC_DEMAP_MAXLOG)
        return set_error(LDPC_EUNSUPPORTED, "%s: no fused kernel for the log-MAP rule (LDPC_DEMAP_LOGMAP); use ldpc_sim_transmit* and a demapper", what);
    return LDPC_OK;
}

// the output of a fused entry point: the format, then the alignment of d_llr and of the optional gain buffer
static int sim_mod_llr_out(const char *what, int llr_fmt, float qscale, const void *d_llr, const float *d_gain, bool has_gain, float &qs) {
    const int rc = check_llr_out(what, llr_fmt, qscale);
    if (rc != LDPC_OK) return rc;
    if ((uintptr_t)d_llr % llr_elem(llr_fmt) != 0 || (uintptr_t)d_gain % 4 != 0)
        return set_error(LDPC_EINVAL, has_gain ? "%s: LLRs must be aligned to their element, gains 4-byte aligned" : "%s: LLRs must be aligned to their element", what);
    qs = qscale == 0.f ? 4.0f : qscale;
    return LDPC_OK;
}

// what the launchers of the modulated path take beside the entry point's own buffers
struct SimModRun {
    hipStream_t st;
    int PB;          // bytes of a packed codeword row
    float sg, inv;   // float32(sigma); float32(1 / (2 sigma^2)), for the fused kernels
};

// the back of every entry point of the modulated path, once its arguments are checked: the noise variance nv (ldpc_sim_noise_var*)
// must be finite and >= 0, for a fused kernel (`fused`) > 0 with 1 / (2 nv) a float32; then the device, and the codewords into sim->d_cw
static int sim_mod_run(const char *what, ldpc_sim *sim, double nv, bool fused, uint64_t seed, uint64_t first_frame, int batch, double ebn0_db, const void *d_msg_in,
                       int msg_fmt, uint8_t *d_msg, void *stream, SimModRun &run) {
    if (!fused && (!(nv >= 0.0) || !std::isfinite(nv))) return set_error(LDPC_EINVAL, "%s: Eb/N0 gives no finite noise variance", what);
    if (fused && (!(nv > 0.0) || !std::isfinite(nv))) return set_error(LDPC_EINVAL, "%s: Eb/N0 gives no finite noise variance > 0", what);
    run.inv = (float)(1.0 / (2.0 * nv));
    if (fused && !std::isfinite(run.inv)) return set_error(LDPC_EINVAL, "%s: 1 / (2 sigma^2) does not fit a float32 at %g dB", what, ebn0_db);
    run.sg = (float)sqrt(nv);
    run.st = (hipStream_t)stream;
    run.PB = (sim->dev.n_tx + 7) / 8;
    HIPCHK(hipSetDevice(sim->device));
    return sim_mod_codewords(what, sim, seed, first_frame, batch, d_msg_in, msg_fmt, d_msg, run.st);
}

int ldpc_sim_transmit(ldpc_sim *sim, const ldpc_modulation *mod, uint64_t seed, uint64_t first_frame, int batch, double ebn0_db, const void *d_msg_in, int msg_fmt,
                      float *d_sym, uint8_t *d_msg, void *stream) {
    int rc = sim_mod_check("ldpc_sim_transmit", sim, mod, batch, d_msg_in, msg_fmt, d_sym);
    if (rc != LDPC_OK) return rc;
    if ((uintptr_t)d_sym % 8 != 0) return set_error(LDPC_EINVAL, "ldpc_sim_transmit: samples must be 8-byte aligned");
    SimModRun r;
    if ((rc = sim_mod_run("ldpc_sim_transmit", sim, ldpc_sim_noise_var(sim, mod, ebn0_db), false, seed, first_frame, batch, ebn0_db, d_msg_in, msg_fmt, d_msg, stream, r)) != LDPC_OK) return rc;
    if (mod->b) return ldpc::product_transmit_launch(r.st, mod->ax, mod->b, batch, sim->dev.n_tx, sim->d_cw, r.PB, seed, first_frame, r.sg, d_sym);
    return ldpc::mod_transmit_launch(r.st, mod->tab, mod->m, batch, sim->dev.n_tx, sim->d_cw, r.PB, seed, first_frame, r.sg, d_sym);
}

int ldpc_sim_generate_mod(ldpc_sim *sim, const ldpc_modulation *mod, uint64_t seed, uint64_t first_frame, int batch, double ebn0_db, const void *d_msg_in, int msg_fmt,
                          void *d_llr, int llr_fmt, float qscale, uint8_t *d_msg, void *stream) {
    int rc = sim_mod_check("ldpc_sim_generate_mod", sim, mod, batch, d_msg_in, msg_fmt, d_llr, true);
    if (rc != LDPC_OK) return rc;
    float qs;
    if ((rc = sim_mod_llr_out("ldpc_sim_generate_mod", llr_fmt, qscale, d_llr, nullptr, false, qs)) != LDPC_OK) return rc;
    SimModRun r;
    if ((rc = sim_mod_run("ldpc_sim_generate_mod", sim, ldpc_sim_noise_var(sim, mod, ebn0_db), true, seed, first_frame, batch, ebn0_db, d_msg_in, msg_fmt, d_msg, stream, r)) != LDPC_OK) return rc;
    if (mod->b) return ldpc::product_generate_launch(r.st, mod->ax, mod->b, batch, sim->dev.n_tx, sim->dev.N, sim->d_cw, r.PB, seed, first_frame, r.sg, r.inv, d_llr, llr_fmt, qs);
    return ldpc::mod_generate_launch(r.st, mod->tab, mod->m, batch, sim->dev.n_tx, sim->dev.N, sim->d_cw, r.PB, seed, first_frame, r.sg, r.inv, d_llr, llr_fmt, qs);
}

// ---- the bit interleaver (csrc/interleaver.h): the object, the demapper and the modulated path through it, the table alone
ldpc_interleaver *ldpc_interleaver_create_on(int device, int n_tx, int N, const int32_t *pos) {
    std::vector<int32_t> holes;
    if (ldpc::interleaver_check("ldpc_interleaver_create_on", n_tx, N, pos, holes) != LDPC_OK) return nullptr;   // before the device is touched
    if (device < 0) { set_error(LDPC_ENODEVICE, "ldpc_init() has not succeeded"); return nullptr; }
    if (check_device(device) != LDPC_OK) return nullptr;
    ldpc_interleaver *il = new (std::nothrow) ldpc_interleaver();
    if (!il) { set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    il->n_tx = n_tx; il->N = N; il->device = device; il->n_holes = (int)holes.size();
    il->pos.assign(pos, pos + n_tx);
    il->max_pos = *std::max_element(il->pos.begin(), il->pos.end());
    // one allocation: pos | pad (0; rounded up so the hole list starts on 16 bytes) | holes
    const size_t hole_at = ((size_t)n_tx + ldpc::kIlPad + 3) / 4 * 4;
    std::vector<int32_t> tab(hole_at + holes.size(), 0);
    std::copy(il->pos.begin(), il->pos.end(), tab.begin());
    std::copy(holes.begin(), holes.end(), tab.begin() + hole_at);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void **)&il->d_tab, tab.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(il->d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_error(LDPC_EHIP, "ldpc_interleaver_create_on: %s", hipGetErrorString(e)); ldpc_interleaver_destroy(il); return nullptr; }
    il->tab.pos = il->d_tab; il->tab.holes = il->d_tab + hole_at; il->tab.n_tx = n_tx; il->tab.N = N; il->tab.n_holes = il->n_holes;
    return il;
}

void ldpc_interleaver_destroy(ldpc_interleaver *il) {
    if (!il) return;
    if (il->d_tab) { (void)hipSetDevice(il->device); hipFree(il->d_tab); }
    delete il;
}

// the calling thread's device, which must be the table's
static int il_device(const char *what, const ldpc_interleaver *il) {
    const int device = current_device();
    if (device < 0) return set_error(LDPC_ENODEVICE, "ldpc_init() has not succeeded");
    if (il->device != device) return set_error(LDPC_EINVAL, "%s: the interleaver lives on device %d, the calling thread's device is %d", what, il->device, device);
    HIPCHK(hipSetDevice(device));
    return LDPC_OK;
}

int ldpc_demap_dev_il(const ldpc_modulation *mod, const ldpc_interleaver *il, int batch, const float *d_sym, double noise_var, void *d_llr, int llr_fmt, float qscale,
                      void *stream) {
    if (!mod || !il || !d_sym || !d_llr) return set_error(LDPC_EINVAL, "ldpc_demap_dev_il: null argument");
    const bool bad = (uintptr_t)d_sym % 8 != 0 || (uintptr_t)d_llr % llr_elem(llr_fmt) != 0;
    float inv, qs;
    int rc = demap_args("ldpc_demap_dev_il", batch, 0, noise_var, llr_fmt, qscale, bad ? "samples must be 8-byte aligned and LLRs aligned to their element" : nullptr, inv, qs);
    if (rc != LDPC_OK) return rc;
    if ((rc = il_device("ldpc_demap_dev_il", il)) != LDPC_OK) return rc;
    if (mod->b) return ldpc::demap_il_product_launch((hipStream_t)stream, mod->ax, mod->b, mod->rule, il->tab, batch, d_sym, inv, d_llr, llr_fmt, qs);
    return ldpc::demap_il_launch((hipStream_t)stream, mod->tab, mod->m, mod->rule, il->tab, batch, d_sym, inv, d_llr, llr_fmt, qs);
}

int ldpc_interleave_bits_dev(const ldpc_interleaver *il, int batch, const void *d_codewords, int cw_fmt, void *d_tx_bits, int tx_fmt, void *stream) {
    if (!il || !d_codewords || !d_tx_bits) return set_error(LDPC_EINVAL, "ldpc_interleave_bits_dev: null argument");
    if (batch <= 0) return set_error(LDPC_EINVAL, "ldpc_interleave_bits_dev: bad dimensions (batch=%d)", batch);
    if ((cw_fmt != LDPC_BITS_BYTES && cw_fmt != LDPC_BITS_PACKED) || (tx_fmt != LDPC_BITS_BYTES && tx_fmt != LDPC_BITS_PACKED))
        return set_error(LDPC_EINVAL, "ldpc_interleave_bits_dev: unknown bit format (LDPC_BITS_BYTES = 0, LDPC_BITS_PACKED = 1)");
    const int rc = il_device("ldpc_interleave_bits_dev", il);
    if (rc != LDPC_OK) return rc;
    return ldpc::interleave_bits_launch((hipStream_t)stream, il->tab, batch, (const uint8_t *)d_codewords, cw_fmt == LDPC_BITS_PACKED, (uint8_t *)d_tx_bits,
                                        tx_fmt == LDPC_BITS_PACKED);
}

int ldpc_deinterleave_llr_dev(const ldpc_interleaver *il, int batch, const void *d_llr_tx, void *d_llr, int llr_fmt, void *stream) {
    if (!il || !d_llr_tx || !d_llr) return set_error(LDPC_EINVAL, "ldpc_deinterleave_llr_dev: null argument");
    if (batch <= 0) return set_error(LDPC_EINVAL, "ldpc_deinterleave_llr_dev: bad dimensions (batch=%d)", batch);
    int rc = check_llr_out("ldpc_deinterleave_llr_dev", llr_fmt, 0.f);
    if (rc != LDPC_OK) return rc;
    if ((uintptr_t)d_llr_tx % llr_elem(llr_fmt) != 0 || (uintptr_t)d_llr % llr_elem(llr_fmt) != 0)
        return set_error(LDPC_EINVAL, "ldpc_deinterleave_llr_dev: LLRs must be aligned to their element");
    if ((rc = il_device("ldpc_deinterleave_llr_dev", il)) != LDPC_OK) return rc;
    return ldpc::deinterleave_llr_launch((hipStream_t)stream, il->tab, batch, d_llr_tx, d_llr, llr_elem(llr_fmt));
}

// what the frame source's paths ask of a table: its lengths are the source's, it lives on the source's device, and it is a permutation
// of the transmitted prefix (the source's packed codewords are cut at n_tx)
static int sim_il_check(const char *what, const ldpc_sim *sim, const ldpc_interleaver *il) {
    if (!il) return set_error(LDPC_EINVAL, "%s: null interleaver", what);
    if (il->n_tx != sim->dev.n_tx || il->N != sim->dev.N)
        return set_error(LDPC_EINVAL, "%s: the interleaver is for n_tx = %d, N = %d, the frame source for n_tx = %d, N = %d", what, il->n_tx, il->N, sim->dev.n_tx, sim->dev.N);
    if (il->max_pos >= sim->dev.n_tx)
        return set_error(LDPC_EINVAL, "%s: the table reaches position %d, the frame source's codewords are cut at n_tx = %d", what, il->max_pos, sim->dev.n_tx);
    if (il->device != sim->device) return set_error(LDPC_EINVAL, "%s: the interleaver lives on device %d, the frame source on device %d", what, il->device, sim->device);
    return LDPC_OK;
}

int ldpc_sim_transmit_il(ldpc_sim *sim, const ldpc_modulation *mod, const ldpc_interleaver *il, uint64_t seed, uint64_t first_frame, int batch, double ebn0_db,
                         const void *d_msg_in, int msg_fmt, float *d_sym, uint8_t *d_msg, void *stream) {
    int rc = sim_mod_check("ldpc_sim_transmit_il", sim, mod, batch, d_msg_in, msg_fmt, d_sym);
    if (rc != LDPC_OK) return rc;
    if ((rc = sim_il_check("ldpc_sim_transmit_il", sim, il)) != LDPC_OK) return rc;
    if ((uintptr_t)d_sym % 8 != 0) return set_error(LDPC_EINVAL, "ldpc_sim_transmit_il: samples must be 8-byte aligned");
    SimModRun r;
    if ((rc = sim_mod_run("ldpc_sim_transmit_il", sim, ldpc_sim_noise_var(sim, mod, ebn0_db), false, seed, first_frame, batch, ebn0_db, d_msg_in, msg_fmt, d_msg, stream, r)) != LDPC_OK) return rc;
    if (mod->b) return ldpc::product_transmit_il_launch(r.st, mod->ax, mod->b, il->tab, batch, sim->d_cw, r.PB, seed, first_frame, r.sg, d_sym);
    return ldpc::mod_transmit_il_launch(r.st, mod->tab, mod->m, il->tab, batch, sim->d_cw, r.PB, seed, first_frame, r.sg, d_sym);
}

int ldpc_sim_generate_mod_il(ldpc_sim *sim, const ldpc_modulation *mod, const ldpc_interleaver *il, uint64_t seed, uint64_t first_frame, int batch, double ebn0_db,
                             const void *d_msg_in, int msg_fmt, void *d_llr, int llr_fmt, float qscale, uint8_t *d_msg, void *stream) {
    int rc = sim_mod_check("ldpc_sim_generate_mod_il", sim, mod, batch, d_msg_in, msg_fmt, d_llr, true);
    if (rc != LDPC_OK) return rc;
    if ((rc = sim_il_check("ldpc_sim_generate_mod_il", sim, il)) != LDPC_OK) return rc;
    float qs;
    if ((rc = sim_mod_llr_out("ldpc_sim_generate_mod_il", llr_fmt, qscale, d_llr, nullptr, false, qs)) != LDPC_OK) return rc;
    SimModRun r;
    if ((rc = sim_mod_run("ldpc_sim_generate_mod_il", sim, ldpc_sim_noise_var(sim, mod, ebn0_db), true, seed, first_frame, batch, ebn0_db, d_msg_in, msg_fmt, d_msg, stream, r)) != LDPC_OK) return rc;
    if (mod->b) return ldpc::product_generate_il_launch(r.st, mod->ax, mod->b, il->tab, batch, sim->d_cw, r.PB, seed, first_frame, r.sg, r.inv, d_llr, llr_fmt, qs);
    return ldpc::mod_generate_il_launch(r.st, mod->tab, mod->m, il->tab, batch, sim->d_cw, r.PB, seed, first_frame, r.sg, r.inv, d_llr, llr_fmt, qs);
}

// ---- the fading channel and the per-symbol channel state (csrc/fading.h): the demapper with a gain per symbol, the modulated path
// with gains drawn per block, the two fused
// the public descriptor checked and turned into the kernel argument
static int fade_arg(const char *what, const ldpc_fading *fad, ldpc::FadeArg &out) {
    if (!fad) return set_error(LDPC_EINVAL, "%s: null ldpc_fading", what);
    if (fad->struct_size < offsetof(ldpc_fading, k_factor) + sizeof(fad->k_factor))
        return set_error(LDPC_EINVAL, "%s: ldpc_fading.struct_size %zu does not cover block and k_factor", what, fad->struct_size);
    if (fad->block < 1) return set_error(LDPC_EINVAL, "%s: %d symbols per fading block (must be >= 1)", what, fad->block);
    if (!(fad->k_factor >= 0.f) || !std::isfinite(fad->k_factor)) return set_error(LDPC_EINVAL, "%s: the Rician K must be finite and >= 0", what);
    const double K = (double)fad->k_factor;
    out.block = fad->block;
    out.mu = (float)sqrt(K / (K + 1.0));
    out.sd = (float)sqrt(1.0 / (2.0 * (K + 1.0)));
    return LDPC_OK;
}

int ldpc_demap_dev_il_csi(const ldpc_modulation *mod, const ldpc_interleaver *il, int batch, const float *d_sym, const float *d_gain, double noise_var, void *d_llr,
                          int llr_fmt, float qscale, void *stream) {
    if (!mod || !il || !d_sym || !d_gain || !d_llr) return set_error(LDPC_EINVAL, "ldpc_demap_dev_il_csi: null argument");
    const bool bad = (uintptr_t)d_sym % 8 != 0 || (uintptr_t)d_gain % 4 != 0 || (uintptr_t)d_llr % llr_elem(llr_fmt) != 0;
    float inv, qs;
    int rc = demap_args("ldpc_demap_dev_il_csi", batch, 0, noise_var, llr_fmt, qscale,
                        bad ? "samples must be 8-byte aligned, gains 4-byte aligned and LLRs aligned to their element" : nullptr, inv, qs);
    if (rc != LDPC_OK) return rc;
    if ((rc = il_device("ldpc_demap_dev_il_csi", il)) != LDPC_OK) return rc;
    if (mod->b) return ldpc::demap_csi_product_launch((hipStream_t)stream, mod->ax, mod->b, mod->rule, il->tab, batch, d_sym, d_gain, inv, d_llr, llr_fmt, qs);
    return ldpc::demap_csi_launch((hipStream_t)stream, mod->tab, mod->m, mod->rule, il->tab, batch, d_sym, d_gain, inv, d_llr, llr_fmt, qs);
}

int ldpc_demap_dev_il_apriori(const ldpc_modulation *mod, const ldpc_interleaver *il, int batch, const float *d_sym, const float *d_gain, double noise_var,
                              const float *d_apriori, void *d_llr, int llr_fmt, float qscale, void *stream) {
    if (!mod || !il || !d_sym || !d_llr) return set_error(LDPC_EINVAL, "ldpc_demap_dev_il_apriori: null argument");
    if (!d_apriori) return set_error(LDPC_EINVAL, "ldpc_demap_dev_il_apriori: null d_apriori (without bit knowledge: ldpc_demap_dev_il_csi)");
    if (mod->b)
        return set_error(LDPC_EUNSUPPORTED, "ldpc_demap_dev_il_apriori: a product constellation (%d bits per axis) has no demapper with a-priori input: its Gray-like "
                         "per-axis labels gain little from iterating with the decoder; table objects (ldpc_modulation_create, m = 1..6) have one", mod->b);
    const char *bad = nullptr;
    if ((uintptr_t)d_sym % 8 != 0 || (uintptr_t)d_gain % 4 != 0 || (uintptr_t)d_apriori % 4 != 0 || (uintptr_t)d_llr % llr_elem(llr_fmt) != 0) {
        bad = "samples must be 8-byte aligned, gains and a-priori values 4-byte aligned and LLRs aligned to their element";
    } else if (batch > 0) {   // every lane reads the a-priori values of its symbol and writes its LLRs: the two buffers must not share a byte
        const uintptr_t a0 = (uintptr_t)d_apriori, a1 = a0 + (size_t)batch * il->N * sizeof(float);
        const uintptr_t l0 = (uintptr_t)d_llr, l1 = l0 + (size_t)batch * il->N * llr_elem(llr_fmt);
        if (a0 < l1 && l0 < a1) bad = "d_apriori overlaps d_llr (no in-place operation)";
    }
    float inv, qs;
    int rc = demap_args("ldpc_demap_dev_il_apriori", batch, 0, noise_var, llr_fmt, qscale, bad, inv, qs);
    if (rc != LDPC_OK) return rc;
    if ((rc = il_device("ldpc_demap_dev_il_apriori", il)) != LDPC_OK) return rc;
    return ldpc::demap_apriori_launch((hipStream_t)stream, mod->tab, mod->m, mod->rule, il->tab, batch, d_sym, d_gain, d_apriori, inv, d_llr, llr_fmt, qs);
}

int ldpc_sim_transmit_il_fading(ldpc_sim *sim, const ldpc_modulation *mod, const ldpc_interleaver *il, const ldpc_fading *fad, uint64_t seed, uint64_t first_frame, int batch,
                                double ebn0_db, const void *d_msg_in, int msg_fmt, float *d_sym, float *d_gain, uint8_t *d_msg, void *stream) {
    int rc = sim_mod_check("ldpc_sim_transmit_il_fading", sim, mod, batch, d_msg_in, msg_fmt, d_sym);
    if (rc != LDPC_OK) return rc;
    if ((rc = sim_il_check("ldpc_sim_transmit_il_fading", sim, il)) != LDPC_OK) return rc;
    ldpc::FadeArg fa;
    if ((rc = fade_arg("ldpc_sim_transmit_il_fading", fad, fa)) != LDPC_OK) return rc;
    if ((uintptr_t)d_sym % 8 != 0 || (uintptr_t)d_gain % 4 != 0) return set_error(LDPC_EINVAL, "ldpc_sim_transmit_il_fading: samples must be 8-byte aligned, gains 4-byte aligned");
    SimModRun r;
    if ((rc = sim_mod_run("ldpc_sim_transmit_il_fading", sim, ldpc_sim_noise_var(sim, mod, ebn0_db), false, seed, first_frame, batch, ebn0_db, d_msg_in, msg_fmt, d_msg, stream, r)) != LDPC_OK) return rc;
    if (mod->b) return ldpc::fading_product_transmit_launch(r.st, mod->ax, mod->b, il->tab, fa, batch, sim->d_cw, r.PB, seed, first_frame, r.sg, d_sym, d_gain);
    return ldpc::fading_transmit_launch(r.st, mod->tab, mod->m, il->tab, fa, batch, sim->d_cw, r.PB, seed, first_frame, r.sg, d_sym, d_gain);
}

int ldpc_sim_generate_mod_il_fading(ldpc_sim *sim, const ldpc_modulation *mod, const ldpc_interleaver *il, const ldpc_fading *fad, uint64_t seed, uint64_t first_frame,
                                    int batch, double ebn0_db, const void *d_msg_in, int msg_fmt, void *d_llr, int llr_fmt, float qscale, float *d_gain, uint8_t *d_msg,
                                    void *stream) {
    int rc = sim_mod_check("ldpc_sim_generate_mod_il_fading", sim, mod, batch, d_msg_in, msg_fmt, d_llr, true);
    if (rc != LDPC_OK) return rc;
    if ((rc = sim_il_check("ldpc_sim_generate_mod_il_fading", sim, il)) != LDPC_OK) return rc;
    ldpc::FadeArg fa;
    if ((rc = fade_arg("ldpc_sim_generate_mod_il_fading", fad, fa)) != LDPC_OK) return rc;
    float qs;
    if ((rc = sim_mod_llr_out("ldpc_sim_generate_mod_il_fading", llr_fmt, qscale, d_llr, d_gain, true, qs)) != LDPC_OK) return rc;
    SimModRun r;
    if ((rc = sim_mod_run("ldpc_sim_generate_mod_il_fading", sim, ldpc_sim_noise_var(sim, mod, ebn0_db), true, seed, first_frame, batch, ebn0_db, d_msg_in, msg_fmt, d_msg, stream, r)) != LDPC_OK) return rc;
    if (mod->b)
        return ldpc::fading_product_generate_launch(r.st, mod->ax, mod->b, il->tab, fa, batch, sim->d_cw, r.PB, seed, first_frame, r.sg, r.inv, d_llr, llr_fmt, qs, d_gain);
    return ldpc::fading_generate_launch(r.st, mod->tab, mod->m, il->tab, fa, batch, sim->d_cw, r.PB, seed, first_frame, r.sg, r.inv, d_llr, llr_fmt, qs, d_gain);
}

// ---- rate matching and HARQ (csrc/ratematch.h): the table whose entries may repeat, the demapper summing through it, the table alone,
// the modulated path reading it
ldpc_ratematch *ldpc_ratematch_create_on(int device, int E, int N, const int32_t *pos) {
    if (ldpc::ratematch_check("ldpc_ratematch_create_on", E, N, pos) != LDPC_OK) return nullptr;   // before the device is touched
    ldpc_ratematch *rm = new (std::nothrow) ldpc_ratematch();
    if (!rm) { set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    std::vector<int32_t> tab;
    // one allocation: pos | pad (0) | inv_ptr | inv_t, each part starting on 16 bytes
    const size_t ptr_at = ((size_t)E + ldpc::kIlPad + 3) / 4 * 4, t_at = ptr_at + ((size_t)N + 1 + 3) / 4 * 4;
    try {
        rm->pos.assign(pos, pos + E);
        if (ldpc::ratematch_invert(E, N, pos, rm->inv_ptr, rm->inv_t) != LDPC_OK) { delete rm; return nullptr; }
        tab.assign(t_at + (size_t)E, 0);
    } catch (const std::bad_alloc &) { delete rm; set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    if (device < 0) { delete rm; set_error(LDPC_ENODEVICE, "ldpc_init() has not succeeded"); return nullptr; }
    if (check_device(device) != LDPC_OK) { delete rm; return nullptr; }
    rm->E = E; rm->N = N; rm->device = device;
    rm->max_pos = *std::max_element(rm->pos.begin(), rm->pos.end());
    std::copy(rm->pos.begin(), rm->pos.end(), tab.begin());
    std::copy(rm->inv_ptr.begin(), rm->inv_ptr.end(), tab.begin() + ptr_at);
    std::copy(rm->inv_t.begin(), rm->inv_t.end(), tab.begin() + t_at);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void **)&rm->d_tab, tab.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(rm->d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_error(LDPC_EHIP, "ldpc_ratematch_create_on: %s", hipGetErrorString(e)); ldpc_ratematch_destroy(rm); return nullptr; }
    rm->tab.pos = rm->d_tab; rm->tab.inv_ptr = rm->d_tab + ptr_at; rm->tab.inv_t = rm->d_tab + t_at; rm->tab.E = E; rm->tab.N = N;
    return rm;
}

void ldpc_ratematch_destroy(ldpc_ratematch *rm) {
    if (!rm) return;
    if (rm->d_tab) { (void)hipSetDevice(rm->device); hipFree(rm->d_tab); }
    delete rm;
}

// the calling thread's device, which must be the table's
static int rm_device(const char *what, const ldpc_ratematch *rm) {
    const int device = current_device();
    if (device < 0) return set_error(LDPC_ENODEVICE, "ldpc_init() has not succeeded");
    if (rm->device != device) return set_error(LDPC_EINVAL, "%s: the table lives on device %d, the calling thread's device is %d", what, rm->device, device);
    HIPCHK(hipSetDevice(device));
    return LDPC_OK;
}

int ldpc_demap_dev_rm(const ldpc_modulation *mod, const ldpc_ratematch *rm, int batch, const float *d_sym, const float *d_gain, double noise_var, void *d_llr, int llr_fmt,
                      float qscale, int accumulate, void *stream) {
    if (!mod || !rm || !d_sym || !d_llr) return set_error(LDPC_EINVAL, "ldpc_demap_dev_rm: null argument");
    const bool bad = (uintptr_t)d_sym % 8 != 0 || (uintptr_t)d_gain % 4 != 0 || (uintptr_t)d_llr % llr_elem(llr_fmt) != 0;
    float inv, qs;
    int rc = demap_args("ldpc_demap_dev_rm", batch, accumulate, noise_var, llr_fmt, qscale,
                        bad ? "samples must be 8-byte aligned, gains 4-byte aligned and LLRs aligned to their element" : nullptr, inv, qs);
    if (rc != LDPC_OK) return rc;
    if ((rc = rm_device("ldpc_demap_dev_rm", rm)) != LDPC_OK) return rc;
    if (mod->b) return ldpc::demap_rm_product_launch((hipStream_t)stream, mod->ax, mod->b, mod->rule, rm->tab, batch, d_sym, d_gain, inv, d_llr, llr_fmt, qs, accumulate != 0);
    return ldpc::demap_rm_launch((hipStream_t)stream, mod->tab, mod->m, mod->rule, rm->tab, batch, d_sym, d_gain, inv, d_llr, llr_fmt, qs, accumulate != 0);
}

int ldpc_ratematch_llr_dev(const ldpc_ratematch *rm, int batch, const float *d_llr_tx, void *d_llr, int llr_fmt, float qscale, int accumulate, void *stream) {
    if (!rm || !d_llr_tx || !d_llr) return set_error(LDPC_EINVAL, "ldpc_ratematch_llr_dev: null argument");
    if (batch <= 0) return set_error(LDPC_EINVAL, "ldpc_ratematch_llr_dev: bad dimensions (batch=%d)", batch);
    if (accumulate != 0 && accumulate != 1) return set_error(LDPC_EINVAL, "ldpc_ratematch_llr_dev: accumulate must be 0 or 1");
    int rc = check_llr_out("ldpc_ratematch_llr_dev", llr_fmt, qscale);
    if (rc != LDPC_OK) return rc;
    if ((uintptr_t)d_llr_tx % 4 != 0 || (uintptr_t)d_llr % llr_elem(llr_fmt) != 0)
        return set_error(LDPC_EINVAL, "ldpc_ratematch_llr_dev: the transmitted LLRs must be 4-byte aligned and the output aligned to its element");
    if ((rc = rm_device("ldpc_ratematch_llr_dev", rm)) != LDPC_OK) return rc;
    return ldpc::ratematch_llr_launch((hipStream_t)stream, rm->tab, batch, d_llr_tx, d_llr, llr_fmt, qscale == 0.f ? 4.0f : qscale, accumulate != 0);
}

int ldpc_ratematch_bits_dev(const ldpc_ratematch *rm, int batch, const void *d_codewords, int cw_fmt, void *d_tx_bits, int tx_fmt, void *stream) {
    if (!rm || !d_codewords || !d_tx_bits) return set_error(LDPC_EINVAL, "ldpc_ratematch_bits_dev: null argument");
    if (batch <= 0) return set_error(LDPC_EINVAL, "ldpc_ratematch_bits_dev: bad dimensions (batch=%d)", batch);
    if ((cw_fmt != LDPC_BITS_BYTES && cw_fmt != LDPC_BITS_PACKED) || (tx_fmt != LDPC_BITS_BYTES && tx_fmt != LDPC_BITS_PACKED))
        return set_error(LDPC_EINVAL, "ldpc_ratematch_bits_dev: unknown bit format (LDPC_BITS_BYTES = 0, LDPC_BITS_PACKED = 1)");
    const int rc = rm_device("ldpc_ratematch_bits_dev", rm);
    if (rc != LDPC_OK) return rc;
    // the interleaver's kernel: it reads pos [E] and gathers, and never assumed an injection
    return ldpc::interleave_bits_launch((hipStream_t)stream, ldpc::rm_as_il(rm->tab), batch, (const uint8_t *)d_codewords, cw_fmt == LDPC_BITS_PACKED, (uint8_t *)d_tx_bits,
                                        tx_fmt == LDPC_BITS_PACKED);
}

double ldpc_sim_noise_var_rm(const ldpc_sim *sim, const ldpc_modulation *mod, const ldpc_ratematch *rm, double ebn0_db) {
    if (!sim || !mod || !rm) { set_error(LDPC_EINVAL, "ldpc_sim_noise_var_rm: null argument"); return 0.0; }
    const double R = (double)sim->dev.k / (double)rm->E;
    return mod->es / (2.0 * R * (double)mod->m * pow(10.0, ebn0_db / 10.0));
}

int ldpc_sim_transmit_rm(ldpc_sim *sim, const ldpc_modulation *mod, const ldpc_ratematch *rm, const ldpc_fading *fad, uint64_t seed, uint64_t first_frame, int batch,
                         double ebn0_db, const void *d_msg_in, int msg_fmt, float *d_sym, float *d_gain, uint8_t *d_msg, void *stream) {
    int rc = sim_mod_check("ldpc_sim_transmit_rm", sim, mod, batch, d_msg_in, msg_fmt, d_sym);
    if (rc != LDPC_OK) return rc;
    if (!rm) return set_error(LDPC_EINVAL, "ldpc_sim_transmit_rm: null table");
    if (rm->N != sim->dev.N) return set_error(LDPC_EINVAL, "ldpc_sim_transmit_rm: the table is for N = %d, the frame source for N = %d", rm->N, sim->dev.N);
    if (rm->max_pos >= sim->dev.n_tx)
        return set_error(LDPC_EINVAL, "ldpc_sim_transmit_rm: the table reaches position %d, the frame source's codewords are cut at n_tx = %d", rm->max_pos, sim->dev.n_tx);
    if (rm->device != sim->device) return set_error(LDPC_EINVAL, "ldpc_sim_transmit_rm: the table lives on device %d, the frame source on device %d", rm->device, sim->device);
    ldpc::FadeArg fa{};
    if (fad && (rc = fade_arg("ldpc_sim_transmit_rm", fad, fa)) != LDPC_OK) return rc;
    if ((uintptr_t)d_sym % 8 != 0 || (uintptr_t)d_gain % 4 != 0) return set_error(LDPC_EINVAL, "ldpc_sim_transmit_rm: samples must be 8-byte aligned, gains 4-byte aligned");
    if ((size_t)batch * (size_t)rm->E > ldpc::kLaneMaxItems) return set_error(LDPC_EINVAL, "ldpc_sim_transmit_rm: batch * E is more than one launch holds");
    SimModRun r;
    if ((rc = sim_mod_run("ldpc_sim_transmit_rm", sim, ldpc_sim_noise_var_rm(sim, mod, rm, ebn0_db), false, seed, first_frame, batch, ebn0_db, d_msg_in, msg_fmt, d_msg, stream, r)) != LDPC_OK) return rc;
    // the interleaved path's kernels with n_tx = E: they read pos alone, through il_positions / il_label, which gather
    const ldpc::IlTab il = ldpc::rm_as_il(rm->tab);
    if (fad) {
        if (mod->b) return ldpc::fading_product_transmit_launch(r.st, mod->ax, mod->b, il, fa, batch, sim->d_cw, r.PB, seed, first_frame, r.sg, d_sym, d_gain);
        return ldpc::fading_transmit_launch(r.st, mod->tab, mod->m, il, fa, batch, sim->d_cw, r.PB, seed, first_frame, r.sg, d_sym, d_gain);
    }
    if (mod->b) return ldpc::product_transmit_il_launch(r.st, mod->ax, mod->b, il, batch, sim->d_cw, r.PB, seed, first_frame, r.sg, d_sym);
    return ldpc::mod_transmit_il_launch(r.st, mod->tab, mod->m, il, batch, sim->d_cw, r.PB, seed, first_frame, r.sg, d_sym);
}

// ---- CRC attach and check (csrc/crc.h): the object, the two kernels on messages, the check on decoded codewords, the tally
ldpc_crc *ldpc_crc_create_on(int device, int width, uint32_t poly, uint32_t init, uint32_t xorout, int n_bits) {
    if (ldpc::crc_check_params("ldpc_crc_create_on", width, poly, init, xorout, n_bits) != LDPC_OK) return nullptr;   // before the device is touched
    ldpc_crc *crc = new (std::nothrow) ldpc_crc();
    if (!crc) { set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    const int k = n_bits + width;
    std::vector<uint32_t> ext;
    try { ext.assign(((size_t)k + 3) / 4 * 4, 0u); } catch (const std::bad_alloc &) { delete crc; set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    if (device < 0) { delete crc; set_error(LDPC_ENODEVICE, "ldpc_init() has not succeeded"); return nullptr; }
    if (check_device(device) != LDPC_OK) { delete crc; return nullptr; }
    crc->width = width; crc->poly = poly; crc->init = init; crc->xorout = xorout; crc->n_bits = n_bits; crc->device = device;
    ldpc::crc_table(width, poly, n_bits, ext.data());
    for (int j = 0; j < width; j++) ext[(size_t)n_bits + j] = 1u << (width - 1 - j);    // the received CRC bits, as the number they spell
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void **)&crc->d_ext, ext.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(crc->d_ext, ext.data(), ext.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_error(LDPC_EHIP, "ldpc_crc_create_on: %s", hipGetErrorString(e)); ldpc_crc_destroy(crc); return nullptr; }
    crc->tab.ext = crc->d_ext; crc->tab.L = n_bits; crc->tab.w = width; crc->tab.k = k;
    crc->tab.c0 = ldpc::crc_serial(width, poly, init, xorout, n_bits, nullptr);
    return crc;
}

void ldpc_crc_destroy(ldpc_crc *crc) {
    if (!crc) return;
    if (crc->d_ext) { (void)hipSetDevice(crc->device); hipFree(crc->d_ext); }
    delete crc;
}

// what the two entry points on messages share; on LDPC_OK the calling thread's device, which is the object's, is current
static int crc_call_check(const char *what, const ldpc_crc *crc, int batch, const void *d_msg, int msg_fmt) {
    if (!crc || !d_msg) return set_error(LDPC_EINVAL, "%s: null argument", what);
    if (batch <= 0 || (size_t)batch * (size_t)crc->tab.k > ldpc::kCrcMaxItems)
        return set_error(LDPC_EINVAL, "%s: batch = %d: must be >= 1 with batch * k at most 2^32 - 256 (k = %d)", what, batch, crc->tab.k);
    if (msg_fmt != LDPC_BITS_BYTES && msg_fmt != LDPC_BITS_PACKED) return set_error(LDPC_EINVAL, "%s: unknown bit format (LDPC_BITS_BYTES = 0, LDPC_BITS_PACKED = 1)", what);
    if (msg_fmt == LDPC_BITS_PACKED && (uintptr_t)d_msg % 4 != 0) return set_error(LDPC_EINVAL, "%s: packed message rows must be 4-byte aligned", what);
    const int device = current_device();
    if (device < 0) return set_error(LDPC_ENODEVICE, "ldpc_init() has not succeeded");
    if (crc->device != device) return set_error(LDPC_EINVAL, "%s: the CRC lives on device %d, the calling thread's device is %d", what, crc->device, device);
    HIPCHK(hipSetDevice(device));
    return LDPC_OK;
}

int ldpc_crc_attach_dev(const ldpc_crc *crc, int batch, void *d_msg, int msg_fmt, void *stream) {
    const int rc = crc_call_check("ldpc_crc_attach_dev", crc, batch, d_msg, msg_fmt);
    if (rc != LDPC_OK) return rc;
    return ldpc::crc_attach_launch((hipStream_t)stream, crc->tab, batch, d_msg, msg_fmt == LDPC_BITS_PACKED);
}

int ldpc_crc_check_dev(const ldpc_crc *crc, int batch, const void *d_msg, int msg_fmt, uint8_t *d_ok, void *stream) {
    if (!d_ok) return set_error(LDPC_EINVAL, "ldpc_crc_check_dev: null argument");
    const int rc = crc_call_check("ldpc_crc_check_dev", crc, batch, d_msg, msg_fmt);
    if (rc != LDPC_OK) return rc;
    const bool packed = msg_fmt == LDPC_BITS_PACKED;
    return ldpc::crc_check_launch((hipStream_t)stream, crc->tab, batch, (const uint8_t *)d_msg, packed ? (size_t)4 * ((crc->tab.k + 31) / 32) : (size_t)crc->tab.k, packed,
                                  nullptr, d_ok);
}

int ldpc_sim_crc_check(const ldpc_sim *sim, const ldpc_crc *crc, int batch, const void *d_bits, int bits_fmt, uint8_t *d_ok, void *stream) {
    if (!sim || !crc || !d_bits || !d_ok) return set_error(LDPC_EINVAL, "ldpc_sim_crc_check: null argument");
    if (bits_fmt != LDPC_BITS_BYTES && bits_fmt != LDPC_BITS_PACKED)
        return set_error(LDPC_EINVAL, "ldpc_sim_crc_check: unknown bit format (LDPC_BITS_BYTES = 0, LDPC_BITS_PACKED = 1)");
    if (crc->tab.k != sim->dev.k)
        return set_error(LDPC_EINVAL, "ldpc_sim_crc_check: the CRC is for messages of %d + %d bits, the frame source's have %d", crc->n_bits, crc->width, sim->dev.k);
    if (crc->device != sim->device) return set_error(LDPC_EINVAL, "ldpc_sim_crc_check: the CRC lives on device %d, the frame source on device %d", crc->device, sim->device);
    if (batch <= 0 || (size_t)batch * (size_t)sim->dev.k > ldpc::kCrcMaxItems)
        return set_error(LDPC_EINVAL, "ldpc_sim_crc_check: batch = %d: must be >= 1 with batch * k at most 2^32 - 256 (k = %d)", batch, sim->dev.k);
    HIPCHK(hipSetDevice(sim->device));
    const bool packed = bits_fmt == LDPC_BITS_PACKED;
    return ldpc::crc_check_launch((hipStream_t)stream, crc->tab, batch, (const uint8_t *)d_bits, packed ? (size_t)(sim->dev.N + 7) / 8 : (size_t)sim->dev.N, packed,
                                  sim->systematic ? sim->sy.msg_pos : nullptr, d_ok);
}

int ldpc_sim_tally_crc(ldpc_sim *sim, int batch, const uint8_t *d_bits, const uint8_t *d_ok, uint64_t *d_tally, void *stream) {
    if (!sim || !d_bits || !d_ok || !d_tally) return set_error(LDPC_EINVAL, "ldpc_sim_tally_crc: null argument");
    if (batch <= 0 || batch > sim->max_batch) return set_error(LDPC_EINVAL, "ldpc_sim_tally_crc: batch %d outside 1..%d", batch, sim->max_batch);
    HIPCHK(hipSetDevice(sim->device));
    return ldpc::crc_tally_launch((hipStream_t)stream, sim->systematic ? sim->sy.msg_pos : nullptr, sim->dev.N, sim->dev.k, sim->dev.kwords, sim->d_msgw, batch,
                                  d_bits, d_ok, (unsigned long long *)d_tally);
}

// ---- the BCH outer code (csrc/bch.h): the object, encode and decode on rows, the decode on decoded codewords
ldpc_bch *ldpc_bch_create_on(int device, int m, uint32_t prim_poly, int t, int n) {
    ldpc_bch *bch = new (std::nothrow) ldpc_bch();
    if (!bch) { set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    std::vector<uint32_t> planes;
    try {
        std::string err;
        if (bch->code.init("ldpc_bch_create_on", m, prim_poly, t, n, err) != 0) {   // before the device is touched
            delete bch;
            set_error(LDPC_EINVAL, "%s", err.c_str());
            return nullptr;
        }
        const int words = (bch->code.p + 31) / 32;
        bch->W = words <= 2 ? words : words <= 4 ? 4 : words <= 6 ? 6 : 8;
        if (device >= 0) bch->code.table(bch->W, planes);
    } catch (const std::bad_alloc &) { delete bch; set_error(LDPC_ENOMEM, "out of host memory"); return nullptr; }
    if (device < 0) return bch;                                                     // a host-only object: the two _host functions serve it
    if (check_device(device) != LDPC_OK) { delete bch; return nullptr; }
    bch->device = device;
    const ldpc::BchCode &c = bch->code;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void **)&bch->d_T, planes.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(bch->d_T, planes.data(), planes.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&bch->d_alog, c.alog.size() * 2);
    if (e == hipSuccess) e = hipMemcpy(bch->d_alog, c.alog.data(), c.alog.size() * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&bch->d_log, c.log.size() * 2);
    if (e == hipSuccess) e = hipMemcpy(bch->d_log, c.log.data(), c.log.size() * 2, hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_error(LDPC_EHIP, "ldpc_bch_create_on: %s", hipGetErrorString(e)); ldpc_bch_destroy(bch); return nullptr; }
    bch->tab.T = bch->d_T; bch->tab.alog = bch->d_alog; bch->tab.log = bch->d_log;
    bch->tab.n = c.n; bch->tab.k = c.k; bch->tab.p = c.p; bch->tab.n4 = (c.n + 3) / 4 * 4; bch->tab.m = c.m; bch->tab.t = c.t; bch->tab.N0 = c.N0;
    bch->tab.prim_poly = c.prim_poly;
    return bch;
}

void ldpc_bch_destroy(ldpc_bch *bch) {
    if (!bch) return;
    if (bch->device >= 0) {
        (void)hipSetDevice(bch->device);
        if (bch->d_T) hipFree(bch->d_T);
        if (bch->d_alog) hipFree(bch->d_alog);
        if (bch->d_log) hipFree(bch->d_log);
    }
    delete bch;
}

// what the two entry points on rows share; on LDPC_OK the calling thread's device, which is the object's, is current
static int bch_call_check(const char *what, const ldpc_bch *bch, int batch, const void *d_rows, int fmt) {
    if (!bch || !d_rows) return set_error(LDPC_EINVAL, "%s: null %s", what, bch ? "d_rows" : "bch");
    if (batch <= 0 || (size_t)batch * (size_t)bch->code.n > ldpc::kBchMaxItems)
        return set_error(LDPC_EINVAL, "%s: batch = %d: must be >= 1 with batch * n at most 2^32 - 256 (n = %d)", what, batch, bch->code.n);
    if (fmt != LDPC_BITS_BYTES && fmt != LDPC_BITS_PACKED) return set_error(LDPC_EINVAL, "%s: fmt = %d: unknown bit format (LDPC_BITS_BYTES = 0, LDPC_BITS_PACKED = 1)", what, fmt);
    if (fmt == LDPC_BITS_PACKED && (uintptr_t)d_rows % 4 != 0) return set_error(LDPC_EINVAL, "%s: d_rows: packed rows must be 4-byte aligned", what);
    if (bch->device < 0) return set_error(LDPC_EINVAL, "%s: bch is a host-only object (created with device = -1)", what);
    const int device = current_device();
    if (device < 0) return set_error(LDPC_ENODEVICE, "ldpc_init() has not succeeded");
    if (bch->device != device) return set_error(LDPC_EINVAL, "%s: bch lives on device %d, the calling thread's device is %d", what, bch->device, device);
    HIPCHK(hipSetDevice(device));
    return LDPC_OK;
}

int ldpc_bch_encode_dev(const ldpc_bch *bch, int batch, void *d_rows, int fmt, void *stream) {
    const int rc = bch_call_check("ldpc_bch_encode_dev", bch, batch, d_rows, fmt);
    if (rc != LDPC_OK) return rc;
    return ldpc::bch_encode_launch((hipStream_t)stream, bch->tab, bch->W, batch, d_rows, fmt == LDPC_BITS_PACKED);
}

int ldpc_bch_decode_dev(const ldpc_bch *bch, int batch, void *d_rows, int fmt, int32_t *d_nerr, void *stream) {
    if (!d_nerr) return set_error(LDPC_EINVAL, "ldpc_bch_decode_dev: null d_nerr");
    const int rc = bch_call_check("ldpc_bch_decode_dev", bch, batch, d_rows, fmt);
    if (rc != LDPC_OK) return rc;
    const bool packed = fmt == LDPC_BITS_PACKED;
    return ldpc::bch_decode_launch((hipStream_t)stream, bch->tab, bch->W, batch, (uint8_t *)d_rows, packed ? (size_t)4 * ((bch->code.n + 31) / 32) : (size_t)bch->code.n, packed,
                                   nullptr, d_nerr);
}

int ldpc_sim_bch_decode(const ldpc_sim *sim, const ldpc_bch *bch, int batch, void *d_bits, int bits_fmt, int32_t *d_nerr, void *stream) {
    if (!sim || !bch || !d_bits || !d_nerr) return set_error(LDPC_EINVAL, "ldpc_sim_bch_decode: null %s", !sim ? "sim" : !bch ? "bch" : !d_bits ? "d_bits" : "d_nerr");
    if (bits_fmt != LDPC_BITS_BYTES && bits_fmt != LDPC_BITS_PACKED)
        return set_error(LDPC_EINVAL, "ldpc_sim_bch_decode: bits_fmt = %d: unknown bit format (LDPC_BITS_BYTES = 0, LDPC_BITS_PACKED = 1)", bits_fmt);
    if (bch->code.n != sim->dev.k)
        return set_error(LDPC_EINVAL, "ldpc_sim_bch_decode: bch is for rows of n = %d bits, the frame source's messages have %d", bch->code.n, sim->dev.k);
    if (bch->device != sim->device) return set_error(LDPC_EINVAL, "ldpc_sim_bch_decode: bch lives on device %d, the frame source on device %d", bch->device, sim->device);
    if (batch <= 0 || (size_t)batch * (size_t)sim->dev.k > ldpc::kBchMaxItems)
        return set_error(LDPC_EINVAL, "ldpc_sim_bch_decode: batch = %d: must be >= 1 with batch * n at most 2^32 - 256 (n = %d)", batch, sim->dev.k);
    HIPCHK(hipSetDevice(sim->device));
    const bool packed = bits_fmt == LDPC_BITS_PACKED;
    return ldpc::bch_decode_launch((hipStream_t)stream, bch->tab, bch->W, batch, (uint8_t *)d_bits, packed ? (size_t)(sim->dev.N + 7) / 8 : (size_t)sim->dev.N, packed,
                                   sim->systematic ? sim->sy.msg_pos : nullptr, d_nerr);
}

int ldpc_sim_extract_messages(const ldpc_sim *sim, int batch, const uint8_t *d_bits, void *d_msg, int msg_fmt, void *stream) {
    const int rc = sim_check_messages("ldpc_sim_extract_messages", sim, batch, d_bits, d_msg, msg_fmt, LDPC_BITS_BYTES, false);
    if (rc != LDPC_OK) return rc;
    if (msg_fmt == LDPC_BITS_PACKED && (uintptr_t)d_msg % 4 != 0) return set_error(LDPC_EINVAL, "ldpc_sim_extract_messages: packed message rows must be 4-byte aligned");
    HIPCHK(hipSetDevice(sim->device));
    return ldpc::sim_extract_messages((hipStream_t)stream, d_bits, sim->dev.N, sim->systematic ? sim->sy.msg_pos : nullptr, d_msg, msg_fmt, sim->dev.kwords, sim->dev.k, batch);
}

int ldpc_sim_tally(ldpc_sim *sim, int batch, const uint8_t *d_bits, const int32_t *d_iters, uint64_t *d_tally, void *stream) {
    if (!sim || !d_bits || !d_tally || batch < 0 || batch > sim->max_batch) return set_error(LDPC_EINVAL, "ldpc_sim_tally: bad arguments");
    if (batch == 0) return LDPC_OK;
    HIPCHK(hipSetDevice(sim->device));
    if (sim->systematic)
        return ldpc::sim_systematic_tally(sim->sy, sim->dev.N, sim->dev.k, sim->dev.kwords, sim->d_msgw, (hipStream_t)stream, batch, d_bits, d_iters,
                                          (unsigned long long *)d_tally);
    return ldpc::sim_tally(sim->dev, sim->d_msgw, (hipStream_t)stream, batch, d_bits, d_iters, (unsigned long long *)d_tally);
}

int ldpc_sim_encode_host(const ldpc_sim *sim, const uint8_t *msg, uint8_t *parity) {
    if (!sim || !msg || !parity) return set_error(LDPC_EINVAL, "null argument");
    if (sim->systematic) {   // parity bit j (at par_pos[j]) = XOR over the set message bits i of P[i][j]
        const ldpc::SystematicForm &sf = sim->sf;
        std::vector<uint64_t> acc((size_t)sf.pw64, 0ull);
        for (int i = 0; i < sf.K; i++)
            if (msg[i])
                for (int w = 0; w < sf.pw64; w++) acc[w] ^= sf.P[(size_t)i * sf.pw64 + w];
        for (int j = 0; j < sf.rank; j++) parity[j] = (uint8_t)((acc[j >> 6] >> (j & 63)) & 1ull);
        return LDPC_OK;
    }
    const int kw = sim->dev.kwords;
    std::vector<uint32_t> mw((size_t)kw, 0u);
    for (int r = 0; r < sim->dev.k; r++) if (msg[r]) mw[r >> 5] |= 1u << (r & 31);
    if (sim->sparse) {   // back-substitution: parity bit j = XOR of the other columns of row order[j], all of them earlier
        const int K = sim->dev.k;
        for (int j = 0; j < sim->p; j++) {
            unsigned b = 0;
            for (int q = sim->sp_ptr[j]; q < sim->sp_ptr[j + 1]; q++) {
                const int c = sim->sp_col[q];
                b ^= c < K ? (unsigned)(msg[c] != 0) : (unsigned)parity[c - K];
            }
            parity[j] = (uint8_t)b;
        }
        return LDPC_OK;
    }
    if (!sim->qc_host.empty()) {
        // Fast/Encoder.hs:42-63 word by word: res[col] = XOR_row mulWord(v'[row], g[row][col]), mulWord = rotate-and-xor
        // over the set bits of the message word
        const int W = sim->dev.qc_w, R = sim->dev.qc_brows, Cc = sim->dev.qc_bcols, sz = 32 * W;
        std::vector<uint32_t> res((size_t)W), rotd((size_t)W);
        for (int c = 0; c < Cc; c++) {
            std::fill(res.begin(), res.end(), 0u);
            for (int r = 0; r < R; r++) {
                const uint32_t *g = &sim->qc_host[((size_t)r * Cc + c) * W];
                for (int n = 0; n < sz; n++) {
                    if (!((mw[(size_t)r * W + (n >> 5)] >> (n & 31)) & 1u)) continue;
                    const int a = n >> 5, b = n & 31;
                    for (int w = 0; w < W; w++) {
                        const uint32_t lo = g[(w - a + W) % W], hi = g[(w - a - 1 + 2 * W) % W];
                        res[w] ^= b ? ((lo << b) | (hi >> (32 - b))) : lo;
                    }
                }
            }
            for (int j = 0; j < sz; j++) parity[(size_t)c * sz + j] = (uint8_t)((res[j >> 5] >> (j & 31)) & 1u);
        }
        return LDPC_OK;
    }
    for (int j = 0; j < sim->p; j++) {
        uint32_t acc = 0;
        for (int w = 0; w < kw; w++) acc ^= mw[w] & sim->gt_host[(size_t)j * kw + w];
        parity[j] = (uint8_t)(__builtin_popcount(acc) & 1);
    }
    return LDPC_OK;
}

}  // extern "C"
