/*
 * ldpc_hip.h -- C ABI of libldpc_hip.so: the MI355X (gfx950) LDPC belief-propagation decoder
 * that replaces the decoder slot of ku-fpg/ecc-ldpc's `Code`/`ECC` record.
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference repository).  The Haskell side keeps its contract: a plug-in is a `Code` built by
 *   mkLDPC_CodeIO name maxThreadCount encoder decoder initialize finalize
 *                                                   (src/ECC/Code/LDPC/Utils.hs:91-108)
 * and everything the CUDA plug-ins do behind that record -- loadFile ptx, getFun, mallocArray,
 * launchKernel, peekListArray (src/ECC/Code/LDPC/GPU/CUDA/Arraylet2.hs:88-297) -- lives behind
 * this header instead.  INTEGRATION.md shows the `foreign import ccall` binding.
 *
 * Conventions
 *   - plain C types only; no C++ exception crosses the ABI.
 *   - every `int` function returns LDPC_OK (0) or a negative LDPC_E* code; the message for the
 *     last failure on the calling thread is ldpc_last_error().
 *   - pointer-returning functions return NULL on failure (message in ldpc_last_error()).
 *   - LLR sign convention of the reference: LLR > 0 <=> bit 1 (`hard x = x > 0`,
 *     src/ECC/Code/LDPC/GPU/Reference.hs:59-60, cudabits/common.h:180-182).
 *   - decoder semantics are exactly the loop of src/ECC/Code/LDPC/Reference/Orig.hs:67-71:
 *     (1) syndrome of hard(lam) zero -> return lam; (2) n >= max_iters -> return the CHANNEL
 *     LLRs (orig_lam); (3) otherwise update.  So bits = hard(lam_n) for a frame that converged
 *     after n updates and hard(channel LLR) for one that did not.
 *   - a context is NOT thread-safe: one ldpc_ctx per calling thread (the reference's CUDA
 *     plug-ins keep mutable device buffers in the closure the same way, Arraylet2.hs:61,118-144).
 */
#ifndef LDPC_HIP_H
#define LDPC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_OK 0
#define LDPC_EINVAL (-1)       /* bad argument */
#define LDPC_ENOMEM (-2)       /* host or device allocation failed */
#define LDPC_EHIP (-3)         /* a HIP runtime call failed (message has the HIP error string) */
#define LDPC_ENODEVICE (-4)    /* no usable gfx950 device / ldpc_init not called */
#define LDPC_EUNSUPPORTED (-5) /* valid request this build has no kernel for */
#define LDPC_EDEGREE (-6)      /* min-sum on a degree-1 check row (Haskell: foldr1 on [], Min.hs:79) */
#define LDPC_EFORMAT (-7)      /* matrix file does not parse */
#define LDPC_ENOTFOUND (-8)    /* matrix file / code name not found */

typedef struct ldpc_code ldpc_code; /* immutable parity-check graph, host + device tables */
typedef struct ldpc_ctx ldpc_ctx;   /* one decoder replica: device buffers + stream          */

/* check-node rule.  LDPC_TANH: Reference/Orig.hs:81-92 ; LDPC_MINSUM: Reference/Min.hs:75-87 ;
 * LDPC_TANH_CM: the tanh rule with the roundings of the reference's `arraylet-cm` decoder (Fast/CachedMult.hs:25-56,
 * 233-264: row product cached as a StableDiv, leave-one-out by division, column sum orig + foldr1 (+)) -- the same real
 * function as LDPC_TANH, ~1e-11 apart in double.  Parity mode only: LDPC_F64, flooding schedule, flood path. */
/* LDPC_TANH_CUDA32 (r04): the arithmetic of the reference's LIVE GPU decoder `cuda-arraylet2` (GPU/CUDA/Arraylet2.hs:88-331 driving
 * cudabits/arraylet2.cu:43-83 selfProduct, common.h:82-88 atanh_, :151-178 updateLam; float_ty = float): float state, factors = the
 * double tanh stored as floats, the leave-one-out product in a double register, atanh_ on its FLOAT value (so the +-18.71 clamp
 * fires when the product rounds to +-1 in float, |x| > ~17, where Orig.hs's Double goes on to ~37), column sums
 * ((orig + ne_1) + ne_2) + ... in float over ascending rows.  In the saturation regime a different function from LDPC_TANH.
 * Parity mode only: LDPC_F32, flooding schedule, flood path, rows up to weight 32 (checker: oracle "cuda32"). */
typedef enum { LDPC_TANH = 0, LDPC_MINSUM = 1, LDPC_TANH_CM = 2, LDPC_TANH_CUDA32 = 3 } ldpc_variant;
/* arithmetic / storage type of LLRs and messages on the device.
 * F32: the cudabits kernels' `typedef float float_ty` (cudabits/common.h:1).  With LDPC_SCHED_LAYERED, min-sum and
 *      LDPC_PATH_FUSED on an H no quasi-cyclic kernel takes, whose frame fits the LDS as f32 (4 N + 32 B <= 160 KB: N <= 40 952):
 *      csrc/layered_csr.hip with lam kept as f32 in LDS -- bit for bit the LDPC_PATH_FLOOD decoder of the same context; a frame whose
 *      LLRs leave the float range is failed, never reported converged (non-finite veto).
 * F64: parity mode, same type as the CPU reference (Double).
 * F16: fp16 storage of whatever the decoder keeps in HBM, fp32 arithmetic (BASELINE.json configs[3]):
 *      every LLR given to an F16 context counts as stored in fp16 (saturating round-to-nearest-even on load);
 *      the flood path also keeps lam and the messages in fp16 between its kernels, the fused paths keep them
 *      on-chip in f32 -- so for F16 the two paths are two different (documented) decoders, each with its own
 *      emulation in oracle/emulate_f16.py, whereas for F32/F64 they agree bit for bit.  With LDPC_SCHED_LAYERED from HBM
 *      (quasi-cyclic codes, min-sum): lam stored in fp16, f32 row records (emulation decode_minsum_f16_layered).  With
 *      LDPC_SCHED_LAYERED, min-sum, on any other H whose frame fits the LDS in fp16 (csrc/layered_csr.hip): lam STORED in fp16
 *      on-chip -- the arithmetic of that from-HBM F16 layered decoder (same emulation), not "the f32 decoder fed fp16-rounded LLRs". */
/* F16PK (extension, BASELINE.json configs[3] "min-sum fp16 LLRs"): ARITHMETIC in IEEE binary16, two frames per lane in
 *      packed instructions (csrc/fused_pk16_body.h holds the specification: the loop of Min.hs:54-104 on fp16 values, the 3/4
 *      applied inside fused multiply-adds; channel LLRs saturate at +-16384 and message magnitudes at 2048, so that no sum
 *      leaves the fp16 range).  Min-sum, on-chip path, either schedule (layered: csrc/fused_layered_body.h), single-circulant
 *      quasi-cyclic codes whose frame fits in LDS, column degree <= 30: built-in instances for the shipped AR4JA matrices,
 *      run-time specialised ones for any other (ldpc_jit_prepare_for); anything else: LDPC_EUNSUPPORTED.  Its checker is the
 *      bit-exact emulation oracle/emulate_f16.py decode_minsum_pk16 / decode_minsum_pk16_layered; BER next to the F32
 *      decoder: DESIGN.md, profiles/r03_ber_pk16_vs_f32.txt. */
/* I8 (extension): a FIXED-POINT decoder, the arithmetic of hardware receivers (6-8 bit LLRs, layered min-sum); integers only, so a
 *      BER is reproducible bit for bit.  Channel LLRs are quantised on load, q = clip(rint(float32(llr) * llr_qscale), -127, 127) -- one
 *      float32 multiply, ties to even, NaN -> 0; int8 LLRs (ldpc_decode_batch_i8) are taken as they are, -128 as -127.  lam is an int8
 *      cell in -127..127, hard(lam) = lam > 0.  A row: t_k = lam[c_k] - msg_k (not clamped), m1 / m2 the two smallest |t_k|,
 *      |msg'_k| = (3 m + 2) >> 2 of the smallest of the OTHER edges (the 3/4 of Min.hs:78, rounded half up), negative iff
 *      (weight odd) ^ (xor of the signs of all t_j) ^ (sign of t_k), a zero counting as positive; lam'[c_k] = clip(t_k + msg'_k, -127, 127).
 *      Stopping rule of LDPC_SCHED_LAYERED; final_lam = lam / llr_qscale (the quantised channel LLRs / llr_qscale for a frame out of
 *      sweeps).  Specification: tests/layered_i8_spec.py, reproduced bit for bit.  Min-sum, LDPC_SCHED_LAYERED, LDPC_PATH_AUTO or
 *      LDPC_PATH_FUSED, on ANY code (a quasi-cyclic code as its CSR form, with the layers it has): csrc/layered_csr.hip with one byte of
 *      LDS per column and 8-byte row records.  Row weight 2..27, N <= 65 535; the context reports LDPC_PATH_FUSED.  Anything else --
 *      flooding, another rule, LDPC_PATH_FLOOD, ldpc_debug_step, ldpc_decode_trace, ldpc_jit_* -- is LDPC_EUNSUPPORTED.  Every decode
 *      entry point is accepted (f32, fp16, f64 LLRs are quantised on load). */
typedef enum { LDPC_F32 = 0, LDPC_F64 = 1, LDPC_F16 = 2, LDPC_F16PK = 3, LDPC_I8 = 4 } ldpc_dtype;
/* message-passing schedule.  FLOODING: the reference's (Orig.hs:81-98: all checks, then all variables).
 * LAYERED (extension, no reference counterpart): checks layer by layer, each seeing the LLRs the layers before it
 * updated in the same sweep -- about half the sweeps to converge; stopping rule: before the first sweep the
 * syndrome of the channel decisions, after a sweep "no check it saw was odd and no hard decision changed"
 * (specification: oracle/ldpc_oracle.c oracle_decode_layered); a frame out of sweeps returns the channel decisions,
 * as Orig.hs:70 does.  `iters` counts sweeps. */
typedef enum { LDPC_SCHED_FLOODING = 0, LDPC_SCHED_LAYERED = 1 } ldpc_schedule;
/* order in which a column's messages are added to the channel LLR.  The registered decoders of the reference compute the same
 * check rule but add a column up differently -- the last ulps of a Double, nothing else:
 *   REFERENCE  foldr (+) orig: ne_1 + (ne_2 + (... + (ne_k + orig)))          Reference/Orig.hs:96, Min.hs:101 (`reference`, `min`)
 *   ARRAYLET   orig + (ne_1 + (ne_2 + (... + ne_k)))                          Fast/Arraylet.hs:105-109,185-186, ArrayletMin.hs:191-192
 *                                                                             (`arraylet`, `arraylet-min`; LDPC_TANH_CM implies it)
 *   SPARSE     orig + (((0 + ne_1) + ne_2) + ... + ne_k)                      Reference/Sparse.hs:112-114, SparseMin.hs:117-119,
 *                                                                             Data/Sparse/Matrix.hs:35-36 (`sparse`, `sparsemin`)
 * rows ascending.  ARRAYLET and SPARSE are PARITY MODES (bit-exact f64 against oracle "arraylet" / "sparse"...): flooding
 * schedule, LDPC_PATH_FLOOD batch-major kernels; the on-chip kernels add in REFERENCE order. */
typedef enum { LDPC_SUM_REFERENCE = 0, LDPC_SUM_ARRAYLET = 1, LDPC_SUM_SPARSE = 2 } ldpc_sum_order;
/* which kernel family a context uses */
typedef enum {
    LDPC_PATH_AUTO = 0,  /* on-chip kernel when the code/variant/dtype has one, else the HBM path */
    LDPC_PATH_FLOOD = 1, /* state in HBM, any H: quasi-cyclic codes one workgroup per frame and ONE launch per batch (either
                            schedule), any other H batch-major with two kernels per iteration                              */
    LDPC_PATH_FUSED = 2  /* whole decode in one launch, state in LDS/registers: QC codes (built-in or run-time specialised
                            instances) and any H whose frame fits in 160 KB of LDS; flooding schedule.  Layered schedule:
                            QC codes on-chip; and LDPC_F16 min-sum on any H no QC kernel takes (csrc/layered_csr.hip: lam
                            STORED in fp16 in LDS for the whole decode, row records streamed through an HBM scratch area) --
                            reported as FUSED because lam never leaves the chip, unlike the QC long-code kernel
                            layered_lds.hip, which also keeps lam in LDS but reports FLOOD; an explicit LDPC_PATH_FLOOD
                            still refuses LDPC_F16 layered on such a code.  The same kernel with lam as f32 (LDPC_F32 min-sum,
                            N <= 40 952) is taken on an explicit LDPC_PATH_FUSED only: LDPC_PATH_AUTO keeps LDPC_F32 layered
                            contexts of such codes on the HBM path                                                         */
} ldpc_path;

/* ---- library life-cycle -------------------------------------------------------------------
 * replaces  initialize :: IO CudaAllocations  (GPU/CUDA/Arraylet2.hs:287-293: dummy malloc to
 * create the context + loadFile "cudabits/arraylet2.ptx") and finalize (:295-297).          */
/* ldpc_init: idempotent; checks that `device` is a gfx950 GPU and makes it the CALLING THREAD's device: objects the
 * thread creates afterwards live there.  The first device any thread initialised is the default of threads that
 * never called ldpc_init.  One process can drive several GPUs: one thread per GPU each calling ldpc_init(its device),
 * or one thread using the *_on constructors below (the reference makes maxThreadCount replicas in one process and
 * picks one by thread, Utils.hs:53,63-69). */
int ldpc_init(int device);
int ldpc_shutdown(void);
int ldpc_current_device(void);      /* the calling thread's device (see ldpc_init), -1 if none */
const char *ldpc_last_error(void);  /* thread-local, never NULL */
int ldpc_last_error_code(void);     /* the LDPC_E* code that message belongs to (0 if none yet) */
int ldpc_abi_version(void);         /* bumps when a signature in this header changes */
int ldpc_device_count(void);        /* HIP devices visible; 0 when there is no GPU (no error) */

/* ---- graph ---------------------------------------------------------------------------------
 * replaces initMatrixlet (GPU/CUDA/Arraylet2.hs:299-331): the quasi-cyclic H as circulant size
 * + a block_rows x block_cols table of rotations, -1 = empty block.  Rotation `off` at block
 * (br,bc) means row r of the block has its 1 at column (r+off) mod sz
 * (src/Data/Matrix/QuasiCyclic.hs:19-25, Fast/Arraylet.hs:34-43).  The library copies `offsets`. */
ldpc_code *ldpc_code_create_qc(int sz, int block_rows, int block_cols, const int32_t *offsets);
/* any H as CSR (what `Matrix Bool` decoders take, Reference/Orig.hs:30): row_ptr[M+1],
 * col_idx[E] strictly ascending inside each row.  The library copies both arrays. */
ldpc_code *ldpc_code_create_csr(int M, int N, const int32_t *row_ptr, const int32_t *col_idx);
void ldpc_code_destroy(ldpc_code *code);
/* M = checks, N = unpunctured code length (cols H), E = edges */
int ldpc_code_dims(const ldpc_code *code, int *M, int *N, int *E);
/* the CSR edge order the library uses for every per-edge array it exposes (debug entry points):
 * row-major, ascending column inside a row == the order of Orig.hs:86-91.  Arrays caller-owned. */
int ldpc_code_csr(const ldpc_code *code, int32_t *row_ptr /*M+1*/, int32_t *col_idx /*E*/);

/* ---- layers (row-layered schedule, an EXTENSION: BASELINE.json configs[4]; the reference has flooding only) -------
 * A layer is a range of consecutive rows that share no column.  Default: the block rows of a quasi-cyclic code (one
 * circulant per block => column-disjoint), every row its own layer for a CSR code.  ldpc_code_set_layers replaces
 * the partition (layer_ptr[0] = 0 < ... < layer_ptr[n_layers] = M; LDPC_EINVAL if two rows of a layer share a column
 * or a context already exists on the code). */
int ldpc_code_set_layers(ldpc_code *code, int n_layers, const int32_t *layer_ptr);
/* A row-layered decoder visits the block rows of a quasi-cyclic H in the order they are given; block rows that follow one another
 * and share no block column can be worked on together with unchanged results, and the long-code kernel (csrc/layered_lds.hip) does so
 * for runs of up to four.  The order of the rows of H is the caller's to choose (a permutation of H's rows is the same code; the
 * SCHEDULE, hence the last digits of a BER, changes with it): this helper proposes one -- perm[i] = the block row to put at place i,
 * runs of up to `run` (1..8) pairwise column-disjoint block rows, full runs first (greedy, deterministic; what
 * tools/gen_dvbs2_like.py applies to codes/dvbs2like.64800.1.2).  Pure host code, needs no GPU.  Returns the number of full runs,
 * < 0 on error.  No counterpart in the reference (flooding only). */
int ldpc_qc_layer_order(int block_rows, int block_cols, const int32_t *offsets, int run, int32_t *perm /* block_rows */);
/* The same for any H, given as CSR the way ldpc_code_create_csr takes it: an order of the rows in which consecutive rows form few
 * column-disjoint layers -- perm[i] = the row to put at place i, layer_ptr[0..n] = the layers of the permuted matrix (what
 * ldpc_code_set_layers takes for the code built from the permuted rows); max_rows > 0 caps the rows of a layer, 0 leaves them
 * uncapped.  First fit in file order (each row joins the lowest layer that holds none of its columns), the rows of a layer in file
 * order: deterministic.  Like ldpc_qc_layer_order it only PROPOSES an order; the on-chip layered kernel for any H
 * (csrc/layered_csr.hip) does one barrier step per run of consecutive column-disjoint layers, so the fewer layers, the faster.
 * Pure host code, needs no GPU.  Returns n (the number of layers), < 0 on error.  No counterpart in the reference. */
int ldpc_csr_layer_order(int M, int N, const int32_t *row_ptr, const int32_t *col_idx, int max_rows,
                         int32_t *perm /* M */, int32_t *layer_ptr /* M + 1 */);
/* Does H (M x N as CSR, 0 < M < N, K = N - M) encode by back-substitution?  Columns 0..K-1 carry the message, K..N-1 the parity
 * bits; last(i) = the largest column of row i.  H QUALIFIES iff no row is empty, last(i) >= K for every row, and i -> last(i) - K
 * is a bijection onto 0..M-1.  Then order[j] = the row with last = K + j: taken in that order the rows have a unit lower-triangular
 * parity part, and  c[0..K) = msg;  c[K+j] = XOR of c[col] over the OTHER columns of row order[j]  (all < K + j)  for j = 0..M-1
 * is the codeword of msg -- the one any systematic generator of the code gives, whatever order the rows are stored in.  DVB-S2-shaped
 * accumulator codes qualify (they are defined this way and ship no generator), codes/moon.7.13 does.  Pure host code, needs no
 * GPU.  LDPC_OK; LDPC_EINVAL for a malformed CSR; LDPC_EUNSUPPORTED when the rule fails, the message naming the first offending
 * row (for two rows that end in one column: both rows and the column).  No counterpart in the reference. */
int ldpc_csr_triangular_order(int M, int N, const int32_t *row_ptr, const int32_t *col_idx, int32_t *order /* M */);
/* A systematic form of ANY H (M x N as CSR; rows may be redundant or empty) by GF(2) elimination.  Visit the columns from N - 1
 * down to 0: column c is a PARITY position iff it is not in the span of the parity positions already chosen (all > c).  The parity
 * positions are par_pos[0..rank) ascending, rank = rank H; every other column is a MESSAGE position, msg_pos[0..K) ascending,
 * K = N - rank.  The codeword of a message m has c[msg_pos[i]] = m[i], and c[par_pos[.]] the unique solution of H c = 0:
 *   c[par_pos[j]] = XOR_i m[i] P[i][j],   P [K][rank] bytes 0/1 (may be NULL; K * rank <= N * N / 4, or call twice).
 * The rule depends on the code only, not on how its rows are stored or how the elimination runs.  Whenever the last rank columns
 * are independent it gives msg ++ parity, the reference's convention (Utils.hs:61) and that of every H
 * ldpc_csr_triangular_order accepts; a zero column is a message position.  Pure host code (bit-packed elimination on 64-bit
 * words), needs no GPU.  LIMIT: M * N <= 2^28 (about 3e10 word operations, tens of seconds, at the limit) -- LDPC_EUNSUPPORTED
 * above it, before any elimination; DVB-S2-shaped matrices of that size encode through ldpc_sim_create_sparse_on.
 * LDPC_EINVAL for a malformed CSR (the checks of ldpc_csr_triangular_order), LDPC_EUNSUPPORTED for K = 0 ("no message bits").
 * msg_pos and par_pos are caller arrays of N entries.  No counterpart in the reference. */
int ldpc_csr_systematic_form(int M, int N, const int32_t *row_ptr, const int32_t *col_idx, int32_t *msg_pos /* N */,
                             int32_t *par_pos /* N */, int *K, int *rank, uint8_t *P /* may be NULL; [K][rank] */);
int ldpc_code_layers(const ldpc_code *code, int *n_layers, int32_t *layer_ptr /* may be NULL; n_layers+1 entries */);

/* ---- decoder replica -------------------------------------------------------------------------
 * replaces one `decoder vars h` call (Utils.hs:53 replicateM maxThreadCount; Arraylet2.hs:88-144:
 * getFun x9, mallocArray of mLet/newMLet/lam/orig_lam/done, Stream.create).  Owns its device
 * buffers and one HIP stream; sized for frames <= max_batch per call. */
ldpc_ctx *ldpc_ctx_create(const ldpc_code *code, int variant, int dtype, int max_batch);
ldpc_ctx *ldpc_ctx_create_ex(const ldpc_code *code, int variant, int dtype, int max_batch, int path);
/* the same on an explicitly named device (no ldpc_init needed on this thread; a code may have replicas on several
 * devices, its graph tables are uploaded once per device) */
ldpc_ctx *ldpc_ctx_create_on(const ldpc_code *code, int device, int variant, int dtype, int max_batch, int path);
/* everything above, plus what was added later, in one extensible structure: set struct_size = sizeof(ldpc_ctx_config)
 * and zero the rest before filling in; device = -1 means the calling thread's device.
 * THE MIN-SUM CHECK-NODE RULE (cn_scale = alpha, cn_offset = beta; extension, no reference counterpart).  Every min-sum kernel of the
 * library computes |msg'| = 3/4 min (Min.hs:78) -- the flooding kernels, the parity modes, the quasi-cyclic on-chip and long-code
 * layered kernels, the run-time specialised ones (ldpc_jit_*: they take a code, not a context, and build 3/4 kernels) do so ALWAYS.
 * The on-chip layered kernel for any H (csrc/layered_csr.hip) also exists with |msg'| = max(alpha min - beta, 0): normalised
 * (beta = 0) or offset (alpha = 1) min-sum, what hardware receivers run.  Float cells (LDPC_F16, LDPC_F32), in float32:
 *   n = fl(fl(alpha) * m) - fl(beta) -- two roundings, no fused multiply-add --, then n < 0 ? 0 : n (a NaN stays a NaN);
 * LDPC_I8, integers only: a = clip(rint(float32(alpha) * 16), 1, 16), b = rint(float32(beta) * float32(llr_qscale)) (ties to even),
 *   n = min(max(((a m + 8) >> 4) - b, 0), 511); the default is a = 12, b = 0, and (12 m + 8) >> 4 == (3 m + 2) >> 2.
 * Everything else of a row -- gathers, signs, arg-min, lam writes, stopping rule, final_lam -- is unchanged.  Specification:
 * tests/layered_rule_spec.py, reproduced bit for bit.  A context whose two fields are 0 or absent, or an explicit (0.75, 0), is
 * selected, named and decoded exactly as without them.  Any other rule is accepted for LDPC_MINSUM, LDPC_SCHED_LAYERED,
 * LDPC_PATH_AUTO or LDPC_PATH_FUSED and LDPC_F16, LDPC_F32 or LDPC_I8, on any code within that kernel's limits (rows of weight
 * 2..27, N <= 65 535, f32 lam N <= 40 952; a quasi-cyclic code is taken as its CSR form with its layers), reports LDPC_PATH_FUSED and
 * ldpc::layered_csr_kernel<D, ldpc::Ruled<LT>>; the flooding schedule, tanh and the parity modes, LDPC_F64, LDPC_F16PK, LDPC_PATH_FLOOD,
 * ldpc_debug_step and ldpc_decode_trace are LDPC_EUNSUPPORTED with a message that names the rule.
 * THE A-MIN* CHECK-NODE RULE (cn_rule = LDPC_CN_AMINSTAR; extension, no reference counterpart; Jones, Valles, Smith, Villasenor 2003).
 * The same kernel family also exists with a row that approximates the sum-product rule and still sends only TWO magnitudes, so that the
 * row record, the soft output and the decode state are what they are.  In float32, every operation rounded on its own:
 *   c(x)  = n = 0.625f - fl(0.25f * x), then n < 0 ? 0 : n                                  (a compare-select: a NaN stays a NaN)
 *   a [+] b = s = fl(min(a, b) + c(fl(a + b))), n = fl(s - c(|fl(a - b)|)), then n < 0 ? 0 : n
 * For a row with differences t_k = lam[c_k] - old msg_k, edges in CSR order: i* = the FIRST k with the least |t_k|, m1 = |t_i*|;
 * Delta = the left fold of [+] over |t_k|, k != i*, in ascending k from the first such edge; n1 = Delta [+] m1.  The message magnitude
 * is Delta on edge i* and n1 on every other edge (an edge that ties with m1 included); a row of weight 2 is exact (the arg-min edge gets
 * the other's |t|, the other gets m1, no [+]).  a [+] b <= min(a, b), so magnitudes are bounded as for cn_scale = 1.  Signs, the parity /
 * flip / stop rule, lam writes (LDPC_F16 saturates and rounds, LDPC_F32 keeps the float and vetoes what is not finite), final_lam, the
 * soft output and the decode state are unchanged.  Specification: tests/layered_aminstar_spec.py, reproduced bit for bit.
 * cn_rule = LDPC_CN_MINSUM (0, or absent) is everything said above.  With LDPC_CN_AMINSTAR cn_scale and cn_offset must be 0 or absent
 * (LDPC_EINVAL otherwise; an unknown cn_rule is LDPC_EINVAL too).  It is accepted exactly where another (cn_scale, cn_offset) is, less
 * LDPC_I8 -- LDPC_MINSUM, LDPC_SCHED_LAYERED, LDPC_PATH_AUTO or LDPC_PATH_FUSED, LDPC_F16 or LDPC_F32, any code within the kernel's
 * limits --, reports LDPC_PATH_FUSED and ldpc::layered_csr_kernel<D, ldpc::MinStar<LT>>; LDPC_I8, the flooding schedule, tanh and the
 * parity modes, LDPC_F64, LDPC_F16PK, LDPC_PATH_FLOOD, ldpc_debug_step and ldpc_decode_trace are LDPC_EUNSUPPORTED with a message that
 * names cn_rule.  ldpc_decode_batch_dev_soft, ldpc_decode_state_* and ldpc_decode_batch_dev_continue serve such a context like any other
 * of the family; the state's layout is unchanged. */
enum ldpc_cn_rule { LDPC_CN_MINSUM = 0, LDPC_CN_AMINSTAR = 1 };
typedef struct {
    size_t struct_size;
    int device, variant, dtype, max_batch, path, schedule;
    int sum_order;   /* ldpc_sum_order; read when struct_size covers it, else LDPC_SUM_REFERENCE */
    float llr_qscale; /* LDPC_I8: the quantiser's scale (LLR units per integer step = 1 / llr_qscale); read for that dtype when struct_size
                         covers it; 0 or absent: 4.0; anything else must be finite and > 0 (LDPC_EINVAL) */
    float cn_scale;   /* alpha; read when struct_size covers it; 0 or absent: 3/4; anything else must be finite and in (0, 1] (LDPC_EINVAL);
                         LDPC_I8: rint(16 alpha) must not be 0 (LDPC_EINVAL) */
    float cn_offset;  /* beta, in LLR units; read when struct_size covers it; 0 or absent: none; anything else must be finite and >= 0
                         (LDPC_EINVAL); LDPC_I8: rint(beta * llr_qscale) must not exceed 127 (LDPC_EINVAL) */
    int cn_rule;      /* ldpc_cn_rule; read when struct_size covers it, else LDPC_CN_MINSUM; LDPC_CN_AMINSTAR wants cn_scale = cn_offset = 0 */
} ldpc_ctx_config;
ldpc_ctx *ldpc_ctx_create_cfg(const ldpc_code *code, const ldpc_ctx_config *cfg);
int ldpc_ctx_schedule(const ldpc_ctx *ctx);
float ldpc_ctx_llr_qscale(const ldpc_ctx *ctx);   /* the quantiser's scale of an LDPC_I8 context, 0 for every other dtype */
/* the min-sum check-node rule the context really computes with: 0.75 and 0 unless configured; the float32 values of the fields for
 * LDPC_F16 / LDPC_F32; the quantised ones, a / 16 and b / llr_qscale, for LDPC_I8; 0 and 0 on a context of the tanh rule and on an
 * A-min* context (neither has a scale or an offset) */
float ldpc_ctx_cn_scale(const ldpc_ctx *ctx);
float ldpc_ctx_cn_offset(const ldpc_ctx *ctx);
/* LDPC_CN_AMINSTAR on an A-min* context, LDPC_CN_MINSUM on every other */
int ldpc_ctx_cn_rule(const ldpc_ctx *ctx);
const ldpc_code *ldpc_ctx_code(const ldpc_ctx *ctx);
int ldpc_ctx_max_batch(const ldpc_ctx *ctx);
int ldpc_ctx_device(const ldpc_ctx *ctx);
void ldpc_ctx_destroy(ldpc_ctx *ctx);
/* LDPC_PATH_FLOOD or LDPC_PATH_FUSED: what the context resolved to */
int ldpc_ctx_path(const ldpc_ctx *ctx);

/* Non-finite channel LLRs.  A NaN or an infinity reaches every decode entry point in ordinary use: the demappers and the fused
 * ldpc_sim_generate_mod* calls write a NaN LLR for a NaN sample or gain (f32 and fp16), and ldpc_decode_batch_f64 on an LDPC_F32
 * context turns a double above FLT_MAX into an infinity.  What a decoder does with such a value (tests/test_nonfinite_llr_gpu.py, one
 * context per kernel family).  THREE KERNELS ARE NOT UNDER THESE RULES YET:
 *   - flood_qc_kernel (a quasi-cyclic code with LDPC_PATH_FLOOD, flooding schedule): a decode of frames with NaN / infinite LLRs has
 *     aborted with a GPU memory fault whose cause is not known; only its +-inf case is tested (tests/test_split_wave_gpu.py);
 *   - the flooding LDPC_F16PK kernel (built-in and run-time specialised): a NaN is taken in as the LLR -16384, not as +0;
 *   - the on-chip layered LDPC_F32 / LDPC_F16 kernel of quasi-cyclic codes (fused_layered_kernel, ldpc_jit_layered_*): LDPC_F16 rounding
 *     takes a NaN as -65504, and a frame whose channel decisions already are a codeword stops before the first sweep, converged, with
 *     the non-finite LLR it was given (after a sweep the check of rule 3 applies).
 * Everywhere else:
 *   1. Converting conversions turn +inf into +max, -inf into -max and a NaN of either sign into +0, an erasure: fp16 storage and
 *      LDPC_F16 rounding (max 65504), LDPC_F16PK (16384; the layered kernel), LDPC_I8 (127: the quantiser's "NaN -> 0" above).  This holds for f32, f64
 *      and fp16 input buffers alike, on the 16-byte loads and on the element-wise ones.  After the conversion the frame is an
 *      ordinary finite frame (oracle/emulate_f16.py r16 / neg_llr16, tests/layered_i8_spec.py quantize).
 *   2. LDPC_F32 and LDPC_F64 state takes the values as they are.
 *   3. LDPC_F32 min-sum -- every kernel family, both schedules, the 3/4 or a per-context rule: whatever comes back converged has
 *      finite final LLRs.  A frame with any non-finite channel LLR therefore FAILS: converged = 0, iters = max_iters, bits = llr > 0
 *      (a NaN of either sign and -inf give 0, +inf gives 1), final_lam = the channel LLRs as given -- also when the channel's hard
 *      decisions already are a codeword.  The soft output of such a frame (ldpc_decode_batch_dev_soft) is lam as it stands when the
 *      frame stopped, not the channel LLRs: it may then hold an infinity or a NaN.
 *   3a. A decode state (ldpc_decode_batch_dev_continue) of an LDPC_F32 context: the veto also looks at the starting lam C' + S.  A slot whose
 *      frame diverged, or was given a non-finite LLR, holds an S that is not finite: it stays failed (converged = 0) in every later call,
 *      whatever LLRs it gets, until ldpc_decode_state_reset.  LDPC_F16 and LDPC_I8 states cannot get there: the cell saturates, S is finite.
 *      Rule 6 holds for slots: the finite frames' results and new state do not depend on what the other slots hold.
 *   4. The tanh rule and LDPC_F64 (the parity modes): no parity with the oracle is claimed on non-finite input; 5 and 6 hold.
 *   5. Self-consistency, every context: a converged frame has H bits = 0 and bits = hard(final_lam); a frame that is not converged
 *      has iters = max_iters and bits = hard(channel LLR as taken in).
 *   6. Isolation, every context: the finite frames of a batch come back bit for bit the same -- bits, iters, flags, final_lam --
 *      whatever non-finite frames share their lane, wave, workgroup or slab of 64, or were decoded by the same workgroup before them. */
/* ---- decode ------------------------------------------------------------------------------------
 * ldpc_decode_one replaces the per-frame closure
 *   Rate -> Int -> U.Vector Double -> IO (Maybe (U.Vector Bool))     (Arraylet2.hs:151-273)
 * llr: N doubles, already un-punctured (zeros appended, Utils.hs:55,69).  bits: N bytes 0/1.
 * A non-zero return is the closure's `Nothing` (Utils.hs:70-71). Blocking. */
int ldpc_decode_one(ldpc_ctx *ctx, int max_iters, const double *llr, uint8_t *bits, int *iters,
                    int *converged);
/* throughput path, host buffers: llr [batch][N] float32 frame-major, bits [batch][N] bytes,
 * iters [batch] (updates run, = max_iters for a non-converged frame), converged [batch].
 * iters / converged may be NULL.  Blocking. */
int ldpc_decode_batch(ldpc_ctx *ctx, int max_iters, int batch, const float *llr, uint8_t *bits,
                      int32_t *iters, uint8_t *converged);
/* same with float64 LLRs in and (optionally) the returned LLR vector out -- `lam` of the frame
 * that converged, the channel LLRs otherwise (what Orig.hs:69-70 returns before `map hard`).
 * final_lam may be NULL. */
int ldpc_decode_batch_f64(ldpc_ctx *ctx, int max_iters, int batch, const double *llr, uint8_t *bits,
                          int32_t *iters, uint8_t *converged, double *final_lam);
/* zero-copy path: every pointer is DEVICE memory on the context's device.  d_llr [batch][N]
 * float32; d_bits [batch][N] bytes; d_iters, d_converged may be NULL.  Work is enqueued on
 * `stream` (a hipStream_t) and NOT synchronised.  NULL = the context's OWN stream, which is
 * non-blocking: it does not order against the default (null) stream, so a caller that produces
 * d_llr on another stream must pass that stream here (or synchronise first).  A context decodes one
 * batch at a time: two calls on one context with different streams must be ordered by the caller. */
int ldpc_decode_batch_dev(ldpc_ctx *ctx, int max_iters, int batch, const float *d_llr,
                          uint8_t *d_bits, int32_t *d_iters, uint8_t *d_converged, void *stream);
/* fp16 channel LLRs (IEEE binary16 bit patterns; BASELINE.json configs[3] "min-sum fp16 LLRs"): the same two
 * throughput entry points with half the bytes per frame over PCIe / out of HBM.  Accepted by a context of any
 * dtype (the values convert exactly to f32/f64).  No counterpart in the reference, whose CUDA path pokes
 * float32 (GPU/CUDA/Arraylet2.hs:151-160). */
int ldpc_decode_batch_f16(ldpc_ctx *ctx, int max_iters, int batch, const uint16_t *llr, uint8_t *bits,
                          int32_t *iters, uint8_t *converged);
int ldpc_decode_batch_dev_f16(ldpc_ctx *ctx, int max_iters, int batch, const uint16_t *d_llr,
                              uint8_t *d_bits, int32_t *d_iters, uint8_t *d_converged, void *stream);
/* int8 channel LLRs, what a demapper delivers: a quarter of the float32 bytes per frame over PCIe / out of HBM (the zero-copy route of
 * page-locked buffers reads 1 byte per element).  Accepted by LDPC_I8 contexts only -- LDPC_EUNSUPPORTED on any other; the values
 * are the decoder's integers as they are (-128 is taken as -127), llr_qscale plays no part.  Same three host routes as
 * ldpc_decode_batch.  No counterpart in the reference. */
int ldpc_decode_batch_i8(ldpc_ctx *ctx, int max_iters, int batch, const int8_t *llr, uint8_t *bits,
                         int32_t *iters, uint8_t *converged);
int ldpc_decode_batch_dev_i8(ldpc_ctx *ctx, int max_iters, int batch, const int8_t *d_llr,
                             uint8_t *d_bits, int32_t *d_iters, uint8_t *d_converged, void *stream);
/* PACKED result bits (r04): ceil(N/8) bytes per frame instead of N -- bit i of a frame is bit (i % 8) of byte i / 8 (LSB first; what
 * SURVEY.md section 8d's byte model counts as a frame's output) -- an eighth of the bytes back over PCIe or out to the caller's HBM
 * buffer; the decoded values are those of the unpacked entry points.  llr_f16 = 1: d_llr / llr are IEEE binary16 patterns; 2: int8 LLRs (LDPC_I8 contexts only); 0: float32.  The decode
 * kernels write one byte per bit into the context's own staging buffer (max_batch x N bytes, allocated on first use) and a second
 * kernel packs them.  The reference returns `Vector Bool` (Arraylet2.hs:271-273): one value per bit, no counterpart. */
int ldpc_decode_batch_dev_packed(ldpc_ctx *ctx, int max_iters, int batch, const void *d_llr, int llr_f16, uint8_t *d_packed,
                                 int32_t *d_iters, uint8_t *d_converged, void *stream);
int ldpc_decode_batch_packed(ldpc_ctx *ctx, int max_iters, int batch, const void *llr, int llr_f16, uint8_t *packed,
                             int32_t *iters, uint8_t *converged);
/* SOFT OUTPUT: ldpc_decode_batch_dev with the decoder's LLRs out, for what follows a decoder in an iterative receiver (a demapper that
 * takes bit knowledge back in, an outer code, a reliability measure).  Served by the on-chip layered min-sum kernel for any H
 * (csrc/layered_csr.hip: LDPC_MINSUM, LDPC_SCHED_LAYERED, dtype LDPC_F16, LDPC_F32 or LDPC_I8, with or without cn_scale / cn_offset), in
 * whose layered schedule the lam cells ARE the posterior: the output is an epilogue of the frame, in instances of their own
 * (ldpc::layered_csr_soft_kernel<...>, what ldpc_ctx_kernel_name reports after this call; the other entry points launch what they launched).
 * Specification: tests/soft_output_spec.py, reproduced bit for bit.
 * All pointers are DEVICE pointers; enqueued on `stream`, not synchronised, ordered as ldpc_decode_batch_dev.  llr_fmt: LDPC_LLR_F32,
 * LDPC_LLR_F16 or (LDPC_I8 contexts only) LDPC_LLR_I8.  d_bits, d_iters, d_converged are EXACTLY those of the matching
 * ldpc_decode_batch_dev* call -- a frame out of sweeps still returns the channel's decisions there; d_iters, d_converged may be NULL.
 * d_soft [batch][N] of element type soft_fmt (LDPC_LLR_*), aligned to that element; soft_kind:
 *   LDPC_SOFT_POSTERIOR  P = lam as it stands when the frame stops, for EVERY frame: converged in sweep n -- lam after sweep n (final_lam
 *                        of ldpc_decode_batch_f64); out of sweeps -- lam after sweep max_iters (final_lam gives the channel LLRs there);
 *                        converged before the first sweep, or max_iters = 0 -- the channel LLRs as the cell took them in; an LDPC_F32
 *                        frame failed by the non-finite veto -- lam as it stands, which may hold an infinity or a NaN.
 *   LDPC_SOFT_EXTRINSIC  E = P - C, C the channel LLR as the cell took it in: fp16 cells, the LLR saturated and rounded to binary16 (a NaN
 *                        as +0); f32 cells, the float; int8 cells, the quantised integer q.  ONE float32 subtraction for float cells, an
 *                        integer subtraction for int8 cells.  What the decoder learned about a bit from all the others: the next
 *                        a-priori input of an iterative receiver.
 * Output formats.  Float cells: LDPC_LLR_F32 the value as it is; LDPC_LLR_F16 clamped to +-65504 and rounded to nearest even as the fp16
 * store of ldpc_demap_dev (for the posterior of an fp16 cell: the cell's own bits); LDPC_LLR_I8 clip(rint(v * soft_qscale), -127, 127),
 * a NaN as 0, soft_qscale 0 = 4.0 as in the demappers.  Int8 cells, integer v: LDPC_LLR_F32 fl(float(v) / llr_qscale), one division;
 * LDPC_LLR_F16 that float as above; LDPC_LLR_I8 clip(v, -127, 127), where soft_qscale must be 0 or the context's scale.
 * LDPC_EINVAL -- before the device is touched -- for a null d_soft, an unknown format or kind, a negative or non-finite soft_qscale (or one
 * that is not the context's, above), a d_soft misaligned for its element type.  LDPC_EUNSUPPORTED on a context of any other kernel
 * family; the message names the family that serves the context and the contexts that have a soft output. */
enum { LDPC_SOFT_POSTERIOR = 0, LDPC_SOFT_EXTRINSIC = 1 };
int ldpc_decode_batch_dev_soft(ldpc_ctx *ctx, int max_iters, int batch, const void *d_llr, int llr_fmt, uint8_t *d_bits, int32_t *d_iters,
                               uint8_t *d_converged, void *d_soft, int soft_fmt, float soft_qscale, int soft_kind, void *stream);
/* A DECODE THAT CONTINUES: the check-to-variable messages of a frame kept between calls, for a receiver that comes back to a frame with new
 * channel LLRs -- the next outer iteration of an iterative receiver (BICM-ID), the next HARQ round after combining -- or with the same ones
 * ("a few sweeps, look at the CRC, a few more").  Served by exactly the contexts that serve ldpc_decode_batch_dev_soft, in instances of their
 * own (ldpc::layered_csr_cont_kernel<...>, what ldpc_ctx_kernel_name reports after a continuing call; the other entry points launch what they
 * launched).  Specification: tests/decode_continue_spec.py, reproduced bit for bit.
 * THE STATE holds, per frame slot, the message on every edge -- as the kernel's row records {mag1, mag2, signs | arg-min}, in the geometry of
 * the context it was made for, so it is bound to that context -- and S, the sum of the check messages per column: float32 for LDPC_F16 and
 * LDPC_F32 cells, an integer in -254 .. 254 (int16) for LDPC_I8 cells.  Device bytes per slot: 12 nslab T + 4 N, or 8 nslab T + 2 N for
 * LDPC_I8 (nslab T: the context's rows, each barrier step rounded up to whole workgroups); ldpc_decode_state_bytes reports the total.  A reset
 * slot has all messages and S zero.  ldpc_decode_state_create returns a state of max_frames reset slots (NULL + LDPC_ENOMEM with the byte
 * count in the message); destroy it BEFORE its context -- a state that outlives its context can only be destroyed: every context, one created
 * later at the same address included, refuses it with LDPC_EINVAL, and so does a reset on the NULL stream.  ldpc_decode_state_reset zero-fills slots first .. first + count - 1: enqueued on
 * `stream` (NULL = the context's own), not synchronised.
 * ONE CALL, ldpc_decode_batch_dev_continue, decodes `batch` frames of channel LLRs; frame f uses slot first + f.  With C' the channel LLR as
 * the cell takes it in (as in ldpc_decode_batch_dev_soft):
 *   - the starting lam is fl32(C' + S) (LDPC_F32), that saturated and rounded to binary16 (LDPC_F16), clip(C' + S, -127, 127) (LDPC_I8);
 *   - the stopping rule before the first sweep is the syndrome of hard(that lam), not of the channel's decisions: a frame that had converged
 *     in the previous call and gets compatible LLRs stops with 0 sweeps;
 *   - the sweeps, the stop rule after a sweep, the LDPC_F32 non-finite veto and the context's check-node rule are unchanged, but the first
 *     sweep subtracts the stored messages;
 *   - d_bits, d_iters, d_converged follow ldpc_decode_batch_dev_soft with C' as "the channel": a frame out of sweeps or vetoed returns hard(C')
 *     and max_iters; the receiver's best guess is hard(P) of the soft output;
 *   - the soft output is optional (d_soft may be NULL): P = lam as it stands when the frame stops, E = P - C', formats as above;
 *   - the new state: S <- P - C' for every frame however it stopped, the messages as the last sweep left them (a frame that ran no sweep
 *     keeps its messages).
 * From a reset slot a call IS ldpc_decode_batch_dev_soft on the same LLRs, bit for bit -- except that a channel LLR of -0.0 enters as +0.0
 * (x + (+0) is x for every x but -0).  A split decode is NOT an unsplit one: n1 sweeps and then n2 more on the same LLRs are not n1 + n2 sweeps
 * in one call (fl(C + fl(P - C)) is not P, and the syndrome before the second call's first sweep can stop a frame that the "nothing moved" rule
 * would have sent round once more).  Non-finite values: see rule 3a above.
 * Ordering as ldpc_decode_batch_dev; calls on overlapping slots must be ordered by the caller.  LDPC_EINVAL -- before the device is touched --
 * for a null state, a state made for another context, first < 0, batch < 0, first + batch above the state's frames, and every argument error
 * of ldpc_decode_batch_dev_soft but the null d_soft.  LDPC_EUNSUPPORTED from create and from the call on a context of any other kernel
 * family; the message names the family that serves the context and the contexts that have the call. */
typedef struct ldpc_decode_state ldpc_decode_state;
ldpc_decode_state *ldpc_decode_state_create(ldpc_ctx *ctx, int max_frames);
void ldpc_decode_state_destroy(ldpc_decode_state *st);
int ldpc_decode_state_frames(const ldpc_decode_state *st);
size_t ldpc_decode_state_bytes(const ldpc_decode_state *st);
int ldpc_decode_state_reset(ldpc_decode_state *st, int first, int count, void *stream);
int ldpc_decode_batch_dev_continue(ldpc_ctx *ctx, ldpc_decode_state *st, int first, int max_iters, int batch, const void *d_llr, int llr_fmt,
                                   uint8_t *d_bits, int32_t *d_iters, uint8_t *d_converged, void *d_soft, int soft_fmt, float soft_qscale,
                                   int soft_kind, void *stream);
/* TWO DECODERS IN A ROW: a batch is decoded by a fast context, and only the frames it did not converge on are decoded again, FROM THE
 * CHANNEL LLRs, by a second one -- 3/4 min-sum on a quasi-cyclic on-chip kernel and then A-min* on the kernel for any H; int8 and then
 * f32; min-sum and then tanh; few sweeps and then many.  The failed frames are found, gathered, decoded and put back on the device, on one
 * stream, with no host round trip.  Specification: tests/cascade_spec.py.  No counterpart in the reference.
 * A cascade binds ctx1 (stage 1) and ctx2 (stage 2) to a capacity in 1 .. ctx2's max_batch: both on one device, codes of one N.  That the
 * two codes ARE one code -- a row-permuted, or quasi-cyclic against CSR, form of the same H -- is the caller's duty.  ctx1 == ctx2 is
 * allowed (the two decodes are ordered on one stream).  The cascade owns the compact LLR buffer (capacity x N x 4 bytes), stage 2's bits,
 * iters and flags, the index list and the buffers that stand in for NULL arguments; ldpc_cascade_bytes reports the total.  NULL +
 * LDPC_ENOMEM with the byte count in the message when that allocation fails.  Destroy it BEFORE its contexts; a cascade whose context was
 * destroyed refuses every call with LDPC_EINVAL.
 * ONE CALL, ldpc_cascade_decode_dev, decodes batch <= ctx1's max_batch frames; every pointer is DEVICE memory:
 *   1. stage 1: ctx1's ldpc_decode_batch_dev* of all the frames with max_iters1;
 *   2. idx = the frames with converged == 0 in ascending frame order, cut to the first `capacity` (a stable compaction: no atomic decides
 *      the order);
 *   3. stage 2: ctx2's ldpc_decode_batch_dev* of exactly those frames' channel LLRs with max_iters2;
 *   4. frames in idx take stage 2's bits, iters and flag ENTIRELY -- one that fails again returns what ctx2 returns for a failed frame --
 *      and d_stage = 2; every other frame, failed frames beyond `capacity` included, keeps stage 1's result and d_stage = 1;
 *   5. d_stats [3] = {frames that failed stage 1, frames sent to stage 2 = min(that, capacity), frames sent and still not converged}.
 * The count stays on the device, so stage 2 always decodes `capacity` rows: the rows past the count are padding with the LLR -1 (f32,
 * fp16 or int8), the all-zero word, on which every decoder stops before its first sweep.  capacity = batch never overflows; a smaller one
 * costs less padding.  d_llr [batch][N] of llr_fmt (LDPC_LLR_F32, LDPC_LLR_F16, LDPC_LLR_I8), aligned to its element; d_bits [batch][N];
 * d_iters, d_converged, d_stage [batch] and d_stats may each be NULL.  Enqueued on `stream` -- ctx2's decode too -- and NOT synchronised;
 * NULL = ctx1's own stream; ordering as ldpc_decode_batch_dev, and a cascade decodes one batch at a time.
 * LDPC_EINVAL -- before the device is touched -- for a null handle, N that differs between the contexts, contexts on different devices,
 * capacity out of range (create); a null cascade, a negative max_iters1 / max_iters2, batch < 0 or above ctx1's max_batch, an unknown
 * llr_fmt, a null d_llr / d_bits, a misaligned d_llr (the call); the message names the argument.  LDPC_LLR_I8 is LDPC_EUNSUPPORTED unless
 * BOTH contexts are LDPC_I8 -- checked up front, no call stops between its stages.  batch = 0 succeeds and touches nothing.
 * Not offered: soft output, packed bits and decode-state variants, more than two stages, and a stage 2 that continues from stage 1's
 * messages (the two stages need not be one kernel family). */
typedef struct ldpc_cascade ldpc_cascade;
ldpc_cascade *ldpc_cascade_create(ldpc_ctx *ctx1, ldpc_ctx *ctx2, int capacity);
void ldpc_cascade_destroy(ldpc_cascade *c);            /* before its contexts */
int ldpc_cascade_capacity(const ldpc_cascade *c);
size_t ldpc_cascade_bytes(const ldpc_cascade *c);
int ldpc_cascade_decode_dev(ldpc_cascade *c, int max_iters1, int max_iters2, int batch, const void *d_llr, int llr_fmt, uint8_t *d_bits, int32_t *d_iters,
                            uint8_t *d_converged, uint8_t *d_stage /* may be NULL */, uint32_t *d_stats /* [3], may be NULL */, void *stream);
/* page-locked host memory for the host-pointer entry points.  With llr AND bits buffers from ldpc_host_alloc (or
 * registered with hipHostRegister) ldpc_decode_batch runs zero-copy: the decode kernel itself reads the LLRs and
 * writes the bits over PCIe (10-11 Gbit/s PCIe-inclusive on jpl.4096); pageable buffers go through a chunked
 * H2D / decode / D2H pipeline at the pageable-copy rate (2-3.5 Gbit/s); up to 16 frames (ldpc_decode_one) take a
 * latency path through internal page-locked bounce buffers.  (The reference pokes pageable Storable vectors,
 * GPU/CUDA/Arraylet2.hs:158-159.)  NULL on failure. */
void *ldpc_host_alloc(size_t bytes);
void ldpc_host_free(void *p);
/* wait for everything enqueued on the context's stream */
int ldpc_ctx_synchronize(ldpc_ctx *ctx);

/* ---- coalescing of per-frame calls ----------------------------------------------------------------------
 * The reference's harness calls the decoder once per frame from up to maxThreadCount threads (Utils.hs:53,63-69) and
 * its CUDA plug-ins decode one codeword per launch sequence (Arraylet2.hs:151-273).  A batcher sits between such
 * callers and ONE decoder replica: the first caller to arrive waits until max_frames requests are queued or
 * max_wait_us have passed, decodes them with one launch and hands every caller its own result.  Thread-safe; each
 * call blocks like ldpc_decode_one and returns exactly what ldpc_decode_one would.  The context must not be used
 * directly while a batcher owns it; max_frames <= the context's max_batch. */
typedef struct ldpc_batcher ldpc_batcher;
ldpc_batcher *ldpc_batcher_create(ldpc_ctx *ctx, int max_frames, int max_wait_us);
void ldpc_batcher_destroy(ldpc_batcher *b);
int ldpc_batcher_decode_one(ldpc_batcher *b, int max_iters, const double *llr, uint8_t *bits, int *iters, int *converged);
int ldpc_batcher_stats(ldpc_batcher *b, long *calls, long *launches);

/* ---- verification entry points (used by tests/; not needed by a harness) ------------------------
 * One teacher-forced update on the device in the context's dtype: from the state (lam, ne) at
 * the top of loop turn n produce (ne', lam') exactly as Orig.hs:81-98 / Min.hs:75-104 would, and
 * report whether the syndrome of hard(lam) is zero (Orig.hs:73-78).  All arrays host, float64,
 * frame-major: orig/lam/lam_out [batch][N], ne/ne_out [batch][E] in ldpc_code_csr edge order. */
int ldpc_debug_step(ldpc_ctx *ctx, int batch, const double *orig, const double *lam, const double *ne,
                    double *ne_out, double *lam_out, uint8_t *syndrome_zero);
/* free-running decode that also returns lam at the top of every loop turn:
 * trace_lam [batch][max_iters+1][N] float64 (turns after a frame stopped are zero-filled). */
int ldpc_decode_trace(ldpc_ctx *ctx, int max_iters, int batch, const double *llr, uint8_t *bits,
                      int32_t *iters, uint8_t *converged, double *trace_lam);

/* ---- dominant-kernel timing (bench.py's `roofline` object) ---------------------------------------
 * When enabled, the context brackets every launch of its dominant kernel (fused: the one decode
 * kernel; HBM path: the one decode kernel of a QC code, the check-node kernel otherwise) with HIP events on the stream the
 * kernel is launched on.
 * ldpc_ctx_kernel_time drains them: number of launches and their summed duration (ms) since the
 * last call.  Blocks until the recorded launches have finished. */
int ldpc_ctx_set_timing(ldpc_ctx *ctx, int enabled);
int ldpc_ctx_kernel_time(ldpc_ctx *ctx, int *launches, double *total_ms);
/* name of that kernel as it appears in a rocprofv3 kernel trace (substring): the kernel family before the context's
 * first decode, narrowed to the launched template instance after it */
const char *ldpc_ctx_kernel_name(const ldpc_ctx *ctx);
/* launch geometry of that kernel after the first decode: threads per workgroup and frames one workgroup decodes (the
 * on-chip kernels and the frame-per-workgroup HBM kernels of QC codes); 0/0 for the batch-major HBM kernels */
int ldpc_ctx_kernel_geometry(const ldpc_ctx *ctx, int *threads_per_workgroup, int *frames_per_workgroup);

/* ---- run-time specialised kernels ------------------------------------------------------------------
 * The fused kernels take the graph as compile-time constants.  For the shipped matrices those instances are built
 * ahead of time; for any other single-circulant quasi-cyclic H (what the reference's QC decoders accept,
 * Fast/Arraylet.hs:68-79) ldpc_ctx_create compiles one the first time -- with the ROCm tool chain (hipcc --genco in a child
 * process) when it is installed, else in-process with hiprtc; LDPC_JIT_COMPILER=hipcc|hiprtc forces one -- and caches the
 * code object on disk (LDPC_JIT_CACHE, default jit_cache/ next to the library).  These entry points let a host warm that cache
 * ahead of time -- they need no GPU -- and look at what would be compiled.  LDPC_JIT=0 disables the mechanism
 * (table-driven / generic kernels are used instead). */
const char *ldpc_jit_cache_dir(void);
/* the generated translation unit for (code, variant, dtype): copies up to cap-1 bytes, returns its full length,
 * or a negative LDPC_E* (LDPC_EUNSUPPORTED with the reason when this code has no such kernel) */
long ldpc_jit_source(const ldpc_code *code, int variant, int dtype, char *buf, size_t cap);
/* compile into the cache (or find it there); kernel_name receives the symbol rocprofv3 will list */
int ldpc_jit_prepare(const ldpc_code *code, int variant, int dtype, char *kernel_name, size_t cap, int *from_cache,
                     double *seconds);
/* the same for a given schedule (ldpc_schedule).  What is specialised at run time: flooding f32 (min-sum, tanh), flooding
 * LDPC_F16PK (min-sum), and the on-chip layered kernels (min-sum; LDPC_F32 or LDPC_F16PK, layers = the block rows).  The two
 * functions above are these with LDPC_SCHED_FLOODING. */
long ldpc_jit_source_for(const ldpc_code *code, int variant, int dtype, int schedule, char *buf, size_t cap);
int ldpc_jit_prepare_for(const ldpc_code *code, int variant, int dtype, int schedule, char *kernel_name, size_t cap,
                         int *from_cache, double *seconds);

/* ---- frame source and error tally for a BER / throughput harness -----------------------------------
 * The reference leaves message generation, BPSK + AWGN and BER statistics to the external tester
 * (ecc-manifold `eccMain`, main/Main.hs:41-48); a harness built on this library can keep frames
 * on the device instead.  Encoding is the reference's systematic rule
 *   codeword = msg ++ take (c_length - k) (msg * G)   (Utils.hs:61, Reference/Orig.hs:25-26,
 * Fast/Encoder.hs:26-63).  G is given dense, row-major bytes [k][p] (0/1), or NULL for all-zero
 * codewords (codes shipped without a generator).  n_tx = transmitted length (c_length, Utils.hs:50);
 * positions n_tx..N-1 are punctured: LLR 0 (Utils.hs:55). */
typedef struct ldpc_sim ldpc_sim;
ldpc_sim *ldpc_sim_create(const ldpc_code *code, int k, int n_tx, int p, const uint8_t *G, int max_batch);
ldpc_sim *ldpc_sim_create_on(const ldpc_code *code, int device, int k, int n_tx, int p, const uint8_t *G, int max_batch);
void ldpc_sim_destroy(ldpc_sim *sim);
/* The generator in QUASI-CYCLIC form, encoded the way the reference's fast encoder does it (Fast/Encoder.hs:26-63:
 * the message cut into sz-bit words, parity word of block column c = XOR over block rows of mulWord = rotate-and-xor
 * over the set message bits).  circ [block_rows][block_cols][sz/32] = the integers of G.q as little-endian 32-bit words
 * (bit b = first-row entry of column b, QuasiCyclic.hs:19-25; ldpc_matrix_qc_words); k = sz * block_rows, parity length
 * sz * block_cols >= n_tx - k.  sz must be 32, 64, 128 or 256 as in the reference (Encoder.hs:28-33: LDPC_EUNSUPPORTED
 * otherwise -- use the dense form).  The device table is the 32 bit-rotations of each circulant
 * (block_rows * block_cols * sz words), never the expanded k x p matrix. */
ldpc_sim *ldpc_sim_create_qc_on(const ldpc_code *code, int device, int k, int n_tx, int sz, int block_rows, int block_cols,
                                const uint32_t *circ, int max_batch);
/* The encoder FROM H, for codes that have no generator file because they are defined by their parity-check matrix: k = N - M,
 * k <= n_tx <= N, positions n_tx..N-1 punctured as above; a quasi-cyclic code is taken as its CSR form.  H must qualify under
 * the rule of ldpc_csr_triangular_order: NULL with LDPC_EUNSUPPORTED and that function's reason otherwise.  Messages are random
 * (the same (seed, frame) -> message words as every other source); the parity bits are solved on the device, 32 frames to a
 * machine word.  Device scratch besides the packed messages and parity bits: at most 4 * N * ceil(max_batch / 32) bytes, and
 * never more than 2048 * N (larger batches pass through it in chunks of 16 384 frames). */
ldpc_sim *ldpc_sim_create_sparse_on(const ldpc_code *code, int device, int n_tx, int max_batch);
/* The encoder from ANY H, through the systematic form of ldpc_csr_systematic_form (its limit and refusals apply: NULL with that
 * function's code and reason): k = K = N - rank H, K <= n_tx <= N (LDPC_EINVAL otherwise), R = K / n_tx, positions n_tx..N-1
 * punctured as above whatever they carry; a quasi-cyclic code is taken as its CSR form.  Message bit i of the usual
 * (seed, frame) -> message words sits at codeword position msg_pos[i] (ldpc_sim_positions): d_msg is [batch][K] in msg_pos order,
 * ldpc_sim_encode_host returns the rank parity bits in par_pos order, ldpc_sim_tally counts message-bit errors at msg_pos.
 * Device memory besides the packed messages: 4 * ceil(N / 32) * max_batch bytes of packed codewords (no further scratch, so no
 * chunking: any batch <= max_batch is one pass) and a generator of 2048 * ceil(K / 32) bytes per 512 codeword positions from the
 * first parity position on. */
ldpc_sim *ldpc_sim_create_systematic_on(const ldpc_code *code, int device, int n_tx, int max_batch);
enum { LDPC_ENCODER_NONE = 0, LDPC_ENCODER_DENSE = 1, LDPC_ENCODER_QC = 2, LDPC_ENCODER_SPARSE = 3, LDPC_ENCODER_SYSTEMATIC = 4 };
int ldpc_sim_encoder(const ldpc_sim *sim);    /* which of these this frame source encodes with */
int ldpc_sim_message_length(const ldpc_sim *sim);     /* k of any source; K = N - rank H for LDPC_ENCODER_SYSTEMATIC */
/* where the message bits (msg_pos [k], may be NULL) and the parity bits (par_pos, may be NULL; N entries suffice) sit in the
 * codeword.  Returns the number of parity positions (< 0 on error).  LDPC_ENCODER_SYSTEMATIC: those of ldpc_csr_systematic_form;
 * every other source: 0..k-1 and k.. */
int ldpc_sim_positions(const ldpc_sim *sim, int32_t *msg_pos, int32_t *par_pos);
/* the encoder alone: codewords [batch][n_tx] bytes (device) of the same messages ldpc_sim_generate would use (message
 * bits of frame f depend on (seed, f) only); d_msg [batch][k] may be NULL.  Enqueued on `stream`. */
int ldpc_sim_encode_batch(ldpc_sim *sim, uint64_t seed, uint64_t first_frame, int batch, uint8_t *d_codewords, uint8_t *d_msg, void *stream);
/* frames [first_frame, first_frame+batch) of the stream identified by `seed`, at Eb/N0 (dB):
 * d_llr [batch][N] float32 (device), d_msg [batch][k] bytes (device, may be NULL).  Enqueued on
 * `stream` (NULL = the HIP default stream -- NOT a context's stream), not synchronised: pass the same
 * explicit stream to generate, decode and tally.  The message words stay inside `sim` for
 * the next ldpc_sim_tally call. */
int ldpc_sim_generate(ldpc_sim *sim, uint64_t seed, uint64_t first_frame, int batch, double ebn0_db,
                      float *d_llr, uint8_t *d_msg, void *stream);
/* same frames, LLRs written as fp16 (= the float32 values of ldpc_sim_generate, saturated to +-65504 and rounded
 * to nearest even) for ldpc_decode_batch_dev_f16 */
int ldpc_sim_generate_f16(ldpc_sim *sim, uint64_t seed, uint64_t first_frame, int batch, double ebn0_db,
                          uint16_t *d_llr, uint8_t *d_msg, void *stream);
/* ---- the caller's own messages.  Two layouts of bits in device memory:
 *   LDPC_BITS_BYTES   one byte per bit.  Input: only bit 0 of a byte is read; output: bytes are 0 or 1.  Messages [batch][k],
 *                     codewords [batch][n_tx] (what ldpc_sim_encode_batch writes).
 *   LDPC_BITS_PACKED  bit i of a row in byte i / 8 at bit i % 8 (the layout of ldpc_decode_batch_packed; read as little-endian
 *                     32-bit words, the library's own message words).  Message rows are 4 * ceil(k / 32) bytes -- whole words,
 *                     4-byte aligned (LDPC_EINVAL otherwise); bits >= k of the last word are ignored on input and 0 on output.
 *                     Codeword rows are ceil(n_tx / 8) bytes, any alignment; the pad bits of the last byte are written as 0.
 * Messages are in msg_pos order (ldpc_sim_positions): positions 0..k-1, but for LDPC_ENCODER_SYSTEMATIC.  All three functions take
 * device pointers, enqueue on `stream` and do not synchronise; inputs and outputs must not overlap; 1 <= batch <= max_batch.
 * LDPC_EINVAL: a null pointer, such a batch, an unknown format.  No counterpart in the reference. */
enum ldpc_bit_format { LDPC_BITS_BYTES = 0, LDPC_BITS_PACKED = 1 };
/* the encoder alone on the caller's messages: the codewords, cut at n_tx, that ldpc_sim_encode_batch would write had it drawn
 * these messages.  LDPC_EUNSUPPORTED on a source with LDPC_ENCODER_NONE (msg ++ zeros is not a codeword).  Packed codewords
 * come straight from the packed message and parity words for LDPC_ENCODER_QC, _SPARSE and _SYSTEMATIC; LDPC_ENCODER_DENSE writes
 * bytes into a staging buffer of max_batch * n_tx bytes inside `sim`, allocated by the first such call (a device allocation: that one
 * call may wait for the device), and a second kernel packs them: n_tx bytes written and read again per frame. */
int ldpc_sim_encode_messages(ldpc_sim *sim, int batch, const void *d_msg, int msg_fmt, void *d_codewords, int cw_fmt, void *stream);
/* the frames of ldpc_sim_generate (llr_f16 = 0: float32 LLRs [batch][N]) or ldpc_sim_generate_f16 (llr_f16 = 1) with the caller's
 * messages in place of the drawn ones: the noise of frame first_frame + f is the same stream of (seed, frame) -- it never
 * depended on the message -- sigma comes from R = k / n_tx, positions >= n_tx get LLR 0.  Given exactly the messages
 * ldpc_sim_generate would draw, the LLRs are bit for bit those of ldpc_sim_generate.  LDPC_EUNSUPPORTED as above.  After this
 * call, and after ldpc_sim_encode_messages, the caller's messages are what ldpc_sim_tally compares against. */
int ldpc_sim_generate_from(ldpc_sim *sim, uint64_t seed, uint64_t first_frame, int batch, double ebn0_db, const void *d_msg, int msg_fmt,
                           void *d_llr, int llr_f16, void *stream);
/* ---- higher-order modulation: a labelled constellation, a max-log soft demapper, and the frame source's modulated path.
 * Modulation object (host only): 2^m points (I, Q), m = 1..6 bits per symbol as a table (product constellations, below, reach
 * m = 12).  LABELLING: symbol s of a frame carries codeword bits
 * m s .. m s + m - 1; its label is sum_j bit(m s + j) << (m - 1 - j) -- the first bit is the MSB -- and the label is the index into
 * `points`.  Bits at positions >= n_tx pad as 0.  The bits are taken in codeword order; any other order is a bit interleaver
 * (ldpc_interleaver, below) and the _il entry points.  Two equal points are allowed.
 * LDPC_EINVAL and NULL for m outside 1..6, a null table or a non-finite point.
 * Built-ins, by formula (NO claim is made that these are any standard's labellings or, for APSK, ring ratios -- a caller who needs a
 * standard's constellation passes its own table):
 *   LDPC_MOD_BPSK   bit b -> (2b - 1, 0): LLR > 0 <=> bit 1, as everywhere in this library
 *   LDPC_MOD_QPSK   (b0, b1) -> ((2 b0 - 1), (2 b1 - 1)) / sqrt 2: Gray
 *   LDPC_MOD_8PSK   unit circle, the point at angle k pi / 4 carries label k ^ (k >> 1): Gray around the circle
 *   LDPC_MOD_16QAM  (b0 b1 | b2 b3) -> (L[b0 b1], L[b2 b3]) / sqrt 10, L: 00 01 11 10 -> -3 -1 +1 +3: Gray per axis, unit energy */
typedef struct ldpc_modulation ldpc_modulation;
enum { LDPC_MOD_BPSK = 1, LDPC_MOD_QPSK = 2, LDPC_MOD_8PSK = 3, LDPC_MOD_16QAM = 4,
       LDPC_MOD_64QAM = 6, LDPC_MOD_256QAM = 8, LDPC_MOD_1024QAM = 10, LDPC_MOD_4096QAM = 12 };   /* the kind number is m */
ldpc_modulation *ldpc_modulation_create(int bits_per_symbol /* m, 1..6 */, const float *points /* [2^m][2]: I, Q */);
ldpc_modulation *ldpc_modulation_create_builtin(int kind);
void ldpc_modulation_destroy(ldpc_modulation *mod);
int ldpc_modulation_bits(const ldpc_modulation *mod);                /* m */
int ldpc_modulation_points(const ldpc_modulation *mod, float *out);  /* [2^m][2] (out may be NULL); returns 2^m */
double ldpc_modulation_energy(const ldpc_modulation *mod);           /* Es = mean |c|^2, accumulated in double in index order */
int ldpc_modulation_symbols(const ldpc_modulation *mod, int n_tx);   /* symbols per frame: ceil(n_tx / m) */
/* PRODUCT constellations, up to 4096 points: an I-axis level set times a Q-axis level set, b = 1..6 bits an axis, m = 2 b bits per
 * symbol.  The labelling rule above holds; of a symbol's m bits the first b (MSB first) are the index into levels_i and the next b the
 * index into levels_q: label = (iI << b) | iQ, and the point of that label is (levels_i[iI], levels_q[iQ]).  The two axes may hold
 * different level sets; non-uniform levels and unequal I/Q scaling are allowed.  Different bits per axis are not provided.  A labelling that
 * interleaves I and Q bits is a bit interleaver's table (ldpc_interleaver, below).  LDPC_EINVAL and NULL for b outside 1..6, a null table or a non-finite level.
 * For such an object
 *   ldpc_modulation_bits    returns 2 b;
 *   ldpc_modulation_points  returns 4^b and writes the materialised table pt[(iI << b) | iQ] = (levels_i[iI], levels_q[iQ]);
 *   ldpc_modulation_energy  is the rule above on that table (double, index order): for b <= 3 bit for bit the Es, and so the sigma, of
 *                           the same table passed to ldpc_modulation_create;
 *   ldpc_demap_dev          separates the max-log rule per axis: for the coordinate y of axis A with levels a_l
 *                             e_l = (y - a_l)^2;  LLR_j = (min over axis labels with bit j = 0 of e_l - min over those with bit j = 1) / (2 noise_var)
 *                           in float32, operation by operation as tests/product_modulation_spec.py states it (bit for bit).  Output
 *                           element m s + j is I-bit j of symbol s, element m s + b + j its Q-bit j.  This is the max-log rule on the
 *                           4^b points -- the other axis's smallest distance adds to both mins and cancels -- at 2 * 2^b distances a
 *                           sample; against ldpc_demap_dev on the materialised table (b <= 3) it differs by the roundings of that
 *                           cancelled term only.  A NaN coordinate makes the b LLRs of ITS axis NaN (int8: 0) and leaves the other
 *                           axis's LLRs as they are (the table rule makes all m NaN);
 *   ldpc_sim_transmit       gives bit for bit the symbols of the materialised table (b <= 3: of that table object).
 * Built-ins LDPC_MOD_64QAM, _256QAM, _1024QAM, _4096QAM (b = 3, 4, 5, 6; product objects), both axes: position k = 0 .. 2^b - 1 has
 * amplitude (2k - (2^b - 1)) / sqrt(2 (4^b - 1) / 3) and carries the axis label k ^ (k >> 1) (binary-reflected Gray); each level is
 * computed in double and rounded to float32 once; unit energy.  For b = 2 that is the level set of LDPC_MOD_16QAM, which stays a table
 * object.  As above, no claim that these are any standard's labellings. */
ldpc_modulation *ldpc_modulation_create_product(int bits_per_axis /* b, 1..6 */, const float *levels_i /* [2^b] */, const float *levels_q /* [2^b] */);
/* b and the two level sets of a product object ([2^b] each; either pointer may be NULL); 0, and nothing written, for a table object */
int ldpc_modulation_axis_levels(const ldpc_modulation *mod, float *levels_i, float *levels_q);
/* Max-log soft demapper on the device: d_sym [batch][n_sym][2] float32 I/Q samples (8-byte aligned), n_sym = ceil(n_tx / m) ->
 * d_llr [batch][N] in one of the decoders' input formats, one pass.  For a sample y and every point c_p:
 *   d_p = |y - c_p|^2;  LLR_j = (min over labels with bit j = 0 of d_p  -  min over labels with bit j = 1 of d_p) / (2 noise_var)
 * in float32, operation by operation as tests/modulation_spec.py states it (the kernel reproduces that bit for bit).  noise_var is
 * sigma^2 per real dimension, finite and > 0, and 1 / (2 noise_var) must fit a float32 (noise_var above about 1.5e-39; LDPC_EINVAL
 * otherwise).  Positions n_tx .. N-1 are written as 0; LLRs of pad bits are not written.
 *   LDPC_LLR_F32  the value;  LDPC_LLR_F16  clamped to +-65504, rounded to nearest even (what ldpc_sim_generate_f16 does);
 *   LDPC_LLR_I8   clip(rint(LLR * qscale), -127, 127), NaN -> 0: the quantiser of an LDPC_I8 context with llr_qscale = qscale, so
 *                 ldpc_decode_batch_dev_i8 decodes these bytes as ldpc_decode_batch_dev would have quantised the floats.  qscale is
 *                 read for LDPC_LLR_I8 only; 0 = 4.0; negative or non-finite: LDPC_EINVAL.
 * A NaN sample gives NaN LLRs (int8: 0, an erasure).  Runs on the calling thread's device, enqueued on `stream`, not synchronised.
 * LDPC_EINVAL: a null pointer, batch <= 0, n_tx <= 0 or > N, an unknown format, such a noise_var or qscale, a misaligned buffer.
 * fp16 samples are not provided; the exact log-MAP rule is a property of the modulation object (THE LLR RULE, below); a bit interleaver
 * between codeword order and transmitted order is ldpc_demap_dev_il, below. */
enum { LDPC_LLR_F32 = 0, LDPC_LLR_F16 = 1, LDPC_LLR_I8 = 2 };   /* the values llr_f16 takes in the packed entry points */
int ldpc_demap_dev(const ldpc_modulation *mod, int batch, int n_tx, int N, const float *d_sym, double noise_var, void *d_llr, int llr_fmt,
                   float qscale, void *stream);
/* THE LLR RULE travels with the modulation object: every demapper entry point (ldpc_demap_dev, _il, _il_csi, _rm) picks it up and none
 * takes a new argument.  LDPC_DEMAP_MAXLOG is the rule stated above, and the rule of every object created any other way.
 * LDPC_DEMAP_LOGMAP is the exact rule.  For one sample and label bit j let d_p be the SAME float32 squared distances the max-log rule
 * computes, from the same operations in the same order, m0 / m1 their minima over the points whose bit j is 0 / 1, and inv_s the
 * symbol's float32(1 / (2 noise_var)) (times its gain where one is given: ldpc_demap_dev_il_csi).  Then
 *   LLR_j = fl(fl(m0 - m1) inv_s)  +  (c1 - c0),   c_v = log(sum over the points p whose bit j is v of exp(-(d_p - m_v) inv_s))
 * The first term is the max-log value, unchanged; c_v lies in [0, log 2^(m-1)], and every sum holds an exp(0) = 1, so nothing
 * underflows to log 0 at any SNR.  For a product object the rule is applied per axis (2^b levels, the bits of that axis, e_l in place
 * of d_p): exact, not an approximation, because the other axis's factor is common to both subsets and cancels.  The rule is restated
 * in tests/demap_logmap_spec.py; the kernels evaluate exp and log with the hardware's base-2 instructions and stay within 2^-14 of
 * it, plus two float32 ulps of the result.  Where c1 - c0 is zero the max-log value stands as it is, the sign of a zero included, so
 *   one point a subset (m = 1; b = 1 per axis): the max-log result bit for bit;
 *   high SNR, every (d_p - m_v) inv_s but the smallest above 104: every other term is 0 in float32 -- the max-log result bit for bit;
 *   inv_s = 0 (a gain of 0): both sums are the same integer -- the max-log result, a zero;
 *   a NaN sample or gain: NaN for exactly the elements that are NaN under max-log; an infinite coordinate: NaN (inf - inf), as there.
 * The output formats, the interleaver, the gains and the sums of ldpc_demap_dev_rm treat the value as they treat a max-log one.
 * COST: m 2^m exponentials a sample for a table object, 2 b 2^b for a product object; ldpc_demap_dev_rm, which evaluates a bit a lane,
 * 2^m (2^b) a bit.
 * ldpc_modulation_with_rule: a NEW object (destroy it as any other) with the constellation of `mod`, table or product, demapped by
 * `rule`; `mod` is untouched.  NULL and LDPC_EINVAL for a null `mod` or any other rule value.  An LDPC_DEMAP_MAXLOG copy is selected and
 * computed exactly as the object it came from.  The transmit-only calls (ldpc_sim_transmit*) ignore the rule.  The fused map + noise +
 * demap calls (ldpc_sim_generate_mod, _il, _il_fading) return LDPC_EUNSUPPORTED for an LDPC_DEMAP_LOGMAP object, the message naming the
 * rule: fusing them doubles the instance count of five more kernels and is left for later; the two-step route (ldpc_sim_transmit*,
 * then a demapper) gives the same LLRs and serves every sweep in the meantime. */
typedef enum { LDPC_DEMAP_MAXLOG = 0, LDPC_DEMAP_LOGMAP = 1 } ldpc_demap_rule;
ldpc_modulation *ldpc_modulation_with_rule(const ldpc_modulation *mod, int rule);
int ldpc_modulation_rule(const ldpc_modulation *mod);   /* LDPC_DEMAP_MAXLOG for every object created any other way */
/* The frame source's modulated path.  sigma^2 per real dimension = Es / (2 R m 10^(dB/10)), R = k / n_tx, in double (for
 * LDPC_MOD_BPSK: the formula of ldpc_sim_generate). */
double ldpc_sim_noise_var(const ldpc_sim *sim, const ldpc_modulation *mod, double ebn0_db);
/* frames [first_frame, first_frame + batch): the codewords of the drawn messages (d_msg_in NULL; those of ldpc_sim_generate) or of
 * the caller's (d_msg_in, msg_fmt: as ldpc_sim_generate_from; LDPC_EUNSUPPORTED on LDPC_ENCODER_NONE), mapped to symbols and sent
 * through complex AWGN: d_sym [batch][n_sym][2] float32, 8-byte aligned, y = c + sigma z per coordinate.  NOISE: symbol pair g =
 * symbols 2g and 2g + 1 takes one Philox call with counter (frame lo, frame hi, g, stream 2) and the Box-Muller of
 * ldpc_sim_generate: (r0, r1) -> I, Q of symbol 2g, (r2, r3) -> I, Q of symbol 2g + 1.  Streams 0 (messages) and 1 (the BPSK
 * source's noise) are untouched.  d_msg [batch][k] bytes may be NULL.  The codewords are encoded into a packed buffer of
 * max_batch * ceil(n_tx / 8) bytes inside `sim`, allocated by the first such call (LDPC_ENCODER_DENSE and _NONE also use the staging
 * buffer of ldpc_sim_encode_messages).  1 <= batch <= max_batch.  The message words stay inside `sim` for ldpc_sim_tally.
 * An Eb/N0 so high that sigma^2 underflows to 0 is accepted here (the symbols are then the constellation points); a NaN Eb/N0 is
 * LDPC_EINVAL. */
int ldpc_sim_transmit(ldpc_sim *sim, const ldpc_modulation *mod, uint64_t seed, uint64_t first_frame, int batch, double ebn0_db,
                      const void *d_msg_in, int msg_fmt, float *d_sym, uint8_t *d_msg, void *stream);
/* ldpc_sim_transmit and ldpc_demap_dev(.., ldpc_sim_noise_var(..), ..) in ONE kernel: the samples never reach memory, and the LLRs
 * d_llr [batch][N] (llr_fmt, qscale: as ldpc_demap_dev) are bit for bit those of the two calls.  Unlike ldpc_sim_transmit it needs
 * sigma^2 > 0 with 1 / (2 sigma^2) inside a float32 (Eb/N0 below about 380 dB): LDPC_EINVAL otherwise.
 * NOTE on LDPC_MOD_BPSK: this path computes ((y + 1)^2 - (y - 1)^2) / (2 sigma^2), which is not bitwise ldpc_sim_generate's
 * (2 / sigma^2) (x + sigma z), and it draws its noise from stream 2.  It is not a replacement for ldpc_sim_generate.
 * Max-log only: LDPC_EUNSUPPORTED for an LDPC_DEMAP_LOGMAP object (THE LLR RULE, above), as ldpc_sim_generate_mod_il and
 * ldpc_sim_generate_mod_il_fading; use ldpc_sim_transmit* and a demapper. */
int ldpc_sim_generate_mod(ldpc_sim *sim, const ldpc_modulation *mod, uint64_t seed, uint64_t first_frame, int batch, double ebn0_db,
                          const void *d_msg_in, int msg_fmt, void *d_llr, int llr_fmt, float qscale, uint8_t *d_msg, void *stream);
/* ---- bit interleaver: a position table between codeword order and transmitted order, fused into the mapper and the demapper.
 * Transmitted bit t is codeword bit pos[t], t = 0 .. n_tx - 1; symbol s carries transmitted bits m s .. m s + m - 1, the first one the
 * MSB of its label, exactly the labelling rule above (bits t >= n_tx of the last symbol pad as 0).  pos is injective into 0 .. N - 1,
 * 1 <= n_tx <= N.  Codeword positions that no pos[t] names are PUNCTURED, anywhere in the codeword: they are not sent and their LLR
 * is 0.  The identity table (n_tx entries) is the behaviour of the entry points without _il, bit for bit.
 * The object holds pos, and the sorted list of the N - n_tx punctured positions, in device memory on `device`.  The arguments are
 * checked before the device is touched: LDPC_EINVAL and NULL for a null table, n_tx < 1 or n_tx > N, an entry outside 0 .. N - 1, a
 * repeated entry; only then LDPC_ENODEVICE (device < 0, no such device) or LDPC_EHIP.
 * An I/Q-alternating labelling of a product constellation of b bits an axis (m = 2 b) is the table
 *   pos'[m s + 2 j] = pos[m s + j],  pos'[m s + 2 j + 1] = pos[m s + b + j],  j = 0 .. b - 1,
 * of any table pos with m | n_tx (the identity included). */
typedef struct ldpc_interleaver ldpc_interleaver;
ldpc_interleaver *ldpc_interleaver_create_on(int device, int n_tx, int N, const int32_t *pos /* [n_tx] */);
void ldpc_interleaver_destroy(ldpc_interleaver *il);
int ldpc_interleaver_dims(const ldpc_interleaver *il, int *n_tx, int *N);            /* either pointer may be NULL */
int ldpc_interleaver_positions(const ldpc_interleaver *il, int32_t *pos /* [n_tx], may be NULL */);   /* returns n_tx */
/* The block interleaver's table, by formula, on the host (no device; NO claim is made that it is any standard's table): codeword bit
 * i = c rows + u is written into column c of a rows x cols matrix at row (u + twist[c]) mod rows, and the matrix is read row by row,
 * taking the columns in the order order[0 .. cols - 1]:
 *   pos[r cols + j] = c rows + ((r - twist[c]) mod rows),  c = order[j].
 * twist NULL = no twist, order NULL = the identity.  With cols = m, symbol r takes one bit from each column.  LDPC_EINVAL for rows < 1,
 * cols < 1, rows * cols overflowing an int, a twist outside 0 .. rows - 1, an order that is not a permutation of 0 .. cols - 1, a null pos. */
int ldpc_interleaver_block_positions(int rows, int cols, const int32_t *twist /* [cols] or NULL */, const int32_t *order /* [cols] or NULL */,
                                     int32_t *pos /* [rows * cols] */);
/* ldpc_demap_dev through the table, in one kernel with no memset before it: per symbol exactly the rule of ldpc_demap_dev; the LLR of
 * transmitted bit t goes to element pos[t] of its row of d_llr [batch][N], the punctured positions get 0, LLRs of pad bits are not
 * written: every element is written exactly once.  n_tx and N are the table's; d_sym [batch][ceil(n_tx / m)][2].  LDPC_EINVAL as
 * ldpc_demap_dev, and for a null `il` or one that lives on another device than the calling thread's.  A block table of m columns keeps
 * the stores of a wave consecutive per bit index; a random table scatters single elements. */
int ldpc_demap_dev_il(const ldpc_modulation *mod, const ldpc_interleaver *il, int batch, const float *d_sym, double noise_var, void *d_llr,
                      int llr_fmt, float qscale, void *stream);
/* ldpc_sim_transmit with the label of symbol s gathered from codeword bits pos[m s + j]; the noise (Philox counters, Box-Muller, stream
 * 2), sigma (R = k / n_tx) and the symbol rule are untouched.  The table's n_tx and N must be the frame source's n_tx and its code's N,
 * every pos[t] must be < n_tx (the source's codewords are cut at n_tx: the table is a permutation of the transmitted prefix) and it
 * must live on the source's device: LDPC_EINVAL otherwise, and for a null `il`. */
int ldpc_sim_transmit_il(ldpc_sim *sim, const ldpc_modulation *mod, const ldpc_interleaver *il, uint64_t seed, uint64_t first_frame, int batch,
                         double ebn0_db, const void *d_msg_in, int msg_fmt, float *d_sym, uint8_t *d_msg, void *stream);
/* ldpc_sim_transmit_il and ldpc_demap_dev_il(.., ldpc_sim_noise_var(..), ..) in ONE kernel, bit for bit; otherwise as
 * ldpc_sim_generate_mod, which it equals bit for bit with the identity table. */
int ldpc_sim_generate_mod_il(ldpc_sim *sim, const ldpc_modulation *mod, const ldpc_interleaver *il, uint64_t seed, uint64_t first_frame, int batch,
                             double ebn0_db, const void *d_msg_in, int msg_fmt, void *d_llr, int llr_fmt, float qscale, uint8_t *d_msg, void *stream);
/* The table alone, for a caller's own modulator or demapper (device pointers, the calling thread's device = the table's, enqueued on
 * `stream`, not synchronised; inputs and outputs must not overlap).
 * ldpc_interleave_bits_dev: codewords [batch][N] as LDPC_BITS_BYTES or LDPC_BITS_PACKED (rows of ceil(N / 8) bytes) -> transmitted
 * bits [batch][n_tx] in either format (rows of ceil(n_tx / 8) bytes, pad bits 0), bit t = codeword bit pos[t].
 * ldpc_deinterleave_llr_dev: d_llr_tx [batch][n_tx] in transmitted order -> d_llr [batch][N], element pos[t] = element t, 0 at the
 * punctured positions; the same element type (llr_fmt) in and out, nothing is requantised. */
int ldpc_interleave_bits_dev(const ldpc_interleaver *il, int batch, const void *d_codewords, int cw_fmt, void *d_tx_bits, int tx_fmt, void *stream);
int ldpc_deinterleave_llr_dev(const ldpc_interleaver *il, int batch, const void *d_llr_tx, void *d_llr, int llr_fmt, void *stream);
/* ---- fading channels and per-symbol channel state, in the interleaved family (the identity table is "no interleaver").  A coherent
 * receiver with perfect channel knowledge is modelled: the phase is taken out and the samples are delivered EQUALISED, so of the channel
 * only the POWER gain a of a symbol appears: the noise variance per real dimension of its sample is noise_var / a.  The rules are
 * restated in float32, one operation at a time, in tests/fading_spec.py; the kernels reproduce them bit for bit.
 *
 * ldpc_demap_dev_il_csi: ldpc_demap_dev_il with d_gain [batch][n_sym] float32 (4-byte aligned), the power gain of every symbol.
 * inv = float32(1 / (2 noise_var)) as there, inv_s = fl(inv a), and the LLRs of symbol s are exactly ldpc_demap_dev_il's rule with
 * inv_s in place of inv: a table object fl(fl(m0_j - m1_j) inv_s), a product object the per-axis form.  Everything else -- positions
 * through the table, zeros at the punctured positions, pad bits, the formats, every element written once, no memset -- is
 * ldpc_demap_dev_il's, and a = 1 everywhere gives its output bit for bit.  With a finite sample a = 0 gives zero LLRs (an erasure) and
 * a NaN gain NaN LLRs (int8: 0).  A negative gain is the caller's error and is not looked for: the gains are device data.
 * LDPC_EINVAL as ldpc_demap_dev_il, and for a null or misaligned d_gain, all before the device is touched. */
int ldpc_demap_dev_il_csi(const ldpc_modulation *mod, const ldpc_interleaver *il, int batch, const float *d_sym /* [batch][n_sym][2] */,
                          const float *d_gain /* [batch][n_sym] */, double noise_var, void *d_llr, int llr_fmt, float qscale, void *stream);
/* THE DEMAPPER WITH A-PRIORI INPUT (csrc/demap_apriori.hip; restated in tests/demap_apriori_spec.py): ldpc_demap_dev_il_csi with bit
 * knowledge, for a receiver that iterates between demapper and decoder (BICM-ID).  d_apriori [batch][N] float32 (4-byte aligned), in
 * CODEWORD order, holds an LLR for every codeword bit -- log P(1) / P(0), positive means bit 1, the library's sign: the extrinsic output
 * of ldpc_decode_batch_dev_soft is one, zeros are none.  d_gain may be NULL: a = 1.  Table objects, m = 1..6.  Everything not named here
 * is ldpc_demap_dev_il_csi's: positions through the table, 0 at the punctured positions, pad bits not written, every element written
 * exactly once, no memset, the three output formats.  The lane of a symbol gathers its m a-priori values through the m table entries it
 * stores through: a-priori values at punctured positions are never read; the pad bits of a ragged last symbol have La = 0.
 * THE RULE, all float32, one operation at a time, nothing fused.  d_p the squared distances of THE LLR RULE, inv_s as above.
 *   a_p = the sum of La_j over the set label bits j of p, MSB first, left to right (a_0 = +0; one set bit: La_j itself)
 *   u_p = fl(a_p - fl(d_p inv_s));  U1_j, U0_j = the max of u_p over the labels whose bit j is 1, 0
 *   max-log:  LLR_j = fl(fl(U1_j - U0_j) - La_j) -- the EXTRINSIC value: the bit's own knowledge is taken out again
 *   log-MAP (an LDPC_DEMAP_LOGMAP object):  fl(U1_j - U0_j) + (c1 - c0) - La_j, c_v = log(sum over the subset, in label order, of
 *             exp(u_p - U_v)); a zero correction leaves the max-log term as it is, as in THE LLR RULE
 * With La = 0 everywhere the result is ldpc_demap_dev_il_csi's up to rounding, not bit for bit -- fl(m0 inv_s) - fl(m1 inv_s) against
 * fl(fl(m0 - m1) inv_s): within 2^-21 (m0 + m1) inv_s.
 * LDPC_EUNSUPPORTED for a product object: its Gray-like per-axis labels gain little from iteration.  LDPC_EINVAL as ldpc_demap_dev_il_csi
 * (a null d_gain excepted), for a null or misaligned d_apriori, and for a d_apriori that overlaps d_llr; all before the device is
 * touched.  A NaN a-priori value is the caller's error; the other frames of the batch are not affected by it. */
int ldpc_demap_dev_il_apriori(const ldpc_modulation *mod, const ldpc_interleaver *il, int batch, const float *d_sym /* [batch][n_sym][2] */,
                              const float *d_gain /* [batch][n_sym] or NULL */, double noise_var, const float *d_apriori /* [batch][N] */, void *d_llr,
                              int llr_fmt, float qscale, void *stream);
/* The channel.  Symbol s of a frame lies in block q = s / block, and all symbols of a block share one gain (block >= n_sym: one gain
 * per frame; block = 1: independent per symbol).  DRAW: block pair Q = blocks 2Q and 2Q + 1 takes one Philox call with counter
 * (frame lo, frame hi, Q, stream 3) and key = seed, and the Box-Muller of the noise: (z0, z1) -> block 2Q, (z2, z3) -> block 2Q + 1.
 * Streams 0, 1 and 2 are untouched.  GAIN: with mu = float32(sqrt(K / (K + 1))) and sd = float32(sqrt(1 / (2 (K + 1)))), computed in
 * double and rounded once (K = k_factor, the Rician factor, linear; 0 = Rayleigh),
 *   hI = fl(mu + fl(sd z0)),  hQ = fl(sd z1),  a = max(fl(fl(hI hI) + fl(hQ hQ)), 2^-20).
 * The floor keeps a sample finite when the Box-Muller radius is 0.  E[a] = 1, so ldpc_sim_noise_var and the meaning of Eb/N0 (the
 * average) are unchanged.  SAMPLE: sg_s = fl(sg / fl(sqrt a)), y = fl(c + fl(sg_s z)) per coordinate with sg and the stream-2 normal z
 * of ldpc_sim_transmit_il; a = 1 gives the AWGN rule.  Doppler-correlated gains, imperfect channel knowledge, fp16 samples and entry
 * points without a table are not provided. */
typedef struct {
    size_t struct_size; /* sizeof(ldpc_fading) */
    int block;          /* symbols per fading block, >= 1 */
    float k_factor;     /* Rician K, linear, finite, >= 0; 0 = Rayleigh */
} ldpc_fading;
/* ldpc_sim_transmit_il over that channel: d_sym as there; d_gain [batch][n_sym] float32 (4-byte aligned) receives the gains and may be
 * NULL.  Everything else -- the labels through the table, the packed codeword buffer, the caller's messages, the words kept for
 * ldpc_sim_tally, the refusals -- is ldpc_sim_transmit_il's.  LDPC_EINVAL also for a null `fad`, a struct_size that does not cover the
 * three fields, block < 1, a negative or non-finite k_factor, a misaligned d_gain. */
int ldpc_sim_transmit_il_fading(ldpc_sim *sim, const ldpc_modulation *mod, const ldpc_interleaver *il, const ldpc_fading *fad, uint64_t seed,
                                uint64_t first_frame, int batch, double ebn0_db, const void *d_msg_in, int msg_fmt, float *d_sym,
                                float *d_gain /* [batch][n_sym], may be NULL */, uint8_t *d_msg, void *stream);
/* ldpc_sim_transmit_il_fading and ldpc_demap_dev_il_csi(.., ldpc_sim_noise_var(..), ..) in ONE kernel, bit for bit: neither samples
 * nor gains need reach memory; a non-null d_gain receives the gains ldpc_sim_transmit_il_fading would have written, bit for bit.
 * Otherwise as ldpc_sim_generate_mod_il. */
int ldpc_sim_generate_mod_il_fading(ldpc_sim *sim, const ldpc_modulation *mod, const ldpc_interleaver *il, const ldpc_fading *fad, uint64_t seed,
                                    uint64_t first_frame, int batch, double ebn0_db, const void *d_msg_in, int msg_fmt, void *d_llr, int llr_fmt,
                                    float qscale, float *d_gain /* [batch][n_sym], may be NULL */, uint8_t *d_msg, void *stream);
/* ---- rate matching and HARQ soft combining: a position table whose entries MAY REPEAT, and a demapper that SUMS through it, optionally
 * onto the soft buffer of earlier transmissions.  The injective table stays the interleaver above, and every entry point above keeps its
 * rule and its bits.  The rule is restated in float32, one operation at a time, in tests/ratematch_spec.py; the kernels reproduce it bit
 * for bit.
 * TABLE: transmitted bit t is codeword bit pos[t], t = 0 .. E - 1; symbol s carries transmitted bits m s .. m s + m - 1 by the labelling
 * rule above (bits t >= E of the last symbol pad as 0).  pos is ANY map into 0 .. N - 1: entries may repeat, and E may be below, at or
 * above N (a circular buffer read for E > N bits repeats bits).  1 <= E <= 2^31 - 1 - 32, and batch * max(E, N) of a call may be at most
 * 2^32 - 256, what one launch holds (LDPC_EINVAL otherwise).  Positions that no entry names are NOT SENT in this round.
 * The object holds, in device memory on `device`, pos and its INVERSE in CSR form: for every position c the transmitted indices t with
 * pos[t] = c, in ASCENDING order -- the order of the float additions below.  The arguments are checked before the device is touched:
 * LDPC_EINVAL and NULL for a null table, E < 1, N < 1 or an entry outside 0 .. N - 1; only then LDPC_ENODEVICE (device < 0, no such
 * device) or LDPC_EHIP.  ldpc_ratematch_fanin: count[c] = how many t name position c (they sum to E). */
typedef struct ldpc_ratematch ldpc_ratematch;
ldpc_ratematch *ldpc_ratematch_create_on(int device, int E, int N, const int32_t *pos /* [E] */);
void ldpc_ratematch_destroy(ldpc_ratematch *rm);
int ldpc_ratematch_dims(const ldpc_ratematch *rm, int *E, int *N);                    /* either pointer may be NULL */
int ldpc_ratematch_positions(const ldpc_ratematch *rm, int32_t *pos /* [E], may be NULL */);   /* returns E */
int ldpc_ratematch_fanin(const ldpc_ratematch *rm, int32_t *count /* [N] */);
/* The circular-buffer table, by formula, on the host (no device; NO claim is made that it is any standard's table):
 *   pos[t] = buf[(start + t) mod n_buf],  t = 0 .. E - 1,
 * buf [n_buf] the buffer's codeword positions in its order (a caller leaves out punctured or filler positions and reorders here), NULL =
 * the identity 0 .. n_buf - 1; start = the offset of the redundancy version.  LDPC_EINVAL for n_buf < 1, E < 1, start outside
 * 0 .. n_buf - 1, a null pos.  The entries of buf are judged by ldpc_ratematch_create_on. */
int ldpc_ratematch_circular_positions(int n_buf, const int32_t *buf /* [n_buf] or NULL */, int start, int E, int32_t *pos /* [E] */);
/* The receive side, one kernel, no memset before it and no atomic in it.  d_sym [batch][ceil(E / m)][2] as ldpc_demap_dev_il; d_gain
 * [batch][n_sym] float32 or NULL = no channel state.  The LLR l_t of transmitted bit t is, bit for bit, ldpc_demap_dev_il's (d_gain
 * NULL) or ldpc_demap_dev_il_csi's (inv_s = fl(inv a)) for that bit, for table objects and product objects; pad bits have none.  For
 * position c with the transmitted indices t_1 < t_2 < .. < t_r,
 *   v = fl(fl(fl(l_t1 + l_t2) + l_t3) + ..)  in float32, left to right;  r = 1: v = l_t1.
 * accumulate = 0: element c = the output conversion of ldpc_demap_dev applied to v; 0 where r = 0.  EVERY element of d_llr [batch][N]
 *   is written exactly once, none is read.  With an injective table this is ldpc_demap_dev_il (or _csi), bit for bit.
 * accumulate = 1 (HARQ): d_llr holds the soft buffer of the earlier rounds in the same format, `old`:
 *   LDPC_LLR_F32  fl(old + v);
 *   LDPC_LLR_F16  fl(f32(old) + v), clamped to +-65504 and rounded as the fp16 store of ldpc_demap_dev; a NaN sum stays NaN;
 *   LDPC_LLR_I8   clip(rint(fl(f32(old) + fl(v qscale))), -127, 127); with a NaN v (a NaN sample or gain) the element keeps `old`: an
 *                 erasure, consistent with the quantiser's NaN -> 0.
 *   An element with r > 0 is read once and then written once (int8 with a NaN v: read, not written); an element with r = 0 is neither
 *   read nor written and keeps `old`.  No element is written twice.  The first round of a HARQ process is accumulate = 0, which also
 *   clears the positions it does not send.
 * The kernel is a GATHER, one lane per element of d_llr: the distances of a symbol are computed again by the lane of each of its bits.
 * LDPC_EINVAL as ldpc_demap_dev_il_csi (a null d_gain excepted), for accumulate outside {0, 1}, and for a table on another device than
 * the calling thread's; all but the last before the device is touched.
 * NOT PROVIDED: a kernel that generates and demaps in one (the gather reads samples that several lanes share, so they must be in
 * memory); combining buffers of different formats; a scale on `old`; punctured-position bookkeeping across rounds beyond "keeps old". */
int ldpc_demap_dev_rm(const ldpc_modulation *mod, const ldpc_ratematch *rm, int batch, const float *d_sym /* [batch][ceil(E/m)][2] */,
                      const float *d_gain /* [batch][n_sym] or NULL */, double noise_var, void *d_llr /* [batch][N] */, int llr_fmt,
                      float qscale, int accumulate, void *stream);
/* The table alone, for a caller's own demapper: the same kernel with l_t = d_llr_tx[f][t] (float32, 4-byte aligned, [batch][E]) in
 * place of the demapper's rule; the sum, the formats, accumulate and what is read and written are ldpc_demap_dev_rm's.  ldpc_demap_dev on
 * n_tx = N = E into float32, followed by this call, equals ldpc_demap_dev_rm bit for bit. */
int ldpc_ratematch_llr_dev(const ldpc_ratematch *rm, int batch, const float *d_llr_tx /* [batch][E] */, void *d_llr /* [batch][N] */,
                           int llr_fmt, float qscale, int accumulate, void *stream);
/* The transmit side.  ldpc_ratematch_bits_dev: codewords [batch][N] as LDPC_BITS_BYTES or LDPC_BITS_PACKED -> transmitted bits
 * [batch][E] in either format (rows of ceil(E / 8) bytes, pad bits 0), bit t = codeword bit pos[t]; as ldpc_interleave_bits_dev.
 * ldpc_sim_noise_var_rm: ldpc_sim_noise_var with the rate of THIS transmission, R = k / E.
 * ldpc_sim_transmit_rm: ldpc_sim_transmit_il (fad NULL: AWGN; d_gain is then not written) or ldpc_sim_transmit_il_fading with the
 * labels gathered through pos [E] and sigma from ldpc_sim_noise_var_rm; d_sym [batch][ceil(E / m)][2].  The noise (Philox counters,
 * stream 2, Box-Muller), the gains (stream 3) and the symbol rule are untouched.  The table's N must be the code's N, every pos[t] must
 * be below the source's n_tx (its codewords are cut there) and the table must live on the source's device: LDPC_EINVAL otherwise.
 * A RETRANSMISSION of the same messages with fresh noise and fresh gains: pass the first round's d_msg as d_msg_in (LDPC_BITS_BYTES)
 * and another seed; Chase combining uses the same table, incremental redundancy another window of the buffer. */
int ldpc_ratematch_bits_dev(const ldpc_ratematch *rm, int batch, const void *d_codewords, int cw_fmt, void *d_tx_bits, int tx_fmt, void *stream);
double ldpc_sim_noise_var_rm(const ldpc_sim *sim, const ldpc_modulation *mod, const ldpc_ratematch *rm, double ebn0_db);
int ldpc_sim_transmit_rm(ldpc_sim *sim, const ldpc_modulation *mod, const ldpc_ratematch *rm, const ldpc_fading *fad /* NULL = AWGN */,
                         uint64_t seed, uint64_t first_frame, int batch, double ebn0_db, const void *d_msg_in, int msg_fmt, float *d_sym,
                         float *d_gain /* [batch][n_sym], may be NULL */, uint8_t *d_msg, void *stream);
/* the receive side: message bit i of a frame = decoded bit msg_pos[i] of d_bits [batch][N] bytes (bit 0 of each), written in
 * msg_fmt.  With the systematic form message and parity bits interleave; any source qualifies, LDPC_ENCODER_NONE included. */
int ldpc_sim_extract_messages(const ldpc_sim *sim, int batch, const uint8_t *d_bits, void *d_msg, int msg_fmt, void *stream);
/* d_tally[4] (device, uint64) += {frames, frame errors, message-bit errors, sum of iterations}
 * for the frames of the last ldpc_sim_generate call; d_iters may be NULL. */
int ldpc_sim_tally(ldpc_sim *sim, int batch, const uint8_t *d_bits, const int32_t *d_iters,
                   uint64_t *d_tally, void *stream);
/* host-side encode of one message with the same rule (parity only, p bytes; M bytes for the encoder from H) -- used by tests */
int ldpc_sim_encode_host(const ldpc_sim *sim, const uint8_t *msg, uint8_t *parity);
/* ---- CRC attach and check: what a receiver has in place of the transmitted message.  A message of k bits is L payload bits followed
 * by the w bits of their CRC.  The rule is integer arithmetic, restated in tests/crc_spec.py; the kernels reproduce it exactly.
 * PARAMETERS: width w in 1 .. 32; poly = the generator without its x^w term, odd and below 2^w; init and xorout below 2^w; the payload
 * length L = n_bits >= 1; k = L + w <= 2^24.
 * REGISTER: r = init; for the payload bits b_i, i = 0 .. L - 1, in message order (msg_pos order, the order ldpc_sim_encode_messages takes):
 *   top = (r >> (w - 1)) & 1;  r = (r << 1) & (2^w - 1);  if (top ^ b_i) r ^= poly;
 * crc = r ^ xorout.  No reflection and no notion of a byte.  APPENDED: message bit L + j = (crc >> (w - 1 - j)) & 1, j = 0 .. w - 1, the
 * MSB first.  LDPC_BITS_PACKED is the layout above (bit i in byte i / 8 at bit i % 8), so for whole bytes w = 32, poly 0x04C11DB7,
 * init = xorout = 0xFFFFFFFF over a packed row is zlib's crc32 of those bytes with its 32 bits reversed.
 * LINEAR FORM: crc = C0 ^ XOR over the set payload bits i of T[i], T[i] = the register after the unit vector e_i with init = xorout = 0,
 * C0 = the CRC of L zero bits.
 * The built-in parameter sets are defined by formula, with NO claim that they are any standard's (w, poly, init, xorout):
 *   LDPC_CRC_6 (6, 0x21, 0, 0)  LDPC_CRC_11 (11, 0x621, 0, 0)  LDPC_CRC_16 (16, 0x1021, 0, 0)  LDPC_CRC_24A (24, 0x864CFB, 0, 0)
 *   LDPC_CRC_24B (24, 0x800063, 0, 0)  LDPC_CRC_24C (24, 0xB2B117, 0, 0)  LDPC_CRC_32 (32, 0x04C11DB7, 0xFFFFFFFF, 0xFFFFFFFF). */
enum { LDPC_CRC_6 = 0, LDPC_CRC_11 = 1, LDPC_CRC_16 = 2, LDPC_CRC_24A = 3, LDPC_CRC_24B = 4, LDPC_CRC_24C = 5, LDPC_CRC_32 = 6 };
/* Host only, no device touched.  ldpc_crc_builtin: the parameters of a kind (any pointer may be NULL); LDPC_EINVAL for an unknown kind.
 * ldpc_crc_bits_host: the bit-serial rule over n_bits bytes, bit 0 of each.  ldpc_crc_table: T [n_bits] of the linear form.  Both check
 * their parameters as ldpc_crc_create_on does. */
int ldpc_crc_builtin(int kind, int *width, uint32_t *poly, uint32_t *init, uint32_t *xorout);
int ldpc_crc_bits_host(int width, uint32_t poly, uint32_t init, uint32_t xorout, int n_bits, const uint8_t *bits /* [n_bits] */, uint32_t *crc);
int ldpc_crc_table(int width, uint32_t poly, int n_bits, uint32_t *table /* [n_bits] */);
/* The object holds the table the kernels read (4 k bytes, rounded up to 16) in device memory on `device`.  The arguments are checked
 * before the device is touched: LDPC_EINVAL and NULL for a width outside 1 .. 32, an even poly, poly, init or xorout at or above 2^w,
 * n_bits < 1, n_bits + width > 2^24; only then LDPC_ENODEVICE (device < 0, no such device) or LDPC_EHIP. */
typedef struct ldpc_crc ldpc_crc;
ldpc_crc *ldpc_crc_create_on(int device, int width, uint32_t poly, uint32_t init, uint32_t xorout, int n_bits);
void ldpc_crc_destroy(ldpc_crc *crc);
int ldpc_crc_params(const ldpc_crc *crc, int *width, uint32_t *poly, uint32_t *init, uint32_t *xorout, int *n_bits);   /* any pointer may be NULL */
/* Device pointers, the calling thread's device = the object's, enqueued on `stream`, not synchronised.  batch >= 1 and batch * k <=
 * 2^32 - 256 (LDPC_EINVAL otherwise, and for a null pointer or an unknown format).  One wave per frame; no atomics.
 * ldpc_crc_attach_dev, IN PLACE: reads message bits 0 .. L - 1 and writes bits L .. k - 1.
 *   LDPC_BITS_BYTES   d_msg [batch][k]: only bit 0 of a payload byte is read and no payload byte is written; the CRC bytes are 0 or 1.
 *   LDPC_BITS_PACKED  rows of 4 * ceil(k / 32) bytes, 4-byte aligned: payload bits are kept, bits >= k of the last word are written 0.
 * ldpc_crc_check_dev: d_ok[f] = 1 if the trailing w bits of message f are the CRC of its first L, else 0; every element of d_ok
 * [batch] is written exactly once, the messages are not written. */
int ldpc_crc_attach_dev(const ldpc_crc *crc, int batch, void *d_msg, int msg_fmt, void *stream);
int ldpc_crc_check_dev(const ldpc_crc *crc, int batch, const void *d_msg, int msg_fmt, uint8_t *d_ok /* [batch] */, void *stream);
/* The same check straight on decoded codewords: message bit i = decoded bit msg_pos[i] of d_bits, [batch][N] bytes (LDPC_BITS_BYTES, bit
 * 0 of each) or packed rows of ceil(N / 8) bytes as ldpc_decode_batch_dev_packed writes them (LDPC_BITS_PACKED).  No message buffer is
 * written in between: the flags are those of ldpc_sim_extract_messages followed by ldpc_crc_check_dev, bit for bit.  LDPC_EINVAL also
 * when L + w is not the source's k, or the object lives on another device than the source. */
int ldpc_sim_crc_check(const ldpc_sim *sim, const ldpc_crc *crc, int batch, const void *d_bits, int bits_fmt, uint8_t *d_ok /* [batch] */, void *stream);
/* d_tally[4] (device, uint64) += {frames, CRC passes (d_ok != 0), frames with a message-bit error, frames that pass AND have an error:
 * the undetected errors}.  d_bits [batch][N] bytes; the messages compared against are those ldpc_sim_tally compares against: the ones
 * the source last drew, or the caller's after ldpc_sim_generate_from, ldpc_sim_encode_messages or a transmit with d_msg_in.
 * 1 <= batch <= max_batch. */
int ldpc_sim_tally_crc(ldpc_sim *sim, int batch, const uint8_t *d_bits, const uint8_t *d_ok /* [batch] */, uint64_t *d_tally /* [4] */, void *stream);
/* ---- BCH outer code: a binary, narrow-sense, primitive BCH code that REPAIRS the few bit errors a decode leaves where the CRC above
 * can only detect them.  The rule is integer arithmetic, restated in tests/bch_spec.py; the kernels reproduce it exactly.
 * FIELD: GF(2^m), m = 3 .. 16, from prim_poly (the x^m term included, e.g. 0x1002D), alpha = x, N0 = 2^m - 1; a prim_poly under which x
 * does not have order N0 is refused.  GENERATOR: g = the product of the distinct minimal polynomials of alpha^1 .. alpha^(2t), t = 1 .. 16,
 * 2t < N0; p = deg g <= m t <= 256.  The code is shortened to n bits, p < n <= N0; k = n - p.
 * ROW: bit i, i = 0 .. n - 1, is the coefficient of x^(n - 1 - i): bits 0 .. k - 1 the message, bits k .. n - 1 the remainder of
 * m(x) x^p mod g, MSB first (the CRC's order).  LDPC_BITS_BYTES rows are n bytes; LDPC_BITS_PACKED rows are 4 * ceil(n / 32) bytes, 4-byte
 * aligned, bit i in byte i / 8 at bit i % 8.
 * DECODE: if a codeword lies within Hamming distance e <= t of the row (it is unique) the row becomes it and nerr = e; otherwise the row
 * stays exactly as it was and nerr = -1.
 * The built-in parameter sets are defined by formula, with NO claim that they are any standard's (m, prim_poly, t):
 *   LDPC_BCH_M16_T8 (16, 0x1002D, 8)  LDPC_BCH_M16_T10 (16, 0x1002D, 10)  LDPC_BCH_M16_T12 (16, 0x1002D, 12)  LDPC_BCH_M14_T12 (14, 0x402B, 12). */
enum { LDPC_BCH_M16_T8 = 0, LDPC_BCH_M16_T10 = 1, LDPC_BCH_M16_T12 = 2, LDPC_BCH_M14_T12 = 3 };
/* The object holds the field's tables and g on the host and, for device >= 0, the kernels' tables in device memory: 4 W n bytes of the
 * remainder's linear form (W = ceil(p / 32) rounded up to 1, 2, 4, 6 or 8) and 6 N0 bytes of antilog (doubled) and log.  device = -1
 * makes a host-only object that serves the _host functions alone.  The arguments are checked before the device is touched: LDPC_EINVAL
 * and NULL, the message naming the argument, for m, t or n out of range, a prim_poly that is not primitive, 2t >= N0, n <= p. */
typedef struct ldpc_bch ldpc_bch;
ldpc_bch *ldpc_bch_create_on(int device, int m, uint32_t prim_poly, int t, int n);
void ldpc_bch_destroy(ldpc_bch *bch);
int ldpc_bch_builtin(int kind, int *m, uint32_t *prim_poly, int *t);                                  /* any pointer may be NULL */
int ldpc_bch_params(const ldpc_bch *bch, int *m, uint32_t *prim_poly, int *t, int *n, int *k);   /* any pointer may be NULL */
int ldpc_bch_generator(const ldpc_bch *bch, uint8_t *g /* [p + 1], g[j] = coeff of x^j; may be NULL */);   /* returns p */
/* The serial rule on one row of n bytes, in place, no device touched: bit 0 of a byte is read, encode writes the p parity bytes as 0 / 1,
 * decode flips bit 0 of the bytes it corrects (*nerr as above). */
int ldpc_bch_encode_host(const ldpc_bch *bch, uint8_t *row /* [n] bytes, in place */);
int ldpc_bch_decode_host(const ldpc_bch *bch, uint8_t *row /* [n] bytes, in place */, int *nerr);
/* Device pointers, the calling thread's device = the object's, enqueued on `stream`, not synchronised.  batch >= 1 and batch * n <=
 * 2^32 - 256 (LDPC_EINVAL otherwise, and for a null pointer, an unknown format or a host-only object).  One wave per frame; no atomics.
 * ldpc_bch_encode_dev, IN PLACE: reads bits 0 .. k - 1 and writes bits k .. n - 1.
 *   LDPC_BITS_BYTES   only bit 0 of a message byte is read and no message byte is written; the parity bytes are 0 or 1.
 *   LDPC_BITS_PACKED  message bits are kept, bits >= n of the last word are written 0.
 * ldpc_bch_decode_dev, IN PLACE: d_nerr[f] is written exactly once; a corrected bit is row[i] ^= 1 (bytes: bits 1 .. 7 survive) or that
 * one bit of a packed row; a row with d_nerr[f] <= 0 is not written. */
int ldpc_bch_encode_dev(const ldpc_bch *bch, int batch, void *d_rows, int fmt, void *stream);
int ldpc_bch_decode_dev(const ldpc_bch *bch, int batch, void *d_rows, int fmt, int32_t *d_nerr /* [batch] */, void *stream);
/* The same decode straight on decoded codewords, to the BCH decoder what ldpc_sim_crc_check is to the CRC: BCH row bit i = decoded bit
 * msg_pos[i] of d_bits, [batch][N] bytes (LDPC_BITS_BYTES) or packed rows of ceil(N / 8) bytes (LDPC_BITS_PACKED), corrected where they
 * lie; no other bit is written.  LDPC_EINVAL also when n is not the source's message length, or the object lives on another device
 * than the source.  ldpc_sim_tally, ldpc_sim_extract_messages and ldpc_sim_tally_crc (with ok = nerr >= 0) then work as they are. */
int ldpc_sim_bch_decode(const ldpc_sim *sim, const ldpc_bch *bch, int batch, void *d_bits /* decoded codewords [batch][N] */, int bits_fmt, int32_t *d_nerr /* [batch] */,
                        void *stream);

/* ---- matrix ingest --------------------------------------------------------------------------------
 * replaces loadMatrix (src/Data/BitMatrix/Loader.hs:58-81): `name` is "<matrix>/H" or "<matrix>/G";
 * for each loader in the reference's order (.q, .alist, .m; Loader.hs:53-57) the first existing
 * file <codes_dir>/<name>.<suffix> is parsed: .q = QuasiCyclic.hs:52-56 (integers of any size),
 * .alist = the reference's reader, Alist.hs:30-46 (zeros dropped, ROWS first, row lists only),
 * .m = Data/BitMatrix/Matlab.hs:20-26. */
typedef struct ldpc_matrix ldpc_matrix;
ldpc_matrix *ldpc_matrix_load(const char *codes_dir, const char *name);
/* one file in MacKay's published alist order (N M first, zero-padded lists), e.g.
 * codes/1920.1280.3.303, which the reference's reader cannot load. */
ldpc_matrix *ldpc_matrix_load_mackay(const char *path);
void ldpc_matrix_destroy(ldpc_matrix *m);
/* rows/cols of the EXPANDED matrix (getNRows/getNCols, Loader.hs:31-46); qc_sz = 0 if not .q */
int ldpc_matrix_info(const ldpc_matrix *m, int *rows, int *cols, int *qc_sz, int *block_rows, int *block_cols);
int ldpc_matrix_dense(const ldpc_matrix *m, uint8_t *out /* rows*cols bytes 0/1 */);  /* QuasiCyclic.hs:19-25 */
/* rank over GF(2) of the expanded matrix (a stand-alone parity-check matrix defines cols - rank message bits:
 * codes/1920.1280.A holds 5760 checks of rank 1280); negative = LDPC_E* */
int ldpc_matrix_rank(const ldpc_matrix *m);
/* a QC source's first-row patterns as little-endian 32-bit words: out [block_rows][block_cols][ceil(sz/32)]
 * (what Fast/Encoder.hs:38-39 converts the Integers of G.q to) */
int ldpc_matrix_qc_words(const ldpc_matrix *m, uint32_t *out);
/* rotation table of a .q matrix, -1 = empty block (Fast/Arraylet.hs:68-79); LDPC_EUNSUPPORTED for
 * a block holding more than one circulant (the reference errors there too). */
int ldpc_matrix_qc_offsets(const ldpc_matrix *m, int32_t *offsets /* block_rows*block_cols */);
/* QC graph when every block is a single circulant, generic CSR otherwise */
ldpc_code *ldpc_code_from_matrix(const ldpc_matrix *m);

/* ---- the plug-in record ----------------------------------------------------------------------------
 * C mirror of what mkLDPC returns (src/ECC/Code/LDPC/Utils.hs:35-75): ECC{name, encode, decode,
 * message_length, codeword_length}, selected by the reference's code-name grammar
 *   ldpc/<decoder>/<matrix-name>/<max-rounds>[/<x>/<y>]        (Utils.hs:82-88,100-108; rate x%y)
 * with <decoder> in {hip-tanh, hip-minsum}[-layered][-bool][-f32|-f64|-f16|-i8] (-i8: hip-minsum-layered only) or hip-tanh-cm-f64 (-bool: H taken as a plain
 * Boolean matrix, the `Matrix Bool` decoders' input).  hip-minsum-layered takes the check-node rule after the dtype suffix:
 * [-s<decimal>][-o<decimal>] = cn_scale, cn_offset of ldpc_ctx_config, e.g. ldpc/hip-minsum-layered-i8-s1-o0.5/<matrix>/<rounds>
 * (<decimal>: digits with at most one point; on any other decoder name the suffix makes the name unknown: LDPC_ENOTFOUND), or, in the same
 * place and instead of them, -amin = cn_rule LDPC_CN_AMINSTAR, e.g. ldpc/hip-minsum-layered-f16-amin/<matrix>/<rounds> (-amin together
 * with -s / -o, or on another decoder name: LDPC_ENOTFOUND; with -i8: the context's LDPC_EUNSUPPORTED).  The reference's own decoder names are accepted as aliases, so a
 * command line written for it runs unchanged: reference, sparse -> hip-tanh-bool; min, sparsemin -> hip-minsum-bool;
 * arraylet, cuda-arraylet1, cuda-arraylet2, two-arrays, cuda-arraylet-cm -> hip-tanh; arraylet-min -> hip-minsum;
 * arraylet-cm -> hip-tanh-cm-f64 (a dtype suffix may follow: ldpc/reference-f64/...).  The ECC keeps the name it was
 * asked for.  NULL + LDPC_ENOTFOUND for any other name (the factory's `_ -> return []`). One decoder replica is created (maxThreadCount = 1, like
 * the CUDA plug-ins, GPU/CUDA/Arraylet2.hs:61). */
typedef struct ldpc_ecc ldpc_ecc;
ldpc_ecc *ldpc_ecc_create(const char *codes_dir, const char *code_name, int max_batch);
/* the reference's maxThreadCount (Utils.hs:53 replicateM maxThreadCount $ decoder0 h): n_replicas decoder replicas in
 * ONE process, replica i on HIP device devices[i] (devices = NULL: all on the calling thread's device) -- one host
 * process can drive every GPU of a node.  ldpc_ecc_decode picks the replica by calling thread, as Utils.hs:63-69
 * does (thread ordinal mod n_replicas); ldpc_ecc_decode_on names it. */
ldpc_ecc *ldpc_ecc_create_replicas(const char *codes_dir, const char *code_name, int max_batch, int n_replicas, const int *devices);
int ldpc_ecc_replicas(const ldpc_ecc *ecc);
ldpc_ctx *ldpc_ecc_ctx_at(ldpc_ecc *ecc, int replica);
ldpc_sim *ldpc_ecc_sim_at(ldpc_ecc *ecc, int replica);
int ldpc_ecc_decode_on(ldpc_ecc *ecc, int replica, const double *llr, uint8_t *msg_bits, int *ok);
/* route ldpc_ecc_decode through a batcher per replica (see above): max_frames = 0 switches it off again */
int ldpc_ecc_set_coalescing(ldpc_ecc *ecc, int max_frames, int max_wait_us);
int ldpc_ecc_coalescing_stats(ldpc_ecc *ecc, long *calls, long *launches);   /* summed over the replicas */
void ldpc_ecc_destroy(ldpc_ecc *ecc);
const char *ldpc_ecc_name(const ldpc_ecc *ecc);            /* Utils.hs:60 */
int ldpc_ecc_message_length(const ldpc_ecc *ecc);          /* Utils.hs:73 */
int ldpc_ecc_codeword_length(const ldpc_ecc *ecc);         /* Utils.hs:74 (after puncturing) */
int ldpc_ecc_unpunctured_length(const ldpc_ecc *ecc);      /* cols H */
int ldpc_ecc_max_iters(const ldpc_ecc *ecc);
/* encode: msg [message_length] bytes -> codeword [codeword_length] bytes (Utils.hs:61) */
int ldpc_ecc_encode(const ldpc_ecc *ecc, const uint8_t *msg, uint8_t *codeword);
/* decode: llr [codeword_length] doubles -> msg_bits [message_length]; *ok = the record's Bool
 * (Utils.hs:62-72: un-puncture with zeros, decode, take message_length) */
int ldpc_ecc_decode(ldpc_ecc *ecc, const double *llr, uint8_t *msg_bits, int *ok);
/* the pieces, for batched use (owned by the record) */
ldpc_ctx *ldpc_ecc_ctx(ldpc_ecc *ecc);
ldpc_sim *ldpc_ecc_sim(ldpc_ecc *ecc);
const ldpc_code *ldpc_ecc_code(const ldpc_ecc *ecc);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_HIP_H */
