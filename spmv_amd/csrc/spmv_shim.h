/*
 * spmv_shim.h -- the ONE place host C meets HIP ("thin shim = the only place
 * host C meets HIP").  spmv_api.c / spmv_plan.c (plain C11, gcc) sit above this interface and
 * hold the reference-shaped logic (handle life-cycle, method -> schedule policy, argument
 * rules); spmv_shim.hip (hipcc, gfx950) sits below it and holds device memory, inspectors and
 * kernels.  Plain pointers and sizes only.
 */
#ifndef SPMV_SHIM_H
#define SPMV_SHIM_H
#include <stddef.h>
#include "spmv_hip.h"

#if defined(__cplusplus)
extern "C" {
#endif

typedef struct spmv_dev spmv_dev; /* opaque: device-resident matrix + inspector products */

enum spmv_sched {
    SPMV_SCHED_CSR_SCALAR = 0,
    SPMV_SCHED_CSR_VECTOR = 1,
    SPMV_SCHED_ROWBLOCK = 2,
    SPMV_SCHED_NNZ_SPLIT = 3,
    SPMV_SCHED_SELL = 4,
    SPMV_SCHED_CSR5 = 5,
    SPMV_SCHED_COUNT,
    SPMV_SCHED_HOST_ROWS = 100 /* no device schedule: the plain-C row loop (host_rows.c), reported by spmv_hip_get_info */
};

#define SPMV_LEN_BUCKETS 11 /* <=4, 8, 16, ..., 2048, longer */

typedef struct spmv_stats {
    int m, n;
    long long nnz;
    int max_row_len, min_row_len, empty_rows;
    double mean_row_len;
    /* row-length histogram: bucket b counts the rows with 4*2^(b-1) < len <= 4*2^b (b = 0: len <= 4;
     * the last bucket: everything longer), and the non-zeros those rows hold */
    long long hist_rows[SPMV_LEN_BUCKETS], hist_nnz[SPMV_LEN_BUCKETS];
} spmv_stats;

typedef struct spmv_plan {
    int sched;          /* enum spmv_sched */
    int lanes_per_row;  /* csr-vector */
    int long_thr;       /* csr-vector: rows longer than this go to the long-row (CSR5 sub-matrix) path; 0 = max(64 L, 256) */
    int sell_c, sell_sigma, sell_lds_x, sell_long_thr;
    int csr5_sigma;
    int slab_kib, block_rows; /* row-block x column-slab executor shape (0 = defaults) */
    int blk_waves, blk_groups, blk_subsort; /* ... waves sharing a block's accumulators (0 auto / 1 / 4 / 8), groups per step (0 = timed), sparse cells sorted by column */
    int deterministic;  /* 1: bit-reproducible results required (default) */
    int cache_block;    /* nnz-split family: 0 never, 1 automatic, 2 always use the row-block x column-slab executor */
    int rowblock_nnz;
    int vector_form, x_windows, xcd_order, csr5_two_deep, run_tiles, row_forward; /* executor-form selectors (spmv_plan.c option table) */
    int pack_values;    /* csr-vector, fp64: 7-byte packed value planes for the tiles that qualify: 0 never, 1 always (no timing), 2 timed and guarded (default) */
    int forced;         /* any of the selectors differs from its default: create() does not time alternatives */
    int autotune;       /* csr-vector: time the applicable kernel forms at create and keep the fastest */
} spmv_plan;

/* All functions return SPMV_HIP_OK or an SPMV_HIP_E_* code and record a message retrievable
 * with spmv_shim_error_text() (thread-local). */
int spmv_shim_device_count(void);
const char *spmv_shim_error_text(void);

/* Classify + copy the CSR arrays into HBM (host or device sources), compute row statistics. */
int spmv_shim_matrix_create(spmv_dev **out, int m, int n, const int *rowptr, const int *colidx,
                            const void *val, size_t value_size);
int spmv_shim_matrix_stats(const spmv_dev *d, spmv_stats *out);
/* Run the inspector of plan->sched (device side); may be called again with another plan. */
int spmv_shim_build(spmv_dev *d, const spmv_plan *plan);
/* y = A x.  x, y: host or device pointers. */
int spmv_shim_run(spmv_dev *d, const void *x, void *y);
int spmv_shim_set_stream(spmv_dev *d, void *stream);
int spmv_shim_set_async(spmv_dev *d, int async);
int spmv_shim_sync(spmv_dev *d);
int spmv_shim_info(const spmv_dev *d, spmv_hip_info *out);
double spmv_shim_time(spmv_dev *d, const void *x, void *y, int warmup, int iters, float *ms_out);
/* min over `iters` (<= 64) launches on scratch vectors, in ms; < 0 on failure */
double spmv_shim_time_self(spmv_dev *d, int iters);
void spmv_shim_matrix_destroy(spmv_dev *d);
/* memcpy that accepts a host or a device source (the reordering inspector works on host copies) */
int spmv_shim_copy_to_host(void *dst, const void *src, size_t bytes);
/* release the device blocks the library keeps for re-use between handles (shim/state.hpp "device-memory pool") */
void spmv_shim_trim_pool(void);
/* 1 if a kernel can use the pointer as is (device or managed memory), else 0 (also without any device) */
int spmv_shim_is_device_ptr(const void *p);
/* After the last spmv_shim_build of a create: give the resident ColIdx copy back when the built schedule's multiply never reads it */
int spmv_shim_release_columns(spmv_dev *d);
/* New values (host or device, nnz entries in CSR order) behind the same pattern: copied to HBM and
 * re-permuted into the schedule's private value layouts; nothing else is rebuilt. */
int spmv_shim_update_values(spmv_dev *d, const void *val);
/* Order-independent 64-bit checksum (sum of the 32-bit words) of nnz values at `val` (host or device). */
int spmv_shim_checksum(spmv_dev *d, const void *val, unsigned long long *out);
/* the same sum over `words` 32-bit words at `val` (host or device) without a matrix: multi-GPU handles */
int spmv_shim_checksum_words(const void *val, long long words, unsigned long long *out);

/* Reverse Cuthill-McKee of the resident (square) matrix on the device; P A P^T replaces it, perm (m ints, host) receives the permutation
 * (row i of the new matrix = row perm[i] of the old).  Before spmv_shim_build. */
int spmv_shim_reorder_rcm(spmv_dev *d, int *perm_host);

/* Y = A X for k right-hand sides over the resident CSR (shim/spmm.hpp): X n x k, Y m x k, row-major, leading dimensions ldx, ldy >= k;
 * host or device pointers.  Needs the resident ColIdx (spmv_shim_restore_columns after spmv_shim_release_columns). */
int spmv_shim_spmm(spmv_dev *d, int k, const void *x, long long ldx, void *y, long long ldy);
/* the same, `iters` launches timed with events on the handle's stream (device X / Y); mean ms, < 0 on failure */
double spmv_shim_time_spmm(spmv_dev *d, int k, const void *x, long long ldx, void *y, long long ldy, int warmup, int iters, float *ms_out);
/* Give a matrix whose ColIdx copy was released its resident copy back, from the create-time arrays (host or device): as is, or permuted
 * with perm_host (m ints, the create-time reordering: row i of the resident matrix = row perm_host[i] of the caller's).  No-op when resident. */
int spmv_shim_restore_columns(spmv_dev *d, const int *rowptr, const int *colidx, const int *perm_host);

/* ---- A^T as a matrix of its own (shim/transpose.hpp; spmv_hip_spmv_transpose) ----
 * spmv_shim_transpose: A^T (n x m, rows listing their entries in ascending row of A) built on the device from the resident CSR -- unplanned,
 * owning its arrays -- and perm (device, nnz ints: perm[p] = the CSR index in A of A^T's entry p).  Needs the resident ColIdx.  The caller
 * plans + builds the child and attaches it (NULLs: detach + destroy); the parent owns both from then on, counts them in its info's
 * device_bytes and frees them at destroy.  spmv_shim_transpose_refresh gathers A's values again after spmv_shim_update_values. */
int spmv_shim_transpose(spmv_dev *d, spmv_dev **out, int **perm_out);
int spmv_shim_attach_transpose(spmv_dev *d, spmv_dev *child, int *perm);
spmv_dev *spmv_shim_transpose_of(const spmv_dev *d); /* NULL until attached */
int spmv_shim_transpose_refresh(spmv_dev *d);
int spmv_shim_transpose_map(spmv_dev *d, int *rowptr_t, int *perm); /* copies to host; either may be NULL */
/* The attached transpose's own column indices again in HBM after its spmv_shim_release_columns gave them back (spmv_shim_spmm on the child
 * gathers through them): colidx_T[p] = row of A of entry perm[p], rebuilt on the device from the parent's RowPtr and perm.  No-op when resident. */
int spmv_shim_transpose_restore_columns(spmv_dev *d);

/* ---- Out[p] = sum_c U[row(p), c] V[col(p), c] over the resident pattern (shim/sddmm.hpp; spmv_hip_sddmm) ----
 * U m x k, V n x k, row-major with leading dimensions ldu, ldv >= k; Out nnz elements in CSR order; host or device pointers each.  Needs the
 * resident ColIdx (spmv_shim_restore_columns after spmv_shim_release_columns). */
int spmv_shim_sddmm(spmv_dev *d, int k, const void *u, long long ldu, const void *v, long long ldv, void *out);
/* `iters` launches timed with events on the handle's stream (device U / V / Out); mean ms, < 0 on failure */
double spmv_shim_time_sddmm(spmv_dev *d, int k, const void *u, long long ldu, const void *v, long long ldv, void *out, int warmup, int iters, float *ms_out);

/* ---- the row softmax over the resident ROW STRUCTURE and its backward (shim/row_softmax.hpp; spmv_hip_row_softmax, _backward) ----
 * S, P, G, Out: nnz elements in CSR order, host or device pointers each; Out may be S (forward) or G (backward).  Reads RowPtr alone: the
 * resident ColIdx is not needed.  Builds spmm's batch table and long-row list at the first call. */
int spmv_shim_row_softmax(spmv_dev *d, const void *s, void *out);
int spmv_shim_row_softmax_backward(spmv_dev *d, const void *p, const void *g, void *out);
/* `iters` forward launches timed with events on the handle's stream (device S / Out); mean ms, < 0 on failure */
double spmv_shim_time_row_softmax(spmv_dev *d, const void *s, void *out, int warmup, int iters, float *ms_out);

/* ---- the fused attention over the resident pattern and its backward: one argument struct each (shim/attention.hpp, shim/attention_backward.hpp) ----
 * What every spmv_hip_attention* entry point passes down; an entry point without a feature fills it as heads = kv_heads = 1, bias = NULL,
 * lse = NULL, the types SPMV_HIP_T_HANDLE.  The operand conventions, once:
 *   - k and dv are ONE head's widths.  Q, G, O, dQ are `heads` blocks wide (heads * k, heads * dv columns), K, V, dK, dV `kv_heads` blocks
 *     (kv_heads * k, kv_heads * dv); heads is a multiple of kv_heads and query head h reads block h / (heads / kv_heads).  Row-major, every
 *     leading dimension at least the operand's width and counted in elements of the operand's own type; host or device pointers each.
 *   - bias: NULL (ldb ignored) or planes of nnz elements in CSR order, QUERY head h's at bias + h * ldb; ldb = 0: one plane for all heads, else
 *     ldb >= nnz.  lse: `heads` planes ldl >= m apart, head h's row i at lse + h * ldl + i.  db: `heads` planes lddb >= nnz apart.  bias, db, lse
 *     and the backward's o are in the handle's precision whatever the types say.
 *   - io_type SPMV_HIP_T_HANDLE: every operand in the handle's precision, and the output types are SPMV_HIP_T_HANDLE too.  io_type SPMV_HIP_T_F16 or
 *     _BF16 (a float handle): the element type of Q, K, V and G; an output type (o_type of O, dq_type of dQ, dkv_type of dK and dV) is
 *     SPMV_HIP_T_HANDLE (float) or io_type.  Anything else, or a double handle with a 16-bit io_type: SPMV_HIP_E_ARG.
 *   - An output pointer that is NULL is not wanted and its leading dimension is not looked at (the forward's O is always wanted).
 *   - A refusal (SPMV_HIP_E_ARG: a bad size, stride or type, a NULL operand while m > 0) writes nothing.
 * The resident values are neither read nor written; the resident ColIdx is needed (spmv_shim_restore_columns). */
typedef struct spmv_attention_call {
    int heads, kv_heads, k, dv;
    double scale;
    int io_type, o_type;
    const void *q;    long long ldq;  /* m x heads * k */
    const void *kk;   long long ldk;  /* n x kv_heads * k */
    const void *v;    long long ldv;  /* n x kv_heads * dv */
    const void *bias; long long ldb;
    void *o;          long long ldo;  /* m x heads * dv */
    void *lse;        long long ldl;  /* NULL: the rows' log-sum-exps are not wanted */
} spmv_attention_call;

typedef struct spmv_attention_backward_call {
    int heads, kv_heads, k, dv;
    int max_heads; /* heads per round of the two passes: option "attention_backward_heads"; 0: what fits an eighth of the device's memory */
    double scale;
    int io_type, dq_type, dkv_type;
    const void *q;    long long ldq;
    const void *kk;   long long ldk;
    const void *v;    long long ldv;
    const void *bias; long long ldb;
    const void *g;    long long ldg;  /* dL/dO, m x heads * dv */
    /* stats != 0: the row pass is driven by o and lse, the FINAL output and log-sum-exp of the attention this handle's entries are a part of
     * (P = exp(t - L), D = <G row, O row>).  stats == 0: it normalises by itself and o and lse are not read -- but with a 16-bit io_type one of
     * the two alone while m > 0 is SPMV_HIP_E_ARG (spmv_hip_attention_gqa_backward_16: both or neither, stats = both) */
    int stats;
    const void *o;    long long ldo;
    const void *lse;  long long ldl;
    void *dq;         long long lddq;
    void *dk;         long long lddk; /* dk or dvo wanted: the attached transpose with its column indices resident is needed (its values are not read) */
    void *dvo;        long long lddv;
    void *db;         long long lddb; /* written by the row pass alone: with only db (or dq) wanted the transpose is not looked at */
} spmv_attention_backward_call;

/* O = softmax_rows(scale * Q K^T + bias on the resident pattern) V in one pass, and the log-sum-exps.  Builds spmm's tables and the long rows'
 * parking space at the first call. */
int spmv_shim_attention(spmv_dev *d, const spmv_attention_call *c);
/* `iters` calls timed with events on the handle's stream; mean ms, < 0 on failure.  Every operand that is given must be a device pointer, and
 * Q, K, V and O must be given. */
double spmv_shim_time_attention(spmv_dev *d, const spmv_attention_call *c, int warmup, int iters, float *ms_out);
/* two partial results merged by their log-sum-exps (spmv_hip_attention_merge): the O operands m x heads*dv, the L operands `heads` planes of m; o may
 * be o1 and l may be l1; l NULL: not wanted.  The matrix is not read.  A plane stride below m: SPMV_HIP_E_ARG, nothing written */
int spmv_shim_attention_merge(spmv_dev *d, int heads, int dv, const void *o1, long long ldo1, const void *l1, long long ldl1, const void *o2, long long ldo2, const void *l2,
                              long long ldl2, void *o, long long ldo, void *l, long long ldl);
double spmv_shim_time_attention_merge(spmv_dev *d, int heads, int dv, const void *o1, long long ldo1, const void *l1, long long ldl1, const void *o2, long long ldo2,
                                      const void *l2, long long ldl2, void *o, long long ldo, void *l, long long ldl, int warmup, int iters, float *ms_out);

/* dQ, dK, dV and dB of spmv_shim_attention in two passes per round of up to hg heads (hg = min(heads, max_heads) when max_heads > 0, else by the
 * memory rule); dK / dV of a K / V block are the sums of its query heads' terms in ascending head.  Builds spmm's tables (the transpose's too)
 * and the two arrays of hg planes of nnz elements at the first call, grown when a call needs more. */
int spmv_shim_attention_backward(spmv_dev *d, const spmv_attention_backward_call *c);
/* `iters` calls timed with events on the handle's stream; mean ms, < 0 on failure.  Every operand that is given must be a device pointer, and
 * Q, K, V, G and, with stats, O and L must be given. */
double spmv_shim_time_attention_backward(spmv_dev *d, const spmv_attention_backward_call *c, int warmup, int iters, float *ms_out);

/* ---- the solves on the resident matrix that stay on the device (shim/solve.hpp): six solvers, one call struct, one loop, one timer ----
 * spmv_hip_cg, spmv_hip_bicgstab (the matrix need not be symmetric), spmv_hip_cg_columns (k right-hand sides in one pass over A per iteration),
 * spmv_hip_gmres (restarted GMRES(restart)), spmv_hip_cg_mixed (fp32 iterations, fp64 solution and true residual) and spmv_hip_lsqr (least
 * squares for any m x n matrix).  What every entry point passes down; one that lacks a field fills it as k = ldb = ldx = 1, restart = 0,
 * low = NULL, update_drop = 0, update_every = 0, updates = NULL, ls_tol = damp = 0, ar = anorm = NULL:
 *   - b, x: m x k elements of the handle's value type, row-major, leading dimensions ldb, ldx >= k; opt.Dinv: ONE vector of m elements (floats
 *     for spmv_hip_cg_mixed, whose handle is fp64); host or device pointers each.  1 <= k <= SPMV_HIP_CG_COLUMNS_MAX for spmv_hip_cg_columns,
 *     which multiplies with spmv_shim_spmm's executor and needs the resident ColIdx (spmv_shim_restore_columns); k = 1 for the others, whose
 *     multiply is the built schedule's own launch.
 *   - restart: 1 <= restart <= SPMV_HIP_GMRES_RESTART_MAX for spmv_hip_gmres.
 *   - low: spmv_hip_cg_mixed's fp32 handle, only multiplied with; the handle of the call is the fp64 one and owns the workspace.  The pair has
 *     the same m = n and nnz, device and stream: SPMV_HIP_E_ARG otherwise.
 *   - spmv_hip_lsqr: the matrix need not be square; b has m elements and x n; its second multiply is the ATTACHED TRANSPOSE's own launch
 *     (spmv_shim_attach_transpose, the values refreshed: spmv_shim_transpose_refresh), SPMV_HIP_E_NOSTATE without one.  ls_tol and damp are
 *     its options, ar and anorm (NULL: not wanted) receive its two further results; opt.Dinv must be NULL.
 *   - res: k entries; opt.history: (max_iterations + 1) * k doubles; updates: spmv_hip_cg_mixed's committed updates.
 * Each solver builds a workspace of its own on the handle at its first call; spmv_hip_cg_columns' is allocated anew when a later call has more
 * columns, spmv_hip_gmres's (restart + 3 vectors) when one has a larger restart.  SPMV_HIP_OK whenever the solve ran (res->status says how it
 * ended); synchronous */
enum { SPMV_SHIM_SOLVE_CG, SPMV_SHIM_SOLVE_BICGSTAB, SPMV_SHIM_SOLVE_CG_COLUMNS, SPMV_SHIM_SOLVE_GMRES, SPMV_SHIM_SOLVE_CG_MIXED, SPMV_SHIM_SOLVE_LSQR,
       SPMV_SHIM_SOLVE_COUNT };
typedef struct spmv_solve_call {
    int solver;      /* SPMV_SHIM_SOLVE_* */
    spmv_dev *low;
    int k, restart;
    const void *b;   long long ldb;
    void *x;         long long ldx;
    spmv_hip_cg_options opt; /* rtol, atol, max_iterations, check_every, use_x0, Dinv, history */
    double update_drop;      /* spmv_hip_cg_mixed: 0 = SPMV_HIP_CG_MIXED_UPDATE_DROP */
    int update_every;
    spmv_hip_cg_result *res;
    int *updates;            /* NULL: not wanted */
    double ls_tol, damp;     /* spmv_hip_lsqr */
    double *ar, *anorm;      /* spmv_hip_lsqr's results; NULL: not wanted */
} spmv_solve_call;
int spmv_shim_solve(spmv_dev *d, const spmv_solve_call *c);
/* `iters` runs of opt.max_iterations iterations each, the stop tests off, timed with events on the handle's stream (device B / X / Dinv); mean ms per
 * run, < 0 on failure.  spmv_hip_gmres: the iterations include the cycle ends and restarts that fall among them; spmv_hip_cg_mixed: an update behind
 * every update_every-th iteration (none at 0).  res, updates, ar and anorm are not looked at */
double spmv_shim_time_solve(spmv_dev *d, const spmv_solve_call *c, int warmup, int iters, float *ms_out);
/* out[i] = the fp64 square root of in[i] as spmv_hip_gmres's kernels take it: n doubles each, device pointers; synchronous */
int spmv_shim_gmres_sqrt(const double *in, double *out, long long n);

/* the resident CSR arrays (device pointers; ColIdx may be NULL after spmv_shim_release_columns) */
void spmv_shim_matrix_arrays(const spmv_dev *d, const int **rowptr, const int **colidx, const void **val);

/* ---- A = A_near + A_far (shim/split.hpp): a matrix with locality in part of its entries ---- */
int spmv_shim_split_candidate(spmv_dev *d);                                   /* 1: worth building and timing */
int spmv_shim_split(spmv_dev *d, spmv_dev **near_out, spmv_dev **far_out);    /* the two halves, unplanned; far multiplies accumulating */
int spmv_shim_attach_split(spmv_dev *d, spmv_dev *near_dev, spmv_dev *far_dev, int release_parent_schedule); /* NULLs: detach + destroy */
void spmv_shim_note_split_ms(spmv_dev *d, double as_built_ms, double split_ms);

/* ---- row blocks over several GPUs of this process (shim/multi.hpp; option "gpus") ---- */
typedef struct spmv_multi spmv_multi;
/* Split the matrix into min(gpus, visible devices) equal-nnz row blocks, one shard (spmv_dev) per device, each with its
 * x buffer, y block and stream; xchg: 0 allgather, 2 broadcast.  The caller then plans + builds every shard. */
int spmv_shim_multi_create(spmv_multi **out, int gpus, int xchg, int m, int n, const int *rowptr, const int *colidx,
                           const void *val, size_t value_size);
/* ... or from G row blocks handed over separately: rows[g] rows, LOCAL 0-based RowPtr, GLOBAL columns (numa.c:277-304) */
int spmv_shim_multi_create_blocks(spmv_multi **out, int G, int xchg, const int *rows, int n, const int *const *rowptr, const int *const *colidx,
                                  const void *const *val, size_t value_size);
int spmv_shim_multi_count(const spmv_multi *mt);
int spmv_shim_multi_rows(const spmv_multi *mt);
/* the boundary rows' sub-matrix of shard g ("range" exchange with overlap), or NULL: planned and built like a shard */
spmv_dev *spmv_shim_multi_boundary(spmv_multi *mt, int g);
int spmv_shim_multi_uses_rccl(const spmv_multi *mt);
long long spmv_shim_multi_nnz(const spmv_multi *mt);
spmv_dev *spmv_shim_multi_shard(spmv_multi *mt, int g);
/* y = A x with full-length host or device vectors: upload / exchange / multiply / collect */
int spmv_shim_multi_run(spmv_multi *mt, const void *x, void *y);
/* distributed vectors: shard g's slice of x (inside its full-length copy) and its block of y, on device *device */
int spmv_shim_multi_slices(spmv_multi *mt, int g, void **x_slice, long long *x_first, long long *x_count, void **y_block,
                           long long *y_first, long long *y_count, int *device);
/* exchange the x slices between the devices and multiply; y stays in the shards' blocks */
int spmv_shim_multi_step(spmv_multi *mt);
/* the same, enqueued only (ordered behind the work already submitted to each device's default stream); _sync waits */
int spmv_shim_multi_step_async(spmv_multi *mt);
int spmv_shim_multi_sync(spmv_multi *mt);
int spmv_shim_multi_update_values(spmv_multi *mt, const void *val);
void spmv_shim_multi_destroy(spmv_multi *mt);

#if defined(__cplusplus)
}
#endif
#endif
