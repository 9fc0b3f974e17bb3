/*
 * spmv_hip_tools.h -- measurement entry points used by bench.py, tests/ and tools/ only.  NOT part of the drop-in surface (spmv.h) and not
 * part of the extension API an application needs (spmv_hip.h): a program that multiplies never includes this header.  The reference times
 * its multiplies from the outside, with gettimeofday around 100 calls (test_spmv.c:103-127); on a GPU the launch stream has to be
 * bracketed by events, which only the library can place between its own launches.
 */
#include "spmv_Defines.h"
#if defined(__cplusplus)
extern "C" {
#endif
#ifndef SPMV_HIP_TOOLS_H
#define SPMV_HIP_TOOLS_H

/* `warmup` untimed + `iters` timed spmv() launches back to back on the handle's stream, each
 * timed launch bracketed by hipEvents recorded on that stream; ms_out[i] (may be NULL) receives
 * launch i's duration.  x and y must be DEVICE pointers.  Returns the mean in ms, < 0 on error. */
double spmv_hip_time_launches(spmv_Handle_t handle, const void *x, void *y,
                              int warmup, int iters, float *ms_out);

/* The same for spmv_hip_spmm: `warmup` untimed + `iters` timed launches of Y = A X (k columns, leading dimensions ldx / ldy) on the
 * handle's stream, each bracketed by hipEvents; X and Y must be DEVICE pointers.  Returns the mean in ms, < 0 on error. */
double spmv_hip_time_spmm_launches(spmv_Handle_t handle, int k, const void *X, long long ldx, void *Y, long long ldy,
                                   int warmup, int iters, float *ms_out);

/* The same for spmv_hip_spmv_transpose (y = A^T x; x: m entries, y: n entries, DEVICE pointers); builds the transpose first if needed. */
double spmv_hip_time_transpose_launches(spmv_Handle_t handle, const void *x, void *y, int warmup, int iters, float *ms_out);
/* The same for spmv_hip_spmm_transpose (Y = A^T X; X: m x k, Y: n x k, DEVICE pointers); builds the transpose and restores its column
 * indices first if needed. */
double spmv_hip_time_spmm_transpose_launches(spmv_Handle_t handle, int k, const void *X, long long ldx, void *Y, long long ldy,
                                             int warmup, int iters, float *ms_out);
/* The same for spmv_hip_sddmm (U: m x k, V: n x k, Out: nnz elements; DEVICE pointers). */
double spmv_hip_time_sddmm_launches(spmv_Handle_t handle, int k, const void *U, long long ldu, const void *V, long long ldv, void *Out,
                                    int warmup, int iters, float *ms_out);
/* The same for spmv_hip_row_softmax (S and Out: nnz elements, DEVICE pointers; Out may be S). */
double spmv_hip_time_row_softmax_launches(spmv_Handle_t handle, const void *S, void *Out, int warmup, int iters, float *ms_out);
/* The same for spmv_hip_attention (Q: m x k, K: n x k, V: n x dv, O: m x dv; DEVICE pointers). */
double spmv_hip_time_attention_launches(spmv_Handle_t handle, int k, int dv, double scale, const void *Q, long long ldq, const void *K, long long ldk,
                                        const void *V, long long ldv, void *O, long long ldo, int warmup, int iters, float *ms_out);
/* The same for spmv_hip_attention_heads (Q: m x heads*k, K: n x heads*k, V: n x heads*dv, O: m x heads*dv; DEVICE pointers). */
double spmv_hip_time_attention_heads_launches(spmv_Handle_t handle, int heads, int k, int dv, double scale, const void *Q, long long ldq, const void *K,
                                              long long ldk, const void *V, long long ldv, void *O, long long ldo, int warmup, int iters, float *ms_out);
/* The same for spmv_hip_attention_backward (Q: m x k, K: n x k, V: n x dv, G: m x dv, dQ / dK / dV or NULL; DEVICE pointers); builds the
 * transpose and restores its column indices first when dK or dV is wanted. */
double spmv_hip_time_attention_backward_launches(spmv_Handle_t handle, int k, int dv, double scale, const void *Q, long long ldq, const void *K, long long ldk,
                                                 const void *V, long long ldv, const void *G, long long ldg, void *dQ, long long lddq, void *dK, long long lddk,
                                                 void *dV, long long lddv, int warmup, int iters, float *ms_out);
/* The same for spmv_hip_attention_heads_backward (Q: m x heads*k, K: n x heads*k, V: n x heads*dv, G: m x heads*dv, dQ / dK / dV at the same
 * widths or NULL; DEVICE pointers). */
double spmv_hip_time_attention_heads_backward_launches(spmv_Handle_t handle, int heads, int k, int dv, double scale, const void *Q, long long ldq, const void *K,
                                                       long long ldk, const void *V, long long ldv, const void *G, long long ldg, void *dQ, long long lddq, void *dK,
                                                       long long lddk, void *dV, long long lddv, int warmup, int iters, float *ms_out);
/* The same for spmv_hip_attention_bias (spmv_hip_attention_heads' operands and B, NULL or `heads` planes ldb apart / one shared plane with
 * ldb = 0; DEVICE pointers). */
double spmv_hip_time_attention_bias_launches(spmv_Handle_t handle, int heads, int k, int dv, double scale, const void *Q, long long ldq, const void *K, long long ldk,
                                             const void *V, long long ldv, const void *B, long long ldb, void *O, long long ldo, int warmup, int iters, float *ms_out);
/* The same for spmv_hip_attention_bias_backward (spmv_hip_attention_heads_backward's operands, B as above or NULL, dB `heads` planes lddb apart
 * or NULL; DEVICE pointers). */
double spmv_hip_time_attention_bias_backward_launches(spmv_Handle_t handle, int heads, int k, int dv, double scale, const void *Q, long long ldq, const void *K,
                                                      long long ldk, const void *V, long long ldv, const void *B, long long ldb, const void *G, long long ldg, void *dQ,
                                                      long long lddq, void *dK, long long lddk, void *dV, long long lddv, void *dB, long long lddb, int warmup, int iters,
                                                      float *ms_out);
/* The same for spmv_hip_attention_gqa and spmv_hip_attention_gqa_backward: the bias timers' arguments plus kv_heads (K, V, dK, dV kv_heads blocks
 * wide; DEVICE pointers). */
double spmv_hip_time_attention_gqa_launches(spmv_Handle_t handle, int heads, int kv_heads, int k, int dv, double scale, const void *Q, long long ldq, const void *K,
                                            long long ldk, const void *V, long long ldv, const void *B, long long ldb, void *O, long long ldo, int warmup, int iters,
                                            float *ms_out);
double spmv_hip_time_attention_gqa_backward_launches(spmv_Handle_t handle, int heads, int kv_heads, int k, int dv, double scale, const void *Q, long long ldq, const void *K,
                                                     long long ldk, const void *V, long long ldv, const void *B, long long ldb, const void *G, long long ldg, void *dQ,
                                                     long long lddq, void *dK, long long lddk, void *dV, long long lddv, void *dB, long long lddb, int warmup, int iters,
                                                     float *ms_out);
/* The same for spmv_hip_attention_gqa_lse, spmv_hip_attention_merge and spmv_hip_attention_gqa_backward_lse: the calls' own arguments (device
   pointers; the CSR arguments left out), then the timers' warmup, iters and ms_out. */
double spmv_hip_time_attention_gqa_lse_launches(spmv_Handle_t handle, int heads, int kv_heads, int k, int dv, double scale, const void *Q, long long ldq, const void *K,
                                                long long ldk, const void *V, long long ldv, const void *B, long long ldb, void *O, long long ldo, void *L, long long ldl,
                                                int warmup, int iters, float *ms_out);
/* The same for spmv_hip_attention_gqa_lse_16 (io_type ahead of Q, o_type behind ldo, as there; DEVICE pointers). */
double spmv_hip_time_attention_gqa_lse_16_launches(spmv_Handle_t handle, int heads, int kv_heads, int k, int dv, double scale, int io_type, const void *Q, long long ldq,
                                                   const void *K, long long ldk, const void *V, long long ldv, const void *B, long long ldb, void *O, long long ldo, int o_type,
                                                   void *L, long long ldl, int warmup, int iters, float *ms_out);
double spmv_hip_time_attention_merge_launches(spmv_Handle_t handle, int heads, int dv, const void *O1, long long ldo1, const void *L1, long long ldl1, const void *O2,
                                              long long ldo2, const void *L2, long long ldl2, void *O, long long ldo, void *L, long long ldl, int warmup, int iters,
                                              float *ms_out);
double spmv_hip_time_attention_gqa_backward_lse_launches(spmv_Handle_t handle, int heads, int kv_heads, int k, int dv, double scale, const void *Q, long long ldq, const void *K,
                                                         long long ldk, const void *V, long long ldv, const void *B, long long ldb, const void *G, long long ldg, const void *O,
                                                         long long ldo, const void *L, long long ldl, void *dQ, long long lddq, void *dK, long long lddk, void *dV,
                                                         long long lddv, void *dB, long long lddb, int warmup, int iters, float *ms_out);
/* The same for spmv_hip_attention_gqa_backward_16 (io_type ahead of Q, dq_type and dkv_type ahead of dQ and dK, as there; DEVICE pointers; O and L
   both NULL or both given). */
double spmv_hip_time_attention_gqa_backward_16_launches(spmv_Handle_t handle, int heads, int kv_heads, int k, int dv, double scale, int io_type, const void *Q, long long ldq,
                                                        const void *K, long long ldk, const void *V, long long ldv, const void *B, long long ldb, const void *G, long long ldg,
                                                        const void *O, long long ldo, const void *L, long long ldl, int dq_type, void *dQ, long long lddq, int dkv_type, void *dK,
                                                        long long lddk, void *dV, long long lddv, void *dB, long long lddb, int warmup, int iters, float *ms_out);
/* spmv_hip_cg's iterations (include spmv_hip.h first: spmv_hip_cg_options): `warmup` untimed + `iters` timed RUNS of opt->max_iterations (>= 1)
   iterations each, with the stop tests disabled.  Every run starts again from B; its iterations -- multiply, cg_dot, cg_update, cg_direction --
   are enqueued back to back on the handle's stream and bracketed by two hipEvents, the start outside them; ms_out[i] (may be NULL) receives
   run i.  What X holds: without use_x0 every run starts from x = 0, so every run computes the same and the call leaves in X the bits that
   spmv_hip_cg returns for rtol = atol = 0 and the same max_iterations when none of its tests ends that solve early.  With use_x0 the FIRST run
   (a warm-up run, if there is one) starts from the guess the caller put into X; X is not put back between runs, so every later run starts from
   the X that the run before it left: only warmup = 0, iters = 1 equals the solve from that guess.  B, X and opt->Dinv must be DEVICE pointers;
   rtol, atol, check_every and history are not used.  Returns the mean ms per run, < 0 on error. */
struct spmv_hip_cg_options;
double spmv_hip_time_cg_iterations(spmv_Handle_t handle, const void *B, void *X, const struct spmv_hip_cg_options *opt, int warmup, int iters, float *ms_out);
/* spmv_hip_bicgstab's iterations, timed as spmv_hip_time_cg_iterations times spmv_hip_cg's: an iteration is multiply, bicg_rv, bicg_half,
   multiply, bicg_ts, bicg_update, bicg_direction.  The same arguments, the same rules, the same return value. */
double spmv_hip_time_bicgstab_iterations(spmv_Handle_t handle, const void *B, void *X, const struct spmv_hip_cg_options *opt, int warmup, int iters, float *ms_out);
/* spmv_hip_cg_columns' iterations, timed as spmv_hip_time_cg_iterations times spmv_hip_cg's: an iteration is the k-column multiply, ccg_dot,
   ccg_alpha, ccg_update, ccg_beta, ccg_direction.  B and X: m x k DEVICE arrays with leading dimensions ldb, ldx >= k, opt->Dinv a DEVICE vector
   of m elements or NULL; 1 <= k <= SPMV_HIP_CG_COLUMNS_MAX; k = 1 with ldb = ldx = 1 times spmv_hip_cg itself.  The same rules about what X
   holds, the same return value. */
double spmv_hip_time_cg_columns_iterations(spmv_Handle_t handle, int k, const void *B, long long ldb, void *X, long long ldx, const struct spmv_hip_cg_options *opt, int warmup,
                                           int iters, float *ms_out);
/* spmv_hip_gmres's iterations, timed as spmv_hip_time_cg_iterations times spmv_hip_cg's: iteration k is step (k - 1) mod restart + 1 of its
   cycle -- multiply, gmres_dots, gmres_coeffs, gmres_sub_dots, gmres_coeffs, gmres_sub_norm, gmres_rotate, gmres_scale -- and every restart-th
   one also the cycle's end and the restart (gmres_solve, gmres_update_x, multiply, gmres_residual, gmres_cycle, gmres_scale).  1 <= restart <=
   SPMV_HIP_GMRES_RESTART_MAX.  The same arguments otherwise, the same rules, the same return value; X holds the iterate of the last FINISHED
   cycle. */
double spmv_hip_time_gmres_iterations(spmv_Handle_t handle, const void *B, void *X, int restart, const struct spmv_hip_cg_options *opt, int warmup, int iters, float *ms_out);
/* spmv_hip_cg_mixed's iterations, timed as spmv_hip_time_cg_iterations times spmv_hip_cg's: an iteration is `low`'s multiply, cg_dot,
   cg_update, mix_direction, and behind every opt->update_every-th one (never when that is 0) the update: mix_try, `high`'s multiply,
   mix_residual, mix_resume.  The stop tests are off and every update is committed, so what is enqueued does not depend on the data.  B and
   X: DEVICE arrays of m doubles, opt->Dinv a DEVICE array of m floats or NULL; X holds the x of the last update.  The pair rules of
   spmv_hip_cg_mixed; rtol, atol, check_every, update_drop and history are not used.  Returns the mean ms per run, < 0 on error. */
struct spmv_hip_cg_mixed_options;
double spmv_hip_time_cg_mixed_iterations(spmv_Handle_t high, spmv_Handle_t low, const double *B, double *X, const struct spmv_hip_cg_mixed_options *opt, int warmup, int iters,
                                         float *ms_out);
/* spmv_hip_lsqr's iterations, timed as spmv_hip_time_cg_iterations times spmv_hip_cg's: an iteration is the multiply, lsqr_u, lsqr_unit_u, the
   transpose's multiply, lsqr_v, lsqr_step.  B: a DEVICE array of m elements, X: one of n elements; the transpose is built when it is not yet.
   spmv_hip_lsqr's handle rules; rtol, atol, ls_tol, check_every and history are not used (damp is).  Returns the mean ms per run, < 0 on error. */
struct spmv_hip_lsqr_options;
double spmv_hip_time_lsqr_iterations(spmv_Handle_t handle, const void *B, void *X, const struct spmv_hip_lsqr_options *opt, int warmup, int iters, float *ms_out);
/* out[i] = the fp64 square root of in[i] exactly as spmv_hip_gmres's kernels take it (a kernel of the same translation unit, the same
   compiler flags): n doubles each, DEVICE pointers on the current device; synchronous.  For the test that holds it against a correctly
   rounded square root; SPMV_HIP_E_ARG for n < 0, NULL or host pointers. */
int spmv_hip_gmres_device_sqrt(const double *in, double *out, long long n);
/* copies the built transpose map to host: rowptr_t (n+1 entries) and perm (nnz entries: perm[p] = CSR index in A of the entry at
   position p of A^T's CSR); either may be NULL.  SPMV_HIP_E_NOSTATE until the transpose is built. */
int spmv_hip_transpose_map(spmv_Handle_t handle, int *rowptr_t, int *perm);

#endif /* SPMV_HIP_TOOLS_H */
#if defined(__cplusplus)
}
#endif
