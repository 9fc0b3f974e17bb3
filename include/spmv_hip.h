/*
 * spmv_hip.h -- extensions of the MI355X build.  NOT part of the reference API: a program that
 * only uses spmv.h never needs this header.  Everything here is optional control around the four
 * drop-in functions; no extension changes what spmv() computes.
 *
 * Why they exist (SURVEY 8b "Errors", "Host-pointer cost", 5 "Config / flags"):
 *   - the reference API is all-void with no error channel      -> spmv_hip_last_error*()
 *   - the reference has no notion of a device or a stream      -> spmv_hip_set_stream / _set_async / _synchronize
 *   - SELL's C and sigma and CSR5's sigma are hard-wired in the reference (common.c:139-140,
 *     csr5_spmv.cpp:30)                                         -> spmv_hip_set_option (also env SPMV_HIP_<KEY>)
 *   - measurement (hipEvent per launch on the launch stream)    -> include/spmv_hip_tools.h (bench.py and tools/ only)
 */
#include "spmv_Defines.h"
#if defined(__cplusplus)
extern "C" {
#endif
#ifndef SPMV_HIP_EXT_H
#define SPMV_HIP_EXT_H

/* ---- error channel ------------------------------------------------------------------------ */
enum {
    SPMV_HIP_OK = 0,
    SPMV_HIP_E_NODEVICE = 1,   /* no usable gfx950 device / HIP runtime failure at init */
    SPMV_HIP_E_ALLOC = 2,      /* hipMalloc failed */
    SPMV_HIP_E_ARG = 3,        /* NULL / negative / inconsistent argument */
    SPMV_HIP_E_RUNTIME = 4,    /* a HIP call or kernel launch failed */
    SPMV_HIP_E_NOSTATE = 5,    /* handle has no device state (create failed or handle was cleared) */
    SPMV_HIP_E_RANGE = 6       /* nnz or padded size does not fit the index type */
};
/* Failures are also printed to stderr (env SPMV_HIP_QUIET silences that); env SPMV_HIP_ABORT_ON_ERROR makes the
 * first failure abort() the process -- for drop-in callers that never look at the error channel.
 * Code of the most recent failure on the calling thread (0 if none since the last clear). */
int spmv_hip_last_error(void);
/* Human-readable text for it ("" if none).  Valid until the next failing call on this thread. */
const char *spmv_hip_last_error_string(void);
void spmv_hip_clear_error(void);

/* ---- device / stream ---------------------------------------------------------------------- */
/* Number of visible HIP devices (0 if none or the runtime cannot initialise). */
int spmv_hip_device_count(void);
/* Launch this handle's kernels on `hip_stream` (a hipStream_t; NULL = the default stream). */
int spmv_hip_set_stream(spmv_Handle_t handle, void *hip_stream);
/* async != 0: spmv() with DEVICE x and y returns after enqueueing (stream-ordered); the caller
 * synchronises.  Default 0: spmv() returns when Y is complete, like the reference.
 * Host x or y always synchronise. */
int spmv_hip_set_async(spmv_Handle_t handle, int async);
int spmv_hip_synchronize(spmv_Handle_t handle);
/* Device blocks freed by destroy / clear / re-inspection are kept (up to SPMV_HIP_POOL_MB MiB, default an eighth of the device's memory; 0 = keep
 * nothing) and handed to the next create: on this runtime a hipMalloc that follows a large hipFree can take seconds.
 * This returns them to the driver now. */
void spmv_hip_trim_pool(void);

/* ---- values changed in place ---------------------------------------------------------------- */
/* The reference re-reads Matrix_Val on every spmv() (common.c:286-298); this library multiplies its
 * HBM-resident copy.  After changing values IN PLACE (same pattern) call this with the array (host or device
 * pointer, RowPtr[m] entries in CSR order): the values are copied to HBM and re-permuted into the schedule's
 * private layouts by device kernels -- no re-inspection, no autotune.  spmv() also watches the array by itself (option
 * "check_values"): by default a HOST Matrix_Val -- the reference's only mode -- is sample-checksummed on every call and a change of the
 * whole array is picked up without any call; SPMV_HIP_CHECK_VALUES=1 makes that a full checksum (device arrays too), at the price of
 * reading the values once more per call.  Not available on handles created with
 * option "reorder".  Returns 0 or an SPMV_HIP_E_* code. */
int spmv_hip_update_values(spmv_Handle_t handle, const void *Matrix_Val);

/* ---- k right-hand sides: Y = A X ------------------------------------------------------------
 * Y = A X for k vectors at once: X is n x k, Y is m x k, both ROW-MAJOR with leading dimensions
 * (X[j*ldx + c], Y[i*ldy + c], ldx >= k, ldy >= k; host or device pointers).  Returns 0 or an SPMV_HIP_E_* code.
 *   - The CSR arguments follow spmv()'s rules: m and the pointers seen at create -> the resident matrix; others -> that matrix is
 *     re-inspected; option "check_values", in-place value changes and spmv_hip_update_values apply as for spmv().
 *   - Only the first k entries of every Y row are written (empty rows: zeros); the padding of Y is never touched, that of X never read.
 *     Offsets are 64-bit: n*ldx and m*ldy may exceed 2^31 elements.
 *   - A is read once per panel of up to 16 (fp64) / 32 (fp32) columns.  Every (row, column) is summed in an order fixed by the matrix:
 *     results are bit-identical run to run and across host / device pointers, ldx / ldy and stream / async settings.
 *     k = 1 with ldx = ldy = 1 runs the handle's spmv() schedule: bit-identical to spmv().
 *   - The handle's stream and async setting apply as for spmv(); host X / Y are staged through handle-owned HBM buffers of n*k and m*k
 *     elements, allocated at first use, freed at destroy / clear / re-inspection and counted in spmv_hip_info.device_bytes.
 *   - Option "reorder" handles multiply the resident P A P^T: the caller gathers X rows and scatters Y rows by handle->index, as for spmv().
 *     Split and cache-blocked handles multiply the resident CSR itself.
 *   - Column indices: with option "keep_columns" = 0 (default) create() may have released the resident ColIdx copy.  The first call
 *     (k > 1 or ld > 1) then copies it back from the call's ColIdx -- by the pointer rule the create-time array, which must therefore still
 *     hold the create-time indices (permuted like the matrix on "reorder" handles): device_bytes grows by 4 B per non-zero from then on,
 *     and spmv() computes exactly what it did before.
 *   - Errors (SPMV_HIP_E_ARG, Y untouched): k < 1, ldx < k, ldy < k; a NULL X or Y when m > 0; multi-GPU handles (option "gpus",
 *     spmv_hip_create_handle_from_blocks); host_rows handles.  A cleared or failed handle: SPMV_HIP_E_NOSTATE.  Every failure is also
 *     reported through spmv_hip_last_error(). */
int spmv_hip_spmm(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                  const void *Matrix_Val, int k, const void *X, long long ldx, void *Y, long long ldy);

/* ---- the transpose: y = A^T x ----------------------------------------------------------------
 * y = A^T x: X has m entries (A's rows), Y has n entries (A's columns, as at create); host or device pointers.  Returns 0 or an SPMV_HIP_E_* code.
 *   - A^T is built on the device from the resident matrix at the first call (or at spmv_hip_prepare_transpose): row j of A^T lists its
 *     entries in ascending row of A, so the transpose is a function of the matrix alone.  It is then planned and inspected exactly as create()
 *     would plan a matrix of that shape, with the handle's requested method and options (spmv_hip_get_transpose_info reports the result).
 *   - The CSR arguments follow spmv()'s rules: m and the pointers seen at create -> the resident matrix; others -> that matrix is
 *     re-inspected and the transpose dropped (rebuilt at the next call); option "check_values", in-place value changes and
 *     spmv_hip_update_values apply as for spmv(): the next transpose call multiplies the new values (gathered again on the device; spmv()
 *     itself pays nothing for this).
 *   - Results are bit-identical run to run and across host / device pointers, stream and async settings (unless the handle was created
 *     with option "deterministic" = 0, as for spmv()).  m = 0 or nnz = 0 writes n zeros; empty columns of A give zero entries of Y.
 *   - The handle's stream and async setting apply, also when changed later; host X / Y are staged as in spmv().
 *   - Option "reorder" handles multiply the transpose of the resident P A P^T, i.e. P A^T P^T: the caller gathers X and scatters Y by
 *     handle->index, as for spmv().  Split and cache-blocked handles transpose the resident CSR itself.
 *   - Column indices: with option "keep_columns" = 0 create() may have released the resident ColIdx copy.  The build then copies it back
 *     from the create-time array (which must therefore still hold the create-time indices, permuted like the matrix on "reorder" handles)
 *     and releases it again afterwards: spmv() computes exactly what it did before.
 *   - Memory: perm (4 B per non-zero), A^T's CSR arrays and its schedule, counted in spmv_hip_info.device_bytes of the handle and freed at
 *     destroy / clear / re-inspection.
 *   - Errors (SPMV_HIP_E_ARG, Y untouched): multi-GPU handles (option "gpus", spmv_hip_create_handle_from_blocks); host_rows handles; a NULL
 *     X when m > 0 or a NULL Y when n > 0.  A cleared or failed handle: SPMV_HIP_E_NOSTATE.  Every failure is also reported through
 *     spmv_hip_last_error(). */
int spmv_hip_spmv_transpose(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                            const void *Matrix_Val, const void *X, void *Y);
/* build the transposed schedule now instead of at the first call (create-time cost, outside a timed loop) */
int spmv_hip_prepare_transpose(spmv_Handle_t handle);
/* spmv_hip_get_transpose_info: below, after spmv_hip_info */

/* ---- the transpose for k right-hand sides: Y = A^T X -------------------------------------------
 * Y = A^T X for k vectors at once: X is m x k (A's rows), Y is n x k (A's columns), both ROW-MAJOR with leading dimensions
 * (X[i*ldx + c], Y[j*ldy + c], ldx >= k, ldy >= k; host or device pointers).  Returns 0 or an SPMV_HIP_E_* code.
 *   - The transpose is the one spmv_hip_spmv_transpose builds (at the first call of either, or at spmv_hip_prepare_transpose), and the CSR
 *     arguments, option "check_values", in-place value changes, spmv_hip_update_values and later stream / async changes are handled as there.
 *   - The multiply is spmv_hip_spmm's executor on A^T: only the first k entries of every Y row are written (empty columns of A: zeros), Y's
 *     padding is never touched, X's never read; offsets are 64-bit.  Every column has the bits spmv_hip_spmm gives on a handle created from
 *     A^T itself (rows of A^T listing their entries in ascending row of A): identical run to run and across ldx / ldy, host / device
 *     pointers, stream and async settings.  k = 1 with ldx = ldy = 1 runs A^T's own schedule: bit-identical to spmv_hip_spmv_transpose.
 *   - Column indices: the transposed schedule may have released ITS resident column indices at the end of its build (option "keep_columns"
 *     = 0).  The first call with k > 1 or ld > 1 then rebuilds them on the device from what the handle keeps (RowPtr and perm; the caller's
 *     arrays are not read): spmv_hip_info.device_bytes grows by 4 B per non-zero from then on, and spmv() and spmv_hip_spmv_transpose
 *     compute exactly what they did before.
 *   - Memory: the batch table, the long-row list and the staging buffers of host X / Y (m*k and n*k elements) belong to the transpose; they
 *     are counted in the handle's spmv_hip_info.device_bytes and freed with it: destroy / clear / re-inspection.
 *   - Option "reorder" handles multiply P A^T P^T: the caller gathers X rows and scatters Y rows by handle->index.
 *   - Errors (SPMV_HIP_E_ARG, Y untouched): k < 1, ldx < k, ldy < k; a NULL X or Y; multi-GPU handles (option "gpus",
 *     spmv_hip_create_handle_from_blocks); host_rows handles.  A cleared or failed handle: SPMV_HIP_E_NOSTATE.  Every failure is also
 *     reported through spmv_hip_last_error(). */
int spmv_hip_spmm_transpose(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                            const void *Matrix_Val, int k, const void *X, long long ldx, void *Y, long long ldy);

/* ---- the sampled dense-dense product: Out = (U V^T) on A's pattern --------------------------------
 * Out[p] = sum over c < k of U[i*ldu + c] * V[j*ldv + c] for every stored entry p of the resident matrix, i its row and j = ColIdx[p]:
 * U is m x k, V is n x k, ROW-MAJOR with leading dimensions ldu, ldv >= k; Out has RowPtr[m] elements in CSR order, in the handle's
 * precision; each of U, V and Out may be a host or a device pointer.  A's VALUES are not used: with U = dL/dY and V = X this is
 * dL/dMatrix_Val of Y = A X.  Returns 0 or an SPMV_HIP_E_* code.
 *   - The CSR arguments follow spmv()'s rules (another matrix is re-inspected first).  Split and cache-blocked handles use the resident
 *     CSR itself.  Option "reorder" handles return SPMV_HIP_E_ARG: the resident matrix is P A P^T, whose entry order is not the caller's
 *     (as for spmv_hip_update_values).
 *   - One launch; RowPtr and ColIdx are read once per call whatever k is, the entries are split evenly over the wavefronts (a long row is
 *     shared by many), nothing is built per matrix.  Exactly the RowPtr[m] elements of Out are written, nothing else; the padding of U and V
 *     is never read.  nnz = 0 or m = 0 returns 0 and writes nothing.
 *   - Summation order of an entry: a function of k and the value type alone.  With W = 2 (fp64) / 4 (fp32) columns per lane and L = the
 *     smallest of 1, 2, 4, 8 with L*W >= k (8 beyond that), lane l of L adds the columns c = l*W + t + q*L*W < k in the order q = 0, 1, ..
 *     outermost, t = 0 .. W-1 innermost -- the first product a plain multiplication, every further one an fma onto the chain; a lane
 *     without a column holds -0, the identity of IEEE addition -- and the lanes' sums are added as ((l0 + l1) + (l2 + l3)) + ((l4 + l5) + (l6 + l7)) (L = 8; the left half
 *     for L = 4; l0 + l1 for L = 2).  Results are therefore bit-identical across ldu / ldv, alignment and load width, host / device
 *     pointers, stream and async settings, the handle's method and the entry's position.  k = 1: Out[p] is the single correctly rounded
 *     product U[i] * V[j] (signed zeros, subnormals, infinities and NaN as IEEE 754 has them); for any k a zero result is -0 exactly when
 *     every one of the k products is -0, as in any sequential IEEE summation.
 *   - The handle's stream and async setting apply as for spmv(); host U / V / Out are staged through handle-owned HBM buffers (m*k, n*k and
 *     nnz elements), allocated at first use, freed at destroy / clear / re-inspection and counted in spmv_hip_info.device_bytes.
 *   - Column indices: as for spmv_hip_spmm -- when create() released the resident ColIdx copy (option "keep_columns" = 0), the first call
 *     copies it back from the create-time array: device_bytes grows by 4 B per non-zero from then on, spmv() is unchanged.
 *   - Errors (SPMV_HIP_E_ARG, Out untouched): k < 1, ldu < k, ldv < k; a NULL U, V or Out while nnz > 0; multi-GPU, host_rows and
 *     "reorder" handles.  A cleared or failed handle: SPMV_HIP_E_NOSTATE.  Every failure is also reported through spmv_hip_last_error(). */
int spmv_hip_sddmm(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                   const void *Matrix_Val, int k, const void *U, long long ldu, const void *V, long long ldv, void *Out);

/* ---- the row softmax over A's pattern, and its backward -------------------------------------------
 * spmv_hip_row_softmax:          Out[p] = exp(S[p] - M_i) / Z_i,  i = the row of entry p,  M_i = max over row i of S,
 *                                Z_i = sum over row i of exp(S[q] - M_i)
 * spmv_hip_row_softmax_backward: Out[p] = P[p] * (G[p] - D_i),  D_i = sum over row i of P[q] * G[q]   (dL/dS from P = softmax(S), G = dL/dP)
 * S, P, G and Out hold RowPtr[m] elements in CSR order, in the handle's precision; each may be a host or a device pointer.  With
 * spmv_hip_sddmm before and spmv_hip_spmm (values = P) after, softmax_rows(Q K^T on A's pattern) V runs on this library's kernels, forward
 * and backward.  Returns 0 or an SPMV_HIP_E_* code.
 *   - The CSR arguments follow spmv()'s rules (another matrix is re-inspected first).  Split and cache-blocked handles use the resident
 *     RowPtr itself.  Option "reorder" handles return SPMV_HIP_E_ARG: the entry order of P A P^T is not the caller's.
 *   - Only the row structure is read: ColIdx and A's values are never touched, and a resident ColIdx copy that create() released (option
 *     "keep_columns" = 0) stays released -- spmv_hip_info.device_bytes grows by the operation's own tables and staging buffers, never by
 *     4 B per non-zero.
 *   - Writes: exactly the RowPtr[m] elements of Out; empty rows write nothing; m = 0 or nnz = 0 returns 0 and writes nothing.  Out may be
 *     the very same pointer as S (forward) or as G (backward), with the same bits as out of place; any other overlap is undefined.
 *   - Arithmetic: the maximum is subtracted, so every finite row gives finite results whatever its magnitude; exp / expf of the device math
 *     library (not the fast intrinsics), one subtraction before it and one division after it.  The backward's map is one subtraction and
 *     one multiplication.  No operation is contracted that is not written as an fma below.
 *   - Special values, as torch.softmax has them on the row: a NaN anywhere in a row, a +inf, or a row of only -inf makes that whole row NaN
 *     (the maximum drops a NaN, the sum restores it) and no other row is affected; a -inf beside finite scores gives an exact +0; a row of
 *     length 1 gives exactly 1 for a finite S.
 *   - Summation order of a row (Z_i, D_i): a function of the row's length and the value type alone.  Rows of up to 512 entries: with W = 1
 *     for a length <= 1, else the smallest power of two >= the length, 64 at the most, lane t of W chains the terms t, t + W, t + 2 W, ..
 *     in that order -- the first term as it is (forward: exp(S - M); backward: the plain product P * G), every further one added onto the
 *     chain (forward: a plain addition; backward: fma(P, G, chain)); a lane without a term holds -0, the identity of IEEE addition -- and
 *     the W chains are added as a balanced tree over neighbours, ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7)) and so on.  Longer rows:
 *     thread t of 256 chains the terms t, t + 256, .. the same way, each 64 consecutive chains are added by that tree and the four sums as
 *     (w0 + w1) + (w2 + w3).  A row's output bits therefore do not depend on where the row sits in the matrix, on its neighbours, the
 *     handle's method, host or device pointers, stream and async settings: results are identical run to run.  No floating-point atomics;
 *     no workgroup waits on another.
 *   - The handle's stream and async setting apply as for spmv(); host arrays are staged through handle-owned HBM buffers (nnz elements
 *     each) allocated at first use; with the batch table and the long-row list (shared with spmv_hip_spmm, built at the first call of
 *     either) they are counted in spmv_hip_info.device_bytes and freed at destroy / clear / re-inspection.
 *   - Errors (SPMV_HIP_E_ARG, Out untouched): a NULL handle; a NULL array while nnz > 0; multi-GPU, host_rows and "reorder" handles.  A
 *     cleared or failed handle: SPMV_HIP_E_NOSTATE.  Every failure is also reported through spmv_hip_last_error(). */
int spmv_hip_row_softmax(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                         const void *Matrix_Val, const void *S, void *Out);
int spmv_hip_row_softmax_backward(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                                  const void *Matrix_Val, const void *P, const void *G, void *Out);

/* ---- sparse attention in one pass: O = softmax_rows(scale * Q K^T on A's pattern) V ---------------
 * O[i*ldo + c] = sum over the stored entries p of row i of P_p * V[j_p*ldv + c] for c < dv, where j_p = ColIdx[p],
 * P = softmax over row i of t_p = scale * sum over c < k of Q[i*ldq + c] * K[j_p*ldk + c].  Q is m x k, K is n x k, V is n x dv, O is m x dv,
 * ROW-MAJOR with leading dimensions ldq, ldk >= k and ldv, ldo >= dv, in the handle's precision; each may be a host or a device pointer; K
 * and V may be the same pointer; O must not overlap an input.  `scale` is converted once to the handle's precision.  A's VALUES are not
 * read, and the handle's resident values are NOT MODIFIED: spmv() before and after computes the same.  This is the composition
 * spmv_hip_sddmm, * scale, spmv_hip_row_softmax, spmv_hip_spmm (values = P) without the scores or P ever stored in the caller's memory --
 * and with the composition's bits.  Returns 0 or an SPMV_HIP_E_* code.
 *   - The CSR arguments follow spmv()'s rules (another matrix is re-inspected first).  Split and cache-blocked handles use the resident
 *     CSR itself.  Option "reorder" handles return SPMV_HIP_E_ARG: the resident matrix is P A P^T.
 *   - Writes: exactly the first dv elements of each of the m rows of O; a row without entries gets dv zeros (+0); the padding of Q, K, V
 *     and O is never read or written; offsets are 64-bit.  m = 0 writes nothing; nnz = 0 writes the zeros.
 *   - Arithmetic and order -- the composition's, step by step, so the result is a function of the matrix, k, dv and the value type alone
 *     (not of ld, alignment, access width, host / device pointers, stream and async settings, the handle's method, run to run):
 *       1. s_p is the dot in spmv_hip_sddmm's order for this k (above).
 *       2. t_p = s_p * scale: one plain multiplication.
 *       3. M_i, Z_i and P_p = exp(t_p - M_i) / Z_i are spmv_hip_row_softmax's: its order by row length, exp / expf of the device math
 *          library, one subtraction and one division.
 *       4. O[i, c] is spmv_hip_spmm's chain.  Rows of up to 512 entries: acc = +0, then acc = fma(P_p, V[j_p, c], acc) in CSR order.  Longer
 *          rows: 64 segments of ceil(len / 64) entries, each chained from +0, the partial sums added left to right.
 *     No other operation is contracted.  Special values follow from these steps: a NaN, a +inf or only -inf among a row's scores makes that
 *     row of O NaN, and only that row; a -inf beside finite scores weighs its V row with an exact +0.
 *   - One launch for the rows of up to 512 entries (a wavefront per batch of whole rows; scores and P live in LDS) and one for the longer
 *     rows (a workgroup each; their scores are parked in a handle-owned array of sum-of-their-lengths elements).  No floating-point atomics;
 *     no workgroup waits on another.
 *   - The handle's stream and async setting apply as for spmv(); host Q / K / V / O are staged through handle-owned HBM buffers (m*k, n*k,
 *     n*dv and m*dv elements) allocated at first use; with the batch table and the long-row list (shared with spmv_hip_spmm) and the long
 *     rows' parking space they are counted in spmv_hip_info.device_bytes and freed at destroy / clear / re-inspection.
 *   - Column indices: as for spmv_hip_spmm -- when create() released the resident ColIdx copy (option "keep_columns" = 0), the first call
 *     copies it back from the create-time array: device_bytes grows by 4 B per non-zero from then on, spmv() is unchanged.
 *   - Errors (SPMV_HIP_E_ARG, O untouched): a NULL handle; k < 1, dv < 1, ldq < k, ldk < k, ldv < dv, ldo < dv; a NULL Q, K, V or O while
 *     m > 0; multi-GPU, host_rows and "reorder" handles.  A cleared or failed handle: SPMV_HIP_E_NOSTATE.  Every failure is also reported
 *     through spmv_hip_last_error(). */
int spmv_hip_attention(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                       const void *Matrix_Val, int k, int dv, double scale,
                       const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                       void *O, long long ldo);

/* ---- sparse attention for H heads over the same pattern, in the same one pass ---------------------
 * Q is m x heads*k, K is n x heads*k, V is n x heads*dv, O is m x heads*dv, ROW-MAJOR with leading dimensions ldq, ldk >= heads*k and
 * ldv, ldo >= heads*dv, in the handle's precision -- the (rows, heads, k) layout: head h of a row is its columns [h*k, (h+1)*k) of Q and K
 * and [h*dv, (h+1)*dv) of V and O.  k, dv and `scale` are ONE head's.  Each operand may be a host or a device pointer; K
 * and V may be the same pointer; O must not overlap an input.  Returns 0 or an SPMV_HIP_E_* code.
 *   - Bits: for every h, head h's block of O has exactly the bits that
 *       spmv_hip_attention(handle, .., k, dv, scale, Q + h*k, ldq, K + h*k, ldk, V + h*dv, ldv, O + h*dv, ldo)
 *     writes (pointer arithmetic in elements).  heads = 1 IS spmv_hip_attention.  So spmv_hip_attention's arithmetic and order, its
 *     special-value rules and its invariance (ld, alignment, access width, host / device pointers, stream and async settings, the handle's
 *     method, run to run) hold head by head; a NaN row in one head does not touch another head of the same row.
 *   - Writes: exactly the first heads*dv elements of each of the m rows of O; a row without entries gets +0 in all of them; the padding
 *     of Q, K, V and O is never read or written; offsets are 64-bit.  m = 0 writes nothing; nnz = 0 writes the zeros.
 *   - A's VALUES are not read, and the handle's resident values are NOT MODIFIED: spmv() before and after computes the same.
 *   - Still one launch for the rows of up to 512 entries and one for the longer rows, whatever heads is: the head loop is inside the
 *     kernels.  RowPtr and ColIdx of a chunk of short rows are read once and kept in LDS for every head; the scores' LDS and the long
 *     rows' parking space are reused head after head, so spmv_hip_info.device_bytes does not depend on heads when the operands are device
 *     pointers.  16-byte accesses additionally need k and dv to be multiples of 16 bytes when heads > 1 (every head's first column must
 *     be aligned); element accesses otherwise -- the width changes no bit.  No floating-point atomics; no workgroup waits on another.
 *   - The CSR arguments, the stream and async setting, the staging of host operands (at widths heads*k and heads*dv, the same four
 *     buffers), the column indices (option "keep_columns") and the handle kinds: as for spmv_hip_attention.
 *   - Errors (SPMV_HIP_E_ARG before the handle is looked at, O untouched): a NULL handle; heads < 1, k < 1, dv < 1; heads*k or heads*dv
 *     not representable in int; ldq, ldk < heads*k; ldv, ldo < heads*dv; a NULL Q, K, V or O while m > 0.  Multi-GPU, host_rows and
 *     "reorder" handles: SPMV_HIP_E_ARG.  A cleared or failed handle: SPMV_HIP_E_NOSTATE.  Every failure is also reported through
 *     spmv_hip_last_error(). */
int spmv_hip_attention_heads(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                             const void *Matrix_Val, int heads, int k, int dv, double scale,
                             const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                             void *O, long long ldo);

/* ---- the gradients of spmv_hip_attention in two passes over A: dQ, dK, dV -----------------------
 * With G = dL/dO (m x dv) and t_p, P_p as in spmv_hip_attention:  dP_p = sum over c < dv of G[i*ldg + c] * V[j_p*ldv + c],
 * D_i = sum over row i of P_q dP_q,  dS_p = P_p (dP_p - D_i) scale,  dQ = A_dS K (m x k),  dK = A_dS^T Q (n x k),  dV = A_P^T G (n x dv), where A_X
 * is A's pattern holding X as values.  All operands are ROW-MAJOR with leading dimensions (ldq, ldk, lddq, lddk >= k; ldv, ldg, lddv >= dv),
 * in the handle's precision; each may be a host or a device pointer; K and V may be the same pointer; no output may overlap an input or
 * another output.  A NULL output means "not wanted": nothing is computed for it; when dK and dV are both NULL the transpose is neither built
 * nor read; when all three are NULL the call returns 0 after argument checking.  A's VALUES are not read, and the handle's resident values are
 * NOT MODIFIED: spmv(), spmv_hip_spmv_transpose() and spmv_hip_spmm compute the same before and after.  This is the composition
 * spmv_hip_sddmm, * scale, spmv_hip_row_softmax, spmv_hip_sddmm(G, V), spmv_hip_row_softmax_backward, * scale, spmv_hip_spmm (values dS),
 * spmv_hip_spmm_transpose (values P, values dS) without a single update of the handle's values -- and with the composition's bits.
 * Returns 0 or an SPMV_HIP_E_* code.
 *   - The CSR arguments follow spmv()'s rules (another matrix is re-inspected first).  Option "reorder" handles return SPMV_HIP_E_ARG.
 *   - Writes: exactly the first k (dQ, dK) or dv (dV) elements of each row of each requested output; padding is never read or written.  Empty
 *     rows of A give +0 rows of dQ, empty columns +0 rows of dK and dV; nnz = 0 writes those zeros; m = 0 writes nothing to dQ and n zero rows
 *     to dK and dV (spmv_hip_spmm_transpose's rule).
 *   - Arithmetic and order -- the composition's, step by step, so the result is a function of the matrix, k, dv and the value type alone
 *     (not of ld, alignment, access width, host / device pointers, stream and async settings, the handle's method, which outputs are wanted):
 *       1. t_p and P_p are exactly spmv_hip_attention's steps 1-3.
 *       2. dP_p is the dot of G[i, :dv] and V[j_p, :dv] in spmv_hip_sddmm's order for dv columns.
 *       3. D_i is spmv_hip_row_softmax_backward's sum by row length: the first term a plain product, every further one fma(P, dP, chain), then
 *          its tree.
 *       4. dS_p = P_p * (dP_p - D_i): one subtraction and one multiplication; then * scale, one more plain multiplication.
 *       5. dQ[i, c] is spmv_hip_spmm's chain with values dS and X = K (the k > 1 / ld > 1 executor, also when k = 1): rows of up to 512 entries
 *          chain from +0 in CSR order, longer rows use 64 segments added left to right.
 *       6. dV[j, c] and dK[j, c] are spmv_hip_spmm_transpose's chain on the handle's device-built transpose: row j of A^T lists its entries in
 *          ascending row of A, then CSR order; dV uses values P and X = G, dK values dS and X = Q; the 512 / 64-segment rule applies to the
 *          column's length.
 *     No other operation is contracted.
 *   - Two passes.  Over A's rows: one launch for the rows of up to 512 entries (a wavefront per batch of whole rows; t, P, dP and dS live in
 *     LDS) and one for the longer rows (a workgroup each); they compute dQ and leave P and dS in two handle-owned arrays of nnz elements
 *     each.  Over A^T's rows, only when dK or dV is wanted: ceil(max(k, dv) / KP) launches (KP = 16 fp64 / 32 fp32) per length class, each
 *     gathering P and dS through the transpose's index map for panel r of both outputs.  No floating-point atomics; no workgroup waits on
 *     another; no scratch memory.
 *   - Memory: the two nnz-sized arrays are allocated at the first call, the transpose (as for spmv_hip_spmm_transpose; its values are not
 *     read) at the first call that wants dK or dV; host operands are staged through handle-owned HBM buffers allocated at first use.  All are
 *     counted in spmv_hip_info.device_bytes and freed at destroy / clear / re-inspection.  The handle's stream and async setting apply as for
 *     spmv().  Column indices: as for spmv_hip_attention.
 *   - Errors (SPMV_HIP_E_ARG, every output untouched): a NULL handle; k < 1, dv < 1; a leading dimension below its width (of the requested
 *     outputs only); a NULL Q, K, V or G while m > 0; multi-GPU, host_rows and "reorder" handles.  A cleared or failed handle:
 *     SPMV_HIP_E_NOSTATE.  Every failure is also reported through spmv_hip_last_error(). */
int spmv_hip_attention_backward(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                                const void *Matrix_Val, int k, int dv, double scale,
                                const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                                const void *G, long long ldg,            /* dL/dO, m x dv */
                                void *dQ, long long lddq,                /* m x k,  or NULL: not wanted */
                                void *dK, long long lddk,                /* n x k,  or NULL */
                                void *dV, long long lddv);               /* n x dv, or NULL */

/* ---- the gradients of spmv_hip_attention_heads: all heads in two passes per group of heads -----------
 * The layout is spmv_hip_attention_heads': Q and dQ are m x heads*k, K and dK n x heads*k, V and dV n x heads*dv, G = dL/dO m x heads*dv, all
 * row-major with leading dimensions at least the full widths; k, dv and scale are ONE head's; each operand may be a host or a device pointer; a
 * NULL output means "not wanted", exactly as in spmv_hip_attention_backward.  For every h, head h's block of every wanted output has exactly
 * the bits spmv_hip_attention_backward writes on the h-th column slices (pointers advanced by h*k and h*dv, the same leading dimensions);
 * heads = 1 IS spmv_hip_attention_backward.  Everything that section promises -- the order, the special values, the invariance under ld,
 * alignment, access width, pointer kind, stream, async, method and which outputs are wanted -- therefore holds head by head; a NaN row in one
 * head touches no other head.  A's VALUES are not read, and the handle's resident values are NOT MODIFIED.  Returns 0 or an SPMV_HIP_E_* code.
 *   - Writes: exactly the first heads*k (dQ, dK) or heads*dv (dV) elements of each row of each wanted output; padding is never read or
 *     written.  Empty rows, empty columns, nnz = 0 and m = 0: the single-head call's rules, at the full widths.
 *   - Groups of heads.  The two handle-owned arrays become HG planes of nnz elements each, plane g one head's P or dS in CSR order, and a call
 *     runs ceil(heads / HG) rounds: one row pass and one column pass over HG heads, the head loop INSIDE the kernels -- so per round the
 *     pattern, the chunking and the transpose's index map are paid once and the launch count is that of one single-head call.  HG: option
 *     "attention_backward_heads" = n > 0 means at most n heads per round; 0 (default) the largest HG <= heads with 2*HG*s*nnz bytes (s = the
 *     value size) within one eighth of the device's memory -- the device pool's default share, used as a bound on memory, not as a measured
 *     optimum -- and at least 1.  The option changes NO BIT, only memory and the number of rounds.
 *   - Memory: the planes are allocated or grown (never shrunk) to what a call needs: a handle that only sees single-head calls holds 2*s*nnz
 *     bytes, the first call with HG > 1 grows spmv_hip_info.device_bytes to 2*HG*s*nnz, an identical second call grows nothing.  Host operands
 *     are staged through spmv_hip_attention_backward's seven buffers at the full widths.  Freed at destroy / clear / re-inspection.
 *   - 16-byte accesses additionally need k and dv to be multiples of 16 bytes when heads > 1; element accesses otherwise -- the width changes
 *     no bit.  No floating-point atomics; no workgroup waits on another; no scratch memory.
 *   - Errors (SPMV_HIP_E_ARG before the handle's state is looked at, every output untouched): a NULL handle; heads, k or dv < 1; heads*k or
 *     heads*dv not representable in int; a leading dimension below its full width (of the requested outputs only); a NULL Q, K, V or G while
 *     m > 0.  Multi-GPU, host_rows and "reorder" handles: SPMV_HIP_E_ARG.  A cleared or failed handle: SPMV_HIP_E_NOSTATE.  All outputs NULL:
 *     0 right after argument checking (the handle's state is not looked at).  Every failure is also reported through spmv_hip_last_error(). */
int spmv_hip_attention_heads_backward(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                                      const void *Matrix_Val, int heads, int k, int dv, double scale,
                                      const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                                      const void *G, long long ldg,            /* dL/dO, m x heads*dv */
                                      void *dQ, long long lddq,                /* m x heads*k,  or NULL: not wanted */
                                      void *dK, long long lddk,                /* n x heads*k,  or NULL */
                                      void *dV, long long lddv);               /* n x heads*dv, or NULL */

/* ---- sparse attention with an additive bias per head and stored entry -----------------------------
 * spmv_hip_attention_heads with  t_p = (s_p * scale) + B_p  in place of its step 2: edge biases of graph transformers, relative-position and
 * ALiBi biases on a band, additive masks (-inf on an entry) that vary per head or per call without another handle.  Everything else -- the
 * layout of Q, K, V and O, k, dv and scale as ONE head's, the writes, steps 1, 3 and 4, the launches, the CSR arguments, the stream and async
 * setting, the column indices, the handle kinds -- is that section's.  A's VALUES are not read and the resident values are NOT MODIFIED.
 *   - B holds bias PLANES in the handle's precision: B[h*ldb + p] is the bias of head h on entry p of the caller's CSR order (the order of
 *     ColIdx and Matrix_Val).  ldb >= nnz: one plane per head; ldb == 0: one plane shared by all heads.  Host or device pointer.  B is only
 *     read, and may be the very array passed as Matrix_Val (edge weights as bias).  Element accesses: B needs no alignment.
 *   - The one new step: t_p = (s_p * scale) + B_p is one plain multiplication followed by one plain addition, NEVER an fma -- the bits of the
 *     composition spmv_hip_sddmm, * scale, + B, spmv_hip_row_softmax, spmv_hip_spmm (values = P), head by head.  The result is a function of
 *     the matrix, k, dv, the value type and B's values alone (not of ldb, shared or per-head planes holding the same values, pointer kind, ..).
 *   - B == NULL: ldb is ignored and the call IS spmv_hip_attention_heads, to the bit.
 *   - Special values follow from the steps: a -inf bias beside finite scores gives that entry an exact +0 weight; a row whose biases are all
 *     -inf, or that holds a NaN or +inf, is NaN in O for that head and that row only.
 *   - Memory: a host B is staged through one more handle-owned buffer (the planes packed, allocated at first use, counted in
 *     spmv_hip_info.device_bytes, freed with the others); with device operands device_bytes grows by nothing over spmv_hip_attention_heads.
 *   - Errors: spmv_hip_attention_heads' (SPMV_HIP_E_ARG before the handle is looked at, O untouched), and ldb < 0 (with a B) with them; once nnz is
 *     known, 0 < ldb < nnz: SPMV_HIP_E_ARG, O untouched.  Handle kinds and SPMV_HIP_E_NOSTATE as there. */
int spmv_hip_attention_bias(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                            const void *Matrix_Val, int heads, int k, int dv, double scale,
                            const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                            const void *B, long long ldb,            /* bias planes, or NULL: spmv_hip_attention_heads */
                            void *O, long long ldo);

/* ---- the gradients of spmv_hip_attention_bias: dQ, dK, dV and dB -------------------------------------
 * spmv_hip_attention_heads_backward with t_p = (s_p * scale) + B_p as in spmv_hip_attention_bias, and one more output:
 *   dB_p = P_p * (dP_p - D_i)   -- spmv_hip_row_softmax_backward's output: one subtraction and one multiplication --
 * the value from which dS_p = dB_p * scale is made as before; dQ, dK and dV follow from dS exactly as there.  B is laid out as in
 * spmv_hip_attention_bias (ldb == 0: shared; else >= nnz).  dB always has `heads` planes, dB[h*lddb + p] with lddb >= nnz, host or device
 * pointer, NULL = not wanted; a shared bias' gradient is the sum of the planes, which is the caller's to take.
 *   - B == NULL: ldb is ignored; dQ, dK and dV are spmv_hip_attention_heads_backward's to the bit, and dB is still the formula above.
 *   - Special values: where B_p = -inf beside finite scores, P_p = +0 and dB_p = +-0.
 *   - Which passes run: dB is written by the row pass alone.  Only dB wanted: the row pass runs, computes no dQ and stores nothing for the
 *     column pass, and the transpose is neither built nor read.  All four outputs NULL: 0 right after argument checking.
 *   - Option "attention_backward_heads" changes no bit of dB either: dB goes straight to the caller's plane of each head, not through the
 *     handle's planes.  Which outputs are wanted changes no bit of any of them.
 *   - Writes: exactly the first nnz elements of each of the `heads` planes of dB; the padding between planes is never read or written.
 *   - Memory: host B / dB are staged through two more handle-owned buffers (shared with spmv_hip_attention_bias); with device operands
 *     device_bytes grows by nothing over spmv_hip_attention_heads_backward.
 *   - Errors: spmv_hip_attention_heads_backward's (SPMV_HIP_E_ARG before the handle's state is looked at, every output untouched), and
 *     ldb < 0 (with a B) or lddb < 0 (with a dB) with them; once nnz is known, 0 < ldb < nnz, or dB != NULL with lddb < nnz: SPMV_HIP_E_ARG, every output untouched. */
int spmv_hip_attention_bias_backward(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                                     const void *Matrix_Val, int heads, int k, int dv, double scale,
                                     const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                                     const void *B, long long ldb,            /* bias planes, or NULL */
                                     const void *G, long long ldg,            /* dL/dO, m x heads*dv */
                                     void *dQ, long long lddq,                /* m x heads*k,  or NULL: not wanted */
                                     void *dK, long long lddk,                /* n x heads*k,  or NULL */
                                     void *dV, long long lddv,                /* n x heads*dv, or NULL */
                                     void *dB, long long lddb);               /* heads planes of nnz, or NULL */

/* ---- grouped-query sparse attention: `heads` query heads over `kv_heads` K / V heads (GQA; kv_heads == 1: MQA) --------------
 * spmv_hip_attention_bias with fewer K / V heads than query heads.  Q and O are `heads` blocks wide as there; K is n x kv_heads*k and V is
 * n x kv_heads*dv (ldk, ldv are checked against THOSE widths); heads % kv_heads == 0 and, with gs = heads / kv_heads, query head h uses K / V head
 * h / gs -- the consecutive grouping of repeat_interleave.  B stays a plane per QUERY head (ldb == 0: one shared plane; B == NULL: no bias).
 *   - Head h's block of O has exactly the bits spmv_hip_attention_bias writes with ONE head on Q + h*k, K + (h/gs)*k, V + (h/gs)*dv, O + h*dv and
 *     plane h of B.  kv_heads == heads IS spmv_hip_attention_bias, to the bit.  K and V are never expanded: a host K / V is staged at its
 *     kv_heads width, and device_bytes is spmv_hip_attention_heads'.
 *   - 16-byte accesses need k and dv to be multiples of 16 bytes when heads > 1, as there; the access width changes no bit.
 *   - Errors: spmv_hip_attention_bias', and kv_heads < 1, heads % kv_heads != 0, kv_heads*k or kv_heads*dv beyond int, ldk < kv_heads*k,
 *     ldv < kv_heads*dv: SPMV_HIP_E_ARG before the handle's state is looked at, O untouched.  Handle kinds and SPMV_HIP_E_NOSTATE as there. */
int spmv_hip_attention_gqa(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                           const void *Matrix_Val, int heads, int kv_heads, int k, int dv, double scale,
                           const void *Q, long long ldq,            /* m x heads*k */
                           const void *K, long long ldk,            /* n x kv_heads*k */
                           const void *V, long long ldv,            /* n x kv_heads*dv */
                           const void *B, long long ldb,            /* `heads` bias planes, one shared plane, or NULL */
                           void *O, long long ldo);                 /* m x heads*dv */

/* ---- the gradients of spmv_hip_attention_gqa: dQ, dK, dV and dB -----------------------------------------------
 * spmv_hip_attention_bias_backward with the layout above: G, dQ `heads` blocks wide, dK n x kv_heads*k, dV n x kv_heads*dv, dB `heads` planes.
 * Let dK(h), dV(h) be what the single-head backward writes for query head h on Q + h*k, K + (h/gs)*k, V + (h/gs)*dv, G + h*dv and plane h of B.
 *   - dQ and dB: head h's bits of that single-head call.
 *   - dK and dV of K / V head g: (((dK(g*gs) + dK(g*gs+1)) + ...) + dK(g*gs+gs-1)), and the same for dV -- plain additions in the handle's
 *     precision in ascending query head, the first term taken as it is (not added to a zero), nothing contracted; gs == 1: no addition at all,
 *     and the call IS spmv_hip_attention_bias_backward to the bit.  A caller restates it with the single-head call per head and that loop.
 *   - No head-wide dK or dV ever exists in memory: the sums are held in registers by the column pass, or in the output element itself, read and
 *     written by one thread.  The handle's P and dS planes stay per QUERY head; device_bytes is spmv_hip_attention_heads_backward's for `heads`.
 *   - Option "attention_backward_heads" changes no bit: a round may end inside a group, and the next round's column pass then continues the
 *     chain from the dK / dV it finds (the thread that stores an element reads back its own earlier store; one stream, in order).  The
 *     default number of heads per round is a multiple of gs whenever it is at least gs, so the default path never reads back.
 *   - Which outputs are wanted, pointer kinds, leading dimensions, alignment, method, stream and async change no bit; only dB wanted runs
 *     no column pass and needs no transpose.  Special values stay in their query head in dQ and dB and reach, in dK and dV, the K / V head
 *     of their group and no other.  Empty rows and columns, nnz == 0, m == 0: spmv_hip_attention_heads_backward's rules at these widths (+0).
 *   - Errors: spmv_hip_attention_bias_backward's, and those of spmv_hip_attention_gqa with lddk < kv_heads*k, lddv < kv_heads*dv for WANTED
 *     outputs: SPMV_HIP_E_ARG before the handle's state is looked at, every output untouched. */
int spmv_hip_attention_gqa_backward(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                                    const void *Matrix_Val, int heads, int kv_heads, int k, int dv, double scale,
                                    const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                                    const void *B, long long ldb,            /* bias planes, or NULL */
                                    const void *G, long long ldg,            /* dL/dO, m x heads*dv */
                                    void *dQ, long long lddq,                /* m x heads*k,     or NULL: not wanted */
                                    void *dK, long long lddk,                /* n x kv_heads*k,  or NULL */
                                    void *dV, long long lddv,                /* n x kv_heads*dv, or NULL */
                                    void *dB, long long lddb);               /* heads planes of nnz, or NULL */

/* ---- the row log-sum-exp out of the forward: attention over a key / value set behind SEVERAL handles ------------------------
 * spmv_hip_attention_gqa with one more output: L holds `heads` planes, L[h*ldl + i] = M_i + log(Z_i) of query head h on row i, ldl >= m, in the
 * handle's precision, host or device pointer.  With L, partial results over disjoint parts of a key / value set (a local-window handle plus a
 * global-token handle, a context cut into key blocks, a pattern too large for one int CSR, a cache that grows between calls) are merged by
 * spmv_hip_attention_merge, and the gradients of each part come from spmv_hip_attention_gqa_backward_lse.
 *   - M_i and Z_i are EXACTLY the values the row softmax of step 3 computes, in its order; log / logf is the device math library's (not a fast
 *     intrinsic) and the addition is one plain addition; nothing is contracted.  O has exactly the bits spmv_hip_attention_gqa writes.
 *   - A row without entries: L = -inf (its O row is +0 as before).  A row that is NaN in O (a NaN or +inf in its scores, all scores -inf) is NaN in
 *     L, for that head and row only.
 *   - L == NULL: ldl is ignored and the call IS spmv_hip_attention_gqa, to the bit and to the launch.
 *   - Writes: exactly the first m elements of each of the `heads` planes; the padding between planes is never read or written.  nnz == 0
 *     writes the -inf values; m == 0 writes nothing.
 *   - L is a function of the matrix, k, the value type, the inputs and B alone: not of leading dimensions, alignment, access width, pointer kind,
 *     method, stream or async.  Head h of an H-head call has the bits of the one-head call on its slices.
 *   - Memory: a host L is staged through one more handle-owned buffer (counted in spmv_hip_info.device_bytes, freed with the others); with device
 *     operands device_bytes is spmv_hip_attention_gqa's.
 *   - Errors: spmv_hip_attention_gqa's, and L != NULL with ldl < m with them (SPMV_HIP_E_ARG before the handle's state is looked at, O and L
 *     untouched).  Handle kinds and SPMV_HIP_E_NOSTATE as there. */
int spmv_hip_attention_gqa_lse(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                               const void *Matrix_Val, int heads, int kv_heads, int k, int dv, double scale,
                               const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                               const void *B, long long ldb,            /* `heads` bias planes, one shared plane, or NULL */
                               void *O, long long ldo,                  /* m x heads*dv */
                               void *L, long long ldl);                 /* heads planes of m, or NULL: spmv_hip_attention_gqa */

/* ---- two partial attention results combined by their log-sum-exps ---------------------------------------
 * m is the handle's; the matrix is NOT read (the handle gives m, the precision, the stream and async setting, the pointer rule and the staging).
 * O1, O2 and O are m x heads*dv, L1, L2 and L `heads` planes of m.  Per row i and head h, in the handle's precision, nothing contracted but the
 * one fma written here, exp and log the device library's:
 *     Lm  = max(L1, L2)                      (fmax: drops a NaN; the exp restores it)
 *     w1  = exp(L1 - Lm),  w2 = exp(L2 - Lm),  W = w1 + w2
 *     O_c = fma(w2, O2_c, w1 * O1_c) / W,   c < dv
 *     L   = Lm + log(W)
 *   - Lm == -inf (both parts empty on that row): O = +0 and L = -inf.  A part that is empty on a row (L = -inf, O = 0) leaves the other part's
 *     O values and L bits.  A NaN in either L makes that head's row NaN in O and L, and no other.
 *   - O may be the very pointer O1 and L the very pointer L1: a running accumulator that parts are folded into from left to right (every element
 *     is read and written by the same thread).  Any other overlap is undefined.  L == NULL: the merged log-sum-exp is not wanted.
 *   - One grid-stride launch, bandwidth-bound; 16-byte accesses when O1, O2 and O allow them (and dv is a multiple of 16 bytes when heads > 1);
 *     the width, the pointer kinds and the leading dimensions change no bit.  Exactly m x heads*dv elements of O and m per plane of L are written.
 *   - Memory: host operands go through six more handle-owned buffers (counted in device_bytes, freed with the others); device operands: nothing.
 *   - Errors (SPMV_HIP_E_ARG before the handle's state is looked at, outputs untouched): a NULL handle; heads or dv < 1; heads*dv beyond int; ldo1,
 *     ldo2 or ldo < heads*dv; a negative ldl*.  Once m is known (outputs untouched): ldl1, ldl2 or (with an L) ldl < m; a NULL O1, L1, O2, L2 or O
 *     while m > 0.  Multi-GPU, host_rows and "reorder" handles: SPMV_HIP_E_ARG.  A cleared or failed handle: SPMV_HIP_E_NOSTATE. */
int spmv_hip_attention_merge(spmv_Handle_t handle, int heads, int dv,
                             const void *O1, long long ldo1, const void *L1, long long ldl1,
                             const void *O2, long long ldo2, const void *L2, long long ldl2,
                             void *O, long long ldo,                    /* m x heads*dv; may be O1 */
                             void *L, long long ldl);                   /* heads planes of m; may be L1; or NULL */

/* ---- the gradients of one part, driven by the FINAL output and log-sum-exp ----------------------------------
 * spmv_hip_attention_gqa_backward with four more inputs: O (m x heads*dv, ldo) and L (`heads` planes of m, ldl >= m) hold the final output and
 * log-sum-exp of the attention this handle's entries are a part of -- for a single handle its own spmv_hip_attention_gqa_lse results, for parts
 * the merged ones.  The steps that differ:
 *     t_p as in the forward, bias included;   P_p = exp(t_p - L_i)   -- one subtraction and one exp: no maximum, no sum, no division --
 *     D_i = <G[i, h*dv .. +dv), O[i, h*dv .. +dv)>   in spmv_hip_sddmm's order for dv columns, once per row and head;
 * dP_p, dB_p = P_p * (dP_p - D_i), dS_p = dB_p * scale, dQ, dK, dV and the group sums of dK / dV are exactly spmv_hip_attention_gqa_backward's,
 * and so are the NULL-output rules, "only dB wanted runs no column pass", option "attention_backward_heads" changing no bit, and the column
 * pass with its transpose.  The parts' dQ are the caller's to add; dK, dV and dB are each part's own.
 *   - A row whose L_i is NaN gives NaN in its head's dQ row and dB entries and in the dK / dV rows it reaches (the K / V head of its group only).
 *   - An L inconsistent with the scores (smaller than the row's true log-sum-exp) gives meaningless values, never a fault.
 *   - Memory: a host O / L is staged through two more handle-owned buffers; with device operands device_bytes is spmv_hip_attention_gqa_backward's.
 *   - Errors: spmv_hip_attention_gqa_backward's, and ldo < heads*dv, ldl < m, a NULL O or L while m > 0 with them (SPMV_HIP_E_ARG before the
 *     handle's state is looked at, every output untouched). */
int spmv_hip_attention_gqa_backward_lse(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                                        const void *Matrix_Val, int heads, int kv_heads, int k, int dv, double scale,
                                        const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                                        const void *B, long long ldb,            /* bias planes, or NULL */
                                        const void *G, long long ldg,            /* dL/dO, m x heads*dv */
                                        const void *O, long long ldo,            /* the final output, m x heads*dv */
                                        const void *L, long long ldl,            /* the final log-sum-exp, heads planes of m */
                                        void *dQ, long long lddq,                /* m x heads*k,     or NULL: not wanted */
                                        void *dK, long long lddk,                /* n x kv_heads*k,  or NULL */
                                        void *dV, long long lddv,                /* n x kv_heads*dv, or NULL */
                                        void *dB, long long lddb);               /* heads planes of nnz, or NULL */

/* ---- the forward on 16-bit Q, K and V (fp16 / bf16), with O in that type or in fp32 ------------------------------------------
 * spmv_hip_attention_gqa_lse for callers that keep Q, K and V in a 16-bit type: the kernels load the 16-bit elements, widen them in registers and
 * run the fp32 arithmetic unchanged, so nothing is widened in memory and the gathers of K and V rows move two bytes per element.
 *   - Handle and types: the handle is an fp32 handle (data_size == 4; an fp64 handle: SPMV_HIP_E_ARG).  io_type is SPMV_HIP_T_F16 (IEEE binary16) or
 *     SPMV_HIP_T_BF16, the element type of Q, K and V; o_type is SPMV_HIP_T_HANDLE (O is fp32) or equal to io_type (O in that type); anything else is
 *     SPMV_HIP_E_ARG.  Leading dimensions count elements of the operand's own type: ldq, ldk and ldv 16-bit elements, ldo elements of O's type.  B and L
 *     are fp32, exactly as in spmv_hip_attention_gqa_lse (ldb == 0: one shared plane; B == NULL: no bias; L == NULL: no L is stored).
 *   - Bits, o_type == SPMV_HIP_T_HANDLE: O and L have exactly the bits spmv_hip_attention_gqa_lse writes when called with Q, K and V converted
 *     element by element to fp32.  That conversion is exact -- fp16 subnormals keep their values, infinities and NaN stay what they are --, and the
 *     lane mapping is the fp32 kernels' (4 columns per lane), so everything promised there holds unchanged: the order, the special values, head h
 *     equal to the one-head call on its slices, and invariance under leading dimensions, alignment, access width, pointer kind, method, stream
 *     and async.
 *   - Bits, o_type == io_type: each element of O is that fp32 value rounded ONCE to the 16-bit type, to nearest, ties to even: fp16 overflow gives
 *     +-inf, NaN stays NaN, the sign of zero is kept, small results become subnormals (what torch.Tensor.to(dtype) does to the fp32 result).  Rows
 *     without entries get +0.  L has the same bits in both modes.
 *   - Access width: a lane's segment of 4 columns is 8 bytes of a 16-bit operand; 8-byte accesses are used when pointer and ld * 2 are multiples
 *     of 8 for Q, K, V and a 16-bit O (16 for an fp32 O), and with heads > 1 also k * 2 and dv * 2; 2-byte accesses otherwise.  The width changes no bit.
 *   - Writes: exactly heads*dv elements of each of the m rows of O, in O's type, and exactly m elements per plane of L; padding is never read or
 *     written.  m == 0 writes nothing.
 *   - Memory: host or device pointers per operand.  A host Q, K, V or 16-bit O is staged through the handle-owned buffers of
 *     spmv_hip_attention_gqa_lse at two bytes per element; with device operands device_bytes is spmv_hip_attention_gqa_lse's.
 *   - Errors: the type rules above and every argument rule of spmv_hip_attention_gqa_lse are SPMV_HIP_E_ARG before the handle's state is looked at,
 *     every output untouched.  Handle kinds and SPMV_HIP_E_NOSTATE as there.  The gradients are spmv_hip_attention_gqa_backward's on fp32 copies. */
enum { SPMV_HIP_T_HANDLE = 0, SPMV_HIP_T_F16 = 1, SPMV_HIP_T_BF16 = 2 };

int spmv_hip_attention_gqa_lse_16(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                                  const void *Matrix_Val, int heads, int kv_heads, int k, int dv, double scale,
                                  int io_type,                             /* SPMV_HIP_T_F16 or SPMV_HIP_T_BF16: the element type of Q, K and V */
                                  const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                                  const void *B, long long ldb,            /* bias planes in the HANDLE's precision (fp32), one shared plane, or NULL */
                                  void *O, long long ldo, int o_type,      /* SPMV_HIP_T_HANDLE: fp32 O; or == io_type: O in that 16-bit type */
                                  void *L, long long ldl);                 /* fp32 planes, or NULL */

/* ---- the backward on 16-bit Q, K, V and G (fp16 / bf16), each gradient in that type or in fp32 ------------------------------
 * spmv_hip_attention_gqa_backward and spmv_hip_attention_gqa_backward_lse for callers that keep Q, K, V and dL/dO in a 16-bit type: the four
 * kernels load the 16-bit elements, widen them in registers and run the fp32 arithmetic unchanged; nothing is widened in memory, and a 16-bit
 * gradient is stored already rounded.
 *   - Handle and types: an fp32 handle (an fp64 handle: SPMV_HIP_E_ARG).  io_type is SPMV_HIP_T_F16 or SPMV_HIP_T_BF16, the element type of Q, K, V
 *     and G.  dq_type is the type of dQ and dkv_type that of dK and dV: SPMV_HIP_T_HANDLE (fp32) or equal to io_type; anything else is
 *     SPMV_HIP_E_ARG.  B, dB, O and L are fp32, exactly as in the fp32 calls.  Leading dimensions count elements of the operand's own type.
 *   - O and L: both NULL -- the self-normalising row pass of spmv_hip_attention_gqa_backward; both given -- the row pass of
 *     spmv_hip_attention_gqa_backward_lse, driven by them.  Exactly one of them NULL while m > 0: SPMV_HIP_E_ARG.
 *   - Bits, fp32 outputs and dB: exactly those of spmv_hip_attention_gqa_backward (O = L = NULL) or spmv_hip_attention_gqa_backward_lse (O and L
 *     given) on Q, K, V and G converted element by element to fp32.  The conversion is exact and the lane mapping is the fp32 kernels' (4 columns
 *     per lane), so everything promised there carries over: the order, the group sums of dK / dV in ascending head, the special values, head h
 *     equal to the one-head call on its slices.
 *   - Bits, 16-bit outputs: each element is that fp32 value rounded ONCE, to nearest, ties to even (what fp32_gradient.to(dtype) gives in torch):
 *     fp16 overflow gives +-inf -- reachable here: a dV element is a sum over a column --, NaN stays NaN, the sign of zero is kept.  No 16-bit
 *     element is ever read back as a partial sum: with kv_heads < heads a 16-bit dK / dV is summed over its group's heads in two handle-owned
 *     fp32 arrays (n x kv_heads*k and n x kv_heads*dv, counted in device_bytes, freed with the handle) and rounded by one bandwidth-bound launch
 *     at the end of the call, whatever the rounds and however long the columns.
 *   - These change no bit: access width (8-byte accesses to a 16-bit operand and 16-byte ones to an fp32 operand when pointer and ld allow them
 *     for every operand and, with heads > 1, k and dv are multiples of 4; element accesses otherwise), leading dimensions, alignment, pointer
 *     kind, method, stream, async and option "attention_backward_heads".  The two output types are independent: the row kernels see only dQ's,
 *     the column kernels only dK's and dV's.
 *   - Memory: host or device pointers per operand; a host operand is staged through the buffers of the fp32 calls at its own element size.
 *   - Errors: the rules above and every argument rule of spmv_hip_attention_gqa_backward(_lse) are SPMV_HIP_E_ARG before the handle's state is
 *     looked at, every output untouched; the NULL-output rules (nothing wanted: no work; only dB wanted: no column pass, no transpose), the
 *     handle kinds and SPMV_HIP_E_NOSTATE are those calls'. */
int spmv_hip_attention_gqa_backward_16(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                                       const void *Matrix_Val, int heads, int kv_heads, int k, int dv, double scale,
                                       int io_type,                             /* SPMV_HIP_T_F16 or SPMV_HIP_T_BF16: the element type of Q, K, V and G */
                                       const void *Q, long long ldq, const void *K, long long ldk, const void *V, long long ldv,
                                       const void *B, long long ldb,            /* fp32 bias planes, or NULL */
                                       const void *G, long long ldg,            /* dL/dO, m x heads*dv */
                                       const void *O, long long ldo,            /* fp32; O and L both NULL: the self-normalising row pass */
                                       const void *L, long long ldl,            /* fp32; both given: driven by the final output and log-sum-exp */
                                       int dq_type, void *dQ, long long lddq,   /* SPMV_HIP_T_HANDLE (fp32) or == io_type; dQ NULL: not wanted */
                                       int dkv_type, void *dK, long long lddk,  /* the type of dK and dV; n x kv_heads*k, or NULL */
                                       void *dV, long long lddv,                /* n x kv_heads*dv, or NULL */
                                       void *dB, long long lddb);               /* fp32, heads planes of nnz, or NULL */

/* ---- options --------------------------------------------------------------------------------
 * Resolved once per handle, at create: process-wide value (spmv_hip_set_option / env), overridden by the
 * calling thread's value (spmv_hip_set_thread_option) -- so two threads can create differently tuned handles
 * without racing -- and stored in the handle (spmv_hip_get_handle_option). */
/* keys: "lanes_per_row" (CSR-vector, 0 = auto, else 1..64 power of two)
 *       "sell_c" (64)  "sell_sigma" (1024)  "sell_lds_x" (0/1: stage narrow x windows in LDS)
 *       "sell_long_thr" (rows longer than this stay out of the slabs; 0 = from the row-length histogram: length classes with
 *                        less than a chunk's worth of rows per sigma window leave, at most max(64, 8 x mean row length) stays)
 *       "csr5_sigma" (0 = auto)  "rowblock_nnz" (equal-nnz share of one Balanced row block, 0 = auto = 8192)
 *       executor-form selectors (what create() otherwise chooses by rule or by timing; tests force every form through them):
 *       "vector_form" (CSR-vector: 0 timed at create, 4 pipe, 5 / 12 tile two deep, 10 / 11 tile four deep, 6 tile eight deep)
 *       "x_windows" (0/1, default 1: stage the tile groups' x windows in LDS)   "xcd_order" (0/1, default 1)   "csr5_two_deep" (0 auto / 1 never / 2 always)
 *       "run_tiles" (0/1, default 1: RUN / BYTE tiles -- spmv_hip_info.run_nnz, byte_nnz)
 *       "row_forward" (0/1, default 1: nnz-split tiles that gather through L2 finish the rows they start -- one launch, no carry fix-up; spmv_hip_info.launch_kernels)
 *       "pack_values" (0/1/2, default 2: fp64 CSR-vector tiles whose values are all k * 2^e -- one e per 256-row tile, integers |k| < 2^55, finite, no -0.0 --
 *                      and whose rows are whole aligned blocks of 4 x lanes_per_row entries read their values as 7 bytes instead of 8, from two planes
 *                      the library keeps beside the value array (7 B per non-zero more in device_bytes), decoded exactly: y is bit-identical.  Integer,
 *                      0/1, quantised or short-mantissa values qualify, e.g. uniform random doubles in [-1, 1); a tile that does not keeps its 8-byte
 *                      stream, in the same launch; spmv_hip_update_values gates and packs again.  0: never.  1: every qualifying tile, untimed (tests,
 *                      A/B).  2: only where create() times the tile forms (nnz >= 2^24, nothing forced) and at least half of the tiles qualify; the
 *                      packed kernel is timed next to the plain winner and kept only below 0.95 x its time, else the planes are freed --
 *                      spmv_hip_info.packed_nnz, pack_ms)
 *       "autotune" (0/1, default 1: for matrices above 2^24 nnz create() times the applicable CSR-vector
 *                   kernel forms once on the resident matrix and keeps the fastest, ~10 ms)
 *       "reorder" (0/1/2, default 0; 1: reverse Cuthill-McKee on the device (kernels/rcm.hpp), 2: the host BFS of round 1.  For matrices whose band was lost to
                  a bad numbering; NOT for power-law matrices: the blocked executor is indifferent to vertex numbers and RCM scatters the hubs (measured
                  slower, profiles/r04_reorder.txt).  Square matrices are reordered at create, B = P A P^T is what stays
 *                  resident, and handle->index holds the permutation -- the caller gathers
 *                  XX[i] = X[index[i]] and scatters Y[index[i]] = YY[i] exactly as the reference's harness
 *                  does for its OPT_LEVEL 3 path, test_spmv.c:95-101, 130-137)
 *       "auto_method" (0/1/2; 2 = like 1, then every candidate schedule is built and timed on scratch vectors at
 *                      create and the fastest kept, +0.1..0.3 s for 3e8 nnz.  1: create() replaces the requested method by the one its row statistics
 *                      favour -- CSR-vector for regular rows, CSR5 otherwise -- and, if that schedule cannot
 *                      stage a single x window on a matrix whose x is far larger than an L2, by
 *                      Method_Balanced_Yid with the cache-blocked executor; the handle reports it)
 *       "cache_block" (0 never / 1 automatic (default) / 2 always: every schedule but the debug kernel CSR-scalar hands the
 *                      multiply to the row-block x column-slab executor when no x window of the matrix fits LDS,
 *                      nnz >= 2^21 and n * size >= 4 MiB (x as large as an XCD's L2; 12 MiB when rows average fewer than 8 entries): ~3x faster on columns
 *                      without locality.  A row block's products are added in an order fixed by the matrix -- one wavefront per block, or the waves
 *                      of the wide form taking turns --, so results are bit-reproducible unless option "deterministic" = 0 waives that.)
 *       "split" (0/1, default 1: a matrix whose entries are partly local, partly scattered may be multiplied as A_near + A_far when
 *               create() measures that faster -- spmv_hip_info.split_ms, far_nnz)
 *       "slab_kib" (KiB of x per column slab, 0 = as narrow as the cell table allows)
 *       "block_rows" (uniform row blocks of that many rows, at most 16384; 0 = equal-work blocks sized by the executor form: up to 9982 rows with a wave per
                     block, up to 20350 in the wide forms)
       "blk_waves" (0 automatic / 1 / 2 / 4 / 8: wavefronts sharing ONE row block's LDS accumulators; 0: create() builds the one-wave form and, on large
                    matrices, the wide form that fits option "deterministic", times them and keeps the faster)
       "blk_groups" (groups of 128 fp64 / 256 fp32 entries per pipeline step, 0 = timed at create)   "blk_subsort" (0/1, default 1)
       "keep_columns" (0/1, default 0: at the end of create() the HBM-resident int32 ColIdx copy is released when the built schedule's multiply never reads it --
                       every tile / group staged, SELL slabs, CSR5 tiles -- 4 B per non-zero less (spmv_hip_info.device_bytes); 1 keeps it)
       "deterministic" (0/1, default 1: every executor adds a row's products in an order fixed by the matrix, so results are bit-identical run to
                        run; 0 lets the wide blocked form add in arrival order -- 10-16 % faster on matrices without column locality, equal to rounding)
 *       "attention_backward_heads" (0..1024, default 0: heads per round of spmv_hip_attention_heads_backward, i.e. planes of the two handle-owned
 *                      arrays; 0 = as many as fit 2*HG*s*nnz bytes into an eighth of the device's memory.  Changes memory and the number of
 *                      rounds, never a bit)
 *       "host_rows" (0/1, default 0: 1 = handles created with VECTOR_NONE and Method_Serial / Method_Parallel run
 *                    a plain-C row loop on the HOST over the caller's arrays (BASELINE config 1: the reference's
 *                    plumbing case); never selected automatically -- without it a missing GPU is an error)
 *       "check_values" (0/1/2, default 2: spmv() watches Matrix_Val for in-place changes and refreshes the resident copies by itself.  2: HOST arrays
                       only, by a SAMPLED checksum (every 64th word, at most 65536, and both ends: sees any update of the whole array, misses most
                       single-entry edits; under a millisecond per call); 1: the full position-weighted checksum on every call, host or device array
                       (reads the values once more per call); 0: never.  Works on multi-GPU handles (option "gpus") too.)
 *       "gpus" (0 = this handle lives on the current device; G > 0: row blocks over min(G, visible devices) GPUs
 *               of this process, see "multi-GPU" below)   "x_exchange" (multi-GPU: 0 allgather, 1 range, 2 broadcast)
 * Each key can also be preset with the environment variable SPMV_HIP_<KEY IN CAPS>.
 * Returns 0, or SPMV_HIP_E_ARG for an unknown key / illegal value. */
int spmv_hip_set_option(const char *key, long value);
long spmv_hip_get_option(const char *key);            /* the value a create() on this thread would use */
int spmv_hip_set_thread_option(const char *key, long value); /* override for handles created by the calling thread */
void spmv_hip_clear_thread_options(void);
long spmv_hip_get_handle_option(spmv_Handle_t handle, const char *key); /* what the handle was created with; -1 unknown */

/* ---- introspection ------------------------------------------------------------------------ */
typedef struct spmv_hip_info {
    int device;                 /* HIP device ordinal the handle lives on */
    int schedule;               /* 0 csr-scalar 1 csr-vector 2 row-block 3 nnz-split 4 sell-c-sigma 5 csr5 */
    int lanes_per_row;          /* csr-vector */
    int sell_c, sell_sigma;     /* sell */
    int tile_nnz;               /* nnz-split / csr5 tile size */
    int m, n;
    long long nnz;
    long long stored_nnz;       /* incl. SELL padding */
    int max_row_len, min_row_len, empty_rows;
    double mean_row_len;
    long long device_bytes;     /* HBM held by the handle */
    long long alg_bytes;        /* B_alg = 4(m+1) + nnz(4+s) + s*n + s*m    */
    double inspect_ms;          /* wall time of the inspector inside create */
    const char *schedule_name;
    const char *kernel_name;    /* symbol of the dominant kernel (as rocprofv3 shows it) */
    int tuned_choice;           /* csr-vector autotune: 0 none, 10/11 tile 4-deep, 5/12 tile 2-deep, 4 pipe (row-block schedule and csr-vector's wide form: 10 / 5 = the rows
                                   kernel four / two steps deep); cache_blocked: 100 / 101 =
                                   the smaller / larger groups-per-pipeline-step form (8 / 12; 6 / 8 with blk_waves = 8) */
    float tune_ms[3];           /* measured ms of {tile/4-deep, tile/2-deep, pipe} at create (0 if not tuned; pipe: 0 when 99 % of the tiles stage their x windows -- not timed); cache_blocked: of the
                                   row-block executor's two groups-per-step forms ([2] unused) */
    int x_groups;               /* tiles / tile groups / sigma windows the inspector analysed for x windows */
    int x_groups_staged;        /* ... of which have their x windows staged in LDS (0: every gather goes to L1/L2) */
    int cache_blocked;          /* 1: the row-block x column-slab executor runs (option "cache_block") */
    long long stream_bytes;     /* HBM bytes ONE spmv() has to move given the schedule's storage format: the value and
                                 * column streams as stored (2 B/nnz LDS slots where x windows are staged -- none for run_nnz --, padding
                                 * included), row pointers / descriptors / window tables, the x elements staged (at most
                                 * 8 n: one pass per XCD; or n once where x is gathered through L2), y written once, carries.  This -- not alg_bytes --
                                 * is what divides by the launch time to give the HBM rate actually sustained. */
    long long x_bytes;          /* the part of stream_bytes charged for reading x */
    float route_ms[2];          /* only when part of the tile groups stage their x windows and part do not: create() builds the tile
                                 * schedule AND the row-block x column-slab executor, times both -- [0] tile schedule, [1] blocked
                                 * executor, ms -- and keeps the faster (0, 0: the choice needed no measurement) */
    float split_ms[2];          /* when a sizeable part of the entries -- not all -- lies near its tile's centre column, create() also builds
                                 * A = A_near + A_far (near: the tile schedule, every tile staged; far: the blocked executor, accumulating) and
                                 * times it: [0] schedule as built, [1] the split pair, ms (0, 0: not tried) */
    long long far_nnz;          /* entries the blocked executor multiplies in a split handle (0: the handle is not split) */
    long long run_nnz;          /* CSR-vector / row-block tile kernels, SELL slabs, CSR5 tile groups: entries in RUN tiles / groups -- staged ones whose rows
                                 * each reference one run of consecutive columns (banded matrices; CSR5: of at least sigma entries); their column stream is
                                 * not read at all (16 bits, SELL: a word, per ROW; CSR5: a word per lane and tile instead) */
    long long byte_nnz;         /* CSR-vector / row-block tile kernels, SELL window groups: entries in BYTE tiles / groups -- staged ones in which every row's LDS slots lie
                                 * within 255 of the row's smallest (SELL: first) slot (banded matrices with holes, block rows): their column stream is one byte per entry
                                 * + 16 bits (SELL: a word) per row */
    long long tmpl_nnz;         /* ... entries in TEMPLATE tiles -- staged tiles whose rows all have the same slot offsets from their first entry (stencil interiors,
                                 * block rows): no column stream either, 16 bits per row + one offset list per tile */
    int blk_waves;              /* cache_blocked: wavefronts that share one row block's accumulators (1: a wave per block, two blocks per CU; 2 / 4 / 8: the
                                 * wide form, one block of up to ~20 k rows per CU); 0 when another executor runs */
    char launch_kernels[160];   /* every kernel ONE spmv() launches, in order, '+'-separated (e.g. "sell_window_kernel+csr5_group_pipe_kernel+csr5_fixup_kernel") */
    int reproducible;           /* 1: the executor adds every row's products in an order fixed by the matrix -- identical bits run to run and handle to
                                 * handle; 0 only for the wide blocked form under option "deterministic" = 0 */
    int x_span_max;             /* elements of the largest x window set the dominant kernel stages for one tile / group (the single window's span, or the
                                 * sum of the windows of a tile covered by several); 0 when it stages nothing (global-column kernels, cache_blocked) */
    int lds_bytes;              /* dynamic LDS, in bytes, the dominant kernel's launch requests: (x_span_max + 1 zero slot) elements in whole KiB, plus SELL's
                                 * row sums of one window group, plus the CSR5 / nnz-split waves' row maps (matrices with empty rows); cache_blocked: one row
                                 * block's accumulators.  The kernels' static LDS is not included */
    long long packed_nnz;       /* CSR-vector tile kernel, fp64: entries in PACKED tiles -- tiles whose values are all k * 2^e with one exponent e per tile and
                                 * integers |k| < 2^55, finite, no -0.0, every row a whole number of aligned 4L-entry blocks: their values are streamed as
                                 * 7 bytes (32 low bits + 24 high bits of k) from planes kept beside the value array and decoded exactly -- the same bits
                                 * in y as from the 8-byte stream.  0 when the planes are not in use (option "pack_values") */
    float pack_ms[2];           /* option pack_values = 2 where create() timed it: [0] the best plain tile form, [1] the best packed form (four or two steps
                                 * in flight), ms; the packed form stays only below 0.95 x [0].  0, 0: not timed */
} spmv_hip_info;
int spmv_hip_get_info(spmv_Handle_t handle, spmv_hip_info *out);
/* the transposed schedule's spmv_hip_info (m, n swapped; schedule, kernels, device_bytes of A^T alone, reproducible); SPMV_HIP_E_NOSTATE until built */
int spmv_hip_get_transpose_info(spmv_Handle_t handle, spmv_hip_info *out);

/* ---- multi-GPU: row blocks over the GPUs of ONE process (option "gpus"; BASELINE config 5) --------------
 * A handle created while option "gpus" = G > 0 splits the matrix into min(G, visible devices) equal-nnz row blocks, one
 * per device, each with its own schedule, stream, full-length x buffer and y block (the GPU analogue of the reference's
 * NUMA experiment, src/samples/numa.c:277-304).  spmv() keeps its signature and meaning: X and Y are FULL vectors (host
 * or device pointers); per call X is distributed (option "x_exchange": 0 = every device receives its slice and the
 * slices are all-gathered over xGMI with RCCL, 2 = X goes to device 0 and is broadcast -- north_star's literal form,
 * 1 = "range": every device receives only the columns its row block references, x[min ColIdx .. max ColIdx] -- for a
 * banded matrix its own slice and a few values either side; in the distributed step they are pulled from the
 * neighbouring devices by peer copies, no collective),
 * every device multiplies its block, and the y blocks are collected into Y.
 * A solver loop keeps the vectors DISTRIBUTED instead: write this step's x into the devices' slices, call
 * spmv_hip_multi_step (exchange + multiply, nothing crosses PCIe), read y from the devices' blocks.
 * RCCL is dlopen'ed only when G > 1; without it the exchange uses peer-to-peer copies. */
int spmv_hip_multi_gpus(spmv_Handle_t handle);        /* devices the handle spans; 0 for an ordinary handle */
int spmv_hip_multi_uses_rccl(spmv_Handle_t handle);   /* 1: the x exchange runs through RCCL communicators */
/* Device `gpu`'s slice of x (x_count elements from global index x_first, device memory on *device, inside that device's
 * full-length copy) and its block of y (rows y_first ... y_first + y_count - 1).  Any out-pointer may be NULL. */
int spmv_hip_multi_slices(spmv_Handle_t handle, int gpu, void **x_slice, long long *x_first, long long *x_count,
                          void **y_block, long long *y_first, long long *y_count, int *device);
/* Exchange the x slices between the devices and multiply; y stays distributed.  Synchronous: every device is drained first
 * (hipDeviceSynchronize), so the x slices may have been written on any stream; returns when the y blocks are complete.
 * x_exchange = 1 ("range") runs the halo copies beside the multiply and redoes the rows that needed them. */
int spmv_hip_multi_step(spmv_Handle_t handle);
/* The same, enqueued only, ordered behind the work the caller has submitted to each device's DEFAULT stream (the x slices must have
 * been written there, or be complete); spmv_hip_multi_synchronize waits for every device (results in the y blocks).  Steps may be enqueued
 * back to back (a step's halo copies wait for the previous step's multiplies); the caller writes the NEXT x slices on the default
 * streams, which a step is ordered behind -- but nothing orders those writes behind a step still running: synchronize (or wait on
 * an event of your own) before overwriting x slices a running step reads. */
int spmv_hip_multi_step_async(spmv_Handle_t handle);
int spmv_hip_multi_synchronize(spmv_Handle_t handle);
/* A multi-GPU handle from row blocks that exist separately -- the way the reference's NUMA experiment hands each memory node
 * its rows (src/samples/numa.c:277-304).  Block g: rows[g] rows, LOCAL 0-based int32 RowPtr[g] (rows[g] + 1 entries), GLOBAL
 * column indices ColIdx[g] in [0, n), values Matrix_Val[g]; host or device pointers; block g is placed on device g (at most
 * as many blocks as visible devices).  No monolithic array exists, so the int32 limit of RowPtr applies per block: BASELINE
 * config 5 (8 x 1e7 rows x 32 = 2.56e9 non-zeros) is created this way.  Options (x_exchange, ...) are read as at any create.
 * spmv() on the handle takes full-length X (n) / Y (sum of rows) and ignores its CSR arguments; spmv_hip_multi_slices /
 * _step work as for option "gpus"; spmv_hip_update_values is not available (clear and create again). */
void spmv_hip_create_handle_from_blocks(spmv_Handle_t *Handle, int blocks, const BASIC_INT_TYPE *rows, BASIC_INT_TYPE n,
                                        BASIC_INT_TYPE *const *RowPtr, BASIC_INT_TYPE *const *ColIdx, void *const *Matrix_Val,
                                        SPMV_METHODS Function, BASIC_SIZE_TYPE size);

/* ---- conjugate gradients on the device: A x = b ------------------------------------------------
 * Preconditioned conjugate gradients for a SYMMETRIC POSITIVE DEFINITE A (m = n) in the standard two-dot form, with an optional diagonal
 * (Jacobi) preconditioner: per iteration the handle's own multiply q = A p -- spmv()'s schedule and bits -- and three vector kernels.  alpha,
 * beta and the stop test are formed on the device; the host enqueues check_every iterations, then looks at a small state word once.
 *   - Returns SPMV_HIP_OK whenever the solve RAN: not converging is a `status`, not an error.  The call is synchronous: it returns with X
 *     complete, on the handle's stream, whatever spmv_hip_set_async says.
 *   - The CSR arguments follow spmv()'s rules: m and the pointers seen at create -> the resident matrix; others -> that matrix is
 *     re-inspected; option "check_values", in-place value changes and spmv_hip_update_values apply as for spmv().
 *   - B, X and Dinv: m elements of the handle's type each, host or device pointers (host ones are staged through handle-owned HBM buffers);
 *     B and X must not overlap.  use_x0 = 0: the solve starts from x = 0 and X is only written; otherwise X holds the initial guess.
 *   - Stop: rr <= max(rtol^2 * bb, atol^2), with rr = <r,r> of the recurrence's residual and bb = <b,b>, both in fp64; rtol = atol = 0
 *     runs max_iterations iterations (unless rr reaches 0).  m = 0: converged, 0 iterations.  bb = 0: X is set to zeros, converged, 0 iterations.
 *   - status: SPMV_HIP_CG_CONVERGED; _MAX_ITERATIONS; _BREAKDOWN: <p,Ap> <= 0 or <r,z> <= 0 while rr > 0 -- A or Dinv is not positive
 *     definite; X is the last iterate before it; _NONFINITE: a NaN or infinity in <b,b>, <r,r>, <r,z>, <p,Ap>, alpha or beta.  `iterations`
 *     counts the updates of x that were applied, rr and bb belong to the returned X.  history (a HOST array of max_iterations + 1 doubles, or
 *     NULL) receives rr after iteration 0 (the initial residual), 1, ..., iterations.
 *   - Workspace: r, p, q (m elements each), the partial sums and the state in one block -- and the history's device copy when one is
 *     wanted -- allocated at the first solve, freed at destroy / clear / re-inspection, counted in spmv_hip_info.device_bytes.
 *   - Option "reorder" handles solve with the resident P A P^T: the caller permutes B, X and Dinv by handle->index (XX[i] = X[index[i]]),
 *     as for spmv().
 *   - Errors (SPMV_HIP_E_ARG, X untouched): a matrix with m != n at create; NULL opt or res; NULL B or X when m > 0; max_iterations < 0,
 *     check_every < 0, a negative or NaN rtol or atol; multi-GPU handles (option "gpus", spmv_hip_create_handle_from_blocks); host_rows
 *     handles.  A cleared or failed handle: SPMV_HIP_E_NOSTATE.  Every failure is also reported through spmv_hip_last_error().
 *
 * The arithmetic contract -- bits, not a tolerance; tests/cg_cases.py restates it in numpy:
 *   Elements are of the handle's type T.  Every dot widens both elements to fp64, multiplies and adds in fp64, separately (no fma; for float
 *   the product of two widened elements is exact).  alpha = <r,z> / <p,q> and beta = <r,z>_new / <r,z>_old are formed in fp64 and rounded to T
 *   ONCE.  The vector updates are in T, a multiply and then an add, never an fma, in this order per iteration:
 *       x = x + alpha*p;  r = r - alpha*q;  z = Dinv*r (z = r without Dinv);  p = z + beta*p.
 *   At the start r = B (or r = B - A*x0), p = z.  The stop test reads the rr of the update just applied.
 *   Order of a dot over m elements: P = min(1024, ceil(m / 1024)) workgroups, L = 1024 * ceil(m / (1024 * P)); workgroup j owns elements
 *   [j*L, min(m, (j + 1)*L)).  Inside a workgroup the element at offset o goes to thread (o / 4) mod 256, slot o mod 4, step o / 1024; each
 *   (thread, slot) accumulator starts at +0.0 and adds its products by ascending step; absent elements add +0.0.  A thread's sum is
 *   (a0 + a1) + (a2 + a3); the 64 lanes of a wave are combined by the adjacent-pair binary tree; the four waves as (w0 + w1) + (w2 + w3).  For
 *   the final sum the P partials are padded with +0.0 to 1024, thread t takes partials 4t .. 4t + 3 as (a + b) + (c + d), then the same wave
 *   and workgroup trees.  The order depends on m alone: not on the value type, the alignment of a pointer, the access width, or whether a
 *   pointer is a host or a device one.
 *   Consequences: Dinv = all ones gives exactly the bits of Dinv = NULL; X, iterations, rr and history are bit-identical run to run and for
 *   every check_every (unless the handle was created with option "deterministic" = 0, whose spmv() is not reproducible either). */
enum { SPMV_HIP_CG_CONVERGED = 0, SPMV_HIP_CG_MAX_ITERATIONS = 1, SPMV_HIP_CG_BREAKDOWN = 2, SPMV_HIP_CG_NONFINITE = 3 };
typedef struct spmv_hip_cg_options {
    double rtol, atol;        /* stop when rr <= max(rtol^2 * bb, atol^2); rr = <r,r>, bb = <b,b>, both in fp64 */
    int max_iterations;       /* >= 0 */
    int check_every;          /* iterations enqueued between two looks at the device's state word; 0 = default */
    int use_x0;               /* 0: start from x = 0 (X is only written); != 0: X holds the initial guess */
    const void *Dinv;         /* NULL, or m elements of the handle's type (host or device): z = Dinv .* r (Jacobi: 1 / diag(A)) */
    double *history;          /* NULL, or HOST array of max_iterations + 1 doubles: rr after iteration 0, 1, ... */
} spmv_hip_cg_options;
typedef struct spmv_hip_cg_result {
    int status;               /* SPMV_HIP_CG_CONVERGED 0, _MAX_ITERATIONS 1, _BREAKDOWN 2, _NONFINITE 3 */
    int iterations;           /* updates of x that were applied */
    double rr, bb;            /* of the returned x (the recurrence's r) */
} spmv_hip_cg_result;
int spmv_hip_cg(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                const void *Matrix_Val, const void *B, void *X,
                const spmv_hip_cg_options *opt, spmv_hip_cg_result *res);

/* ---- BiCGStab on the device: A x = b for a matrix that need not be symmetric --------------------
 * Right-preconditioned BiCGStab for a square A (m = n) with an optional diagonal preconditioner: per iteration two of the handle's own
 * multiplies -- spmv()'s schedule and bits -- and five vector kernels.  alpha, omega, beta and the stop tests are formed on the device; the
 * host enqueues check_every iterations, then looks at a small state once.
 * The options, the result, the status values and EVERY rule of spmv_hip_cg above hold word for word: the return value, the synchronous call,
 * the CSR arguments, host or device B / X / Dinv, use_x0, history (max_iterations + 1 doubles), m = 0, bb = 0, option "reorder", the errors.
 * What differs:
 *   - Dinv is a RIGHT preconditioner: the iteration runs on A diag(Dinv) and x = diag(Dinv) y is accumulated directly, so X solves the
 *     original system and r, rr, history and the stop test rr <= max(rtol^2 * bb, atol^2) belong to the original system whatever Dinv is.
 *   - status: _BREAKDOWN: <rhat,v> = 0 or rho = 0 (nothing of the iteration is applied), or <t,t> = 0, <t,s> = 0 or omega = 0 (X keeps the half
 *     step x + alpha ph); _NONFINITE: a NaN or infinity in any dot, alpha, omega or beta.  An iteration counts from its half step on.
 *   - Workspace: r, rhat, p, v, t and y (m elements each, y only used with Dinv), eight partial arrays and the state in one block of the
 *     solver's own, and the history's device copy in another: allocated at the first BiCGStab solve, freed at destroy / clear /
 *     re-inspection, counted in spmv_hip_info.device_bytes.  spmv_hip_cg's workspace is neither shared nor grown.
 *
 * The arithmetic contract -- bits, not a tolerance; tests/bicgstab_cases.py restates it in numpy.  Elements are of the handle's type T.  Every
 * dot is spmv_hip_cg's dot exactly (the same P, L, slot, step, wave and workgroup trees; fp64 products and sums, no fma).  alpha, omega and
 * beta are formed in fp64 and rounded to T ONCE.  The vector updates are in T, every multiply and every add a separate operation.
 *   start:  x = 0, r = B  (or r = B - A*x0);  rhat = r;  p = r
 *           rho = <rhat,r>, rr = <r,r>, bb = <B,B>;  history[0] = rr
 *           nonfinite(bb, rr, rho) -> NONFINITE;  bb == 0 -> x = 0, rr = 0, CONVERGED;  rr <= thresh -> CONVERGED          (0 iterations)
 *   iteration k = 1, 2, ...:
 *           ph = Dinv*p (ph = p without Dinv);  v = A*ph                          -- the handle's multiply, spmv()'s bits
 *           rv = <rhat,v>;  nonfinite(rv, rho) -> NONFINITE;  rv == 0 or rho == 0 -> BREAKDOWN   (nothing applied, iterations = k - 1)
 *           alpha = T(rho / rv);  nonfinite(alpha) -> NONFINITE                                    (the same)
 *           x = x + alpha*ph;  s = r - alpha*v;  ss = <s,s>                       -- from here on iterations = k
 *           nonfinite(ss) -> NONFINITE;  ss <= thresh -> CONVERGED                (the half step: rr = history[k] = ss)
 *           sh = Dinv*s (sh = s);  t = A*sh
 *           ts = <t,s>, tt = <t,t>;  nonfinite -> NONFINITE;  tt == 0 or ts == 0 -> BREAKDOWN    (rr = history[k] = ss, x keeps the half step)
 *           omega = T(ts / tt);  nonfinite(omega) -> NONFINITE;  omega == 0 -> BREAKDOWN          (the same)
 *           x = x + omega*sh;  r = s - omega*t;  rho_new = <rhat,r>, rr = <r,r>;  history[k] = rr
 *           nonfinite(rr, rho_new) -> NONFINITE;  rr <= thresh -> CONVERGED
 *           beta = T((rho_new / rho) * (double(alpha) / double(omega)));  nonfinite(beta) -> NONFINITE
 *           p = r + beta*(p - omega*v)                                            -- in T: omega*v, p - that, beta * that, r + that
 *           rho = rho_new
 *   k == max_iterations without a status -> MAX_ITERATIONS.  thresh = max(rtol^2 * bb, atol^2).
 *   Consequences: res.rr and res.bb belong to the returned X; Dinv = all ones gives exactly the bits of Dinv = NULL; X, iterations, rr and
 *   history are bit-identical run to run and for every check_every (unless the handle was created with option "deterministic" = 0). */
int spmv_hip_bicgstab(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                      const void *Matrix_Val, const void *B, void *X,
                      const spmv_hip_cg_options *opt, spmv_hip_cg_result *res);

/* ---- conjugate gradients for k right-hand sides: A X = B, one pass over A per iteration ----------
 * k INDEPENDENT conjugate-gradient recurrences (1 <= k <= SPMV_HIP_CG_COLUMNS_MAX) that share the matrix stream: per iteration ONE multiply
 * Q = A P for all columns -- spmv_hip_spmm's executor, one panel, A read once -- and five vector kernels.  Every column has its own alpha,
 * beta, stop test, status and iteration count.  This is not block CG: no Krylov space is shared, a column knows nothing of the others.
 * spmv_hip_cg's rules hold word for word -- the return value, the synchronous call, the CSR arguments, use_x0, the stop test, m = 0, bb = 0,
 * the status values, option "reorder", the errors -- with these differences:
 *   - B and X are m x k, row-major with leading dimensions ldb, ldx >= k (spmv_hip_spmm's layout), host or device pointers; B's padding is
 *     never read and X's never written; B and X must not overlap.  More than SPMV_HIP_CG_COLUMNS_MAX columns: call again.
 *   - opt->Dinv is ONE vector of m elements for all columns (the preconditioner belongs to A).  rtol, atol, max_iterations, check_every and
 *     use_x0 apply to every column alike.  opt->history, when given, is a HOST array of (max_iterations + 1) * k doubles: entry [it * k + j] is
 *     column j's rr after iteration it, written for it <= res[j].iterations; the entries behind that are left as they were.
 *   - res has k entries; res[j] is column j's status, iterations, rr and bb.  The call ends when every column has ended or at max_iterations.
 *   - A column that has ended -- converged, breakdown, non-finite, or bb = 0 (its X column is set to zeros) -- is FROZEN: its X column, rr and
 *     iterations are not touched again while the others go on (it is still multiplied; that is cheaper than re-packing).
 *   - The resident ColIdx is needed as for spmv_hip_spmm with k > 1 (option keep_columns = 0: restored from the create-time arrays).
 *   - Workspace, the solver's own: r, p, q (m x k elements each, compact), 4 k partial arrays of 1024 doubles and the per-column state in one
 *     block of 3 * roundup(m * k * sizeof(T), 256) + 4 * k * 8192 + 1024 bytes, allocated at the first call and allocated anew when a later
 *     call has a larger k; the history's device copy in another; freed and counted as spmv_hip_cg's.  spmv_hip_cg's and spmv_hip_bicgstab's
 *     workspaces are neither shared nor grown.
 *   - Errors (SPMV_HIP_E_ARG, X untouched): spmv_hip_cg's, and k < 1, k > SPMV_HIP_CG_COLUMNS_MAX, ldb < k, ldx < k, NULL res.
 *   - k = 1 with ldb = ldx = 1 IS spmv_hip_cg: the same code path, workspace and bits (the handle's own multiply).  Every other form -- k = 1
 *     with a leading dimension above 1 included -- runs the k-column kernels around spmv_hip_spmm's executor.
 *
 * The per-column contract -- bits, not a tolerance; tests/cg_columns_cases.py restates it in numpy.  Column j of a call is spmv_hip_cg's
 * recurrence above, word for word: the start, the order of the updates x += alpha p; r -= alpha q; z = Dinv r; p = z + beta p (each a multiply
 * and then an add in T), alpha and beta fp64 quotients rounded to T once, every test that ends the loop and their order.  Two differences:
 *   1. The multiply is column j of spmv_hip_spmm's result: for rows of up to 512 entries ONE sequential fma chain per (row, column) in CSR
 *      order; longer rows in the 64-segment form (see spmv_hip_spmm).
 *   2. Every dot of column j is spmv_hip_cg's dot over that column's m elements by ROW index: the same P and L; the row at offset o of its
 *      workgroup has position o mod 1024 and step o / 1024 (position = 4 * thread + slot of the single solve); one accumulator per (position,
 *      column) starts at +0.0 and adds by ascending step; then the perfect adjacent-pair binary tree over the 1024 positions (slots, lanes,
 *      waves), and the same tree over the <= 1024 partials.  tests/cg_cases.dot applied to a column is the model, unchanged.  The order does
 *      not depend on k, ldb, ldx, alignment, access width, host or device pointers, or the contents or fate of another column.
 *   Consequences: X[:, j], res[j] and column j's history are bit-identical for every k in 2 .. 16, every position j, every leading dimension,
 *   every check_every and every method the handle was created with (for k > 1 the multiply does not depend on the method); a NaN or a breakdown
 *   in one column changes no bit of any other; a frozen column's X, rr and iterations stay what they were when it ended. */
#define SPMV_HIP_CG_COLUMNS_MAX 16
int spmv_hip_cg_columns(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                        const void *Matrix_Val, int k, const void *B, long long ldb, void *X, long long ldx,
                        const spmv_hip_cg_options *opt, spmv_hip_cg_result *res /* k entries */);

/* ---- restarted GMRES on the device: A x = b for a matrix that need not be symmetric -------------
 * Right-preconditioned GMRES(restart) for a square A (m = n) with an optional diagonal preconditioner; the new Krylov vector is made orthogonal
 * by classical Gram-Schmidt applied TWICE, unconditionally.  An ITERATION is one inner step: one of the handle's own multiplies -- spmv()'s
 * schedule and bits -- one new basis vector, seven vector kernels.  Within a cycle the residual estimate never rises, and the only breakdown is
 * a singular A diag(Dinv).  The coefficients, the rotations and the stop tests are formed on the device; the host enqueues check_every
 * iterations, then looks at a small state once.
 * The options, the result, the status values and EVERY rule of spmv_hip_cg above hold word for word: the return value, the synchronous call,
 * the CSR arguments, host or device B / X / Dinv, use_x0, history (max_iterations + 1 doubles), m = 0, bb = 0, option "reorder", the errors.
 * What differs:
 *   - restart < 1 or restart > SPMV_HIP_GMRES_RESTART_MAX is SPMV_HIP_E_ARG as well.
 *   - Dinv is a RIGHT preconditioner, as for spmv_hip_bicgstab: the residual, rr, the history and the stop test belong to the original system.
 *   - `iterations` counts the steps whose column is in the returned X.  rr is the recurrence's residual ESTIMATE g_(j+1)^2 of the last step
 *     applied (the initial <r,r> at 0 iterations), and so is history[k]: within a cycle no residual vector exists.  At every restart the true
 *     r = B - A x is formed and the next cycle starts from its norm; rr and the history do not show it.
 *   - status: _BREAKDOWN: the diagonal entry d of the rotated Hessenberg column is exactly 0 -- A diag(Dinv) is singular on the space built so
 *     far; X is the iterate of the last step before it -- or h_(j+1,j) = 0 (the space is exhausted) while the estimate is above the threshold:
 *     that step IS applied.  h_(j+1,j) = 0 with the estimate at or below the threshold is _CONVERGED (the lucky case).  _NONFINITE: a NaN or
 *     infinity in any dot, norm, rotation or coefficient; X is the iterate of the last step before it.  _MAX_ITERATIONS in the middle of a
 *     cycle: X includes the columns of the unfinished cycle.
 *   - Workspace, the solver's own: w, z and restart + 1 basis vectors (m elements each), 35 partial arrays of 1024 doubles and the state
 *     (the Hessenberg columns, the rotations, g, y) in one block of (restart + 3) * roundup(m * sizeof(T), 256) + 35 * 8192 + 10240 bytes,
 *     allocated at the first call and allocated anew when a later call has a larger restart; the history's device copy in another; freed
 *     and counted as spmv_hip_cg's.  The other solvers' workspaces are neither shared nor grown.
 *
 * The arithmetic contract -- bits, not a tolerance; tests/gmres_cases.py restates it in numpy.  Elements are of the handle's type T.  Every dot
 * is spmv_hip_cg's dot exactly.  Every scalar is fp64, with every product, sum, quotient and square root a separate operation; the square root
 * is the correctly rounded one (IEEE 754).  A scalar that multiplies a vector is rounded to T once.  The vector updates are in T, a multiply and
 * then an add or a subtraction, never an fma.  thresh = max(rtol^2 * bb, atol^2).
 *   start:   x = 0, r = B (or r = B - A*x0);  rr = <r,r>, bb = <B,B>;  history[0] = rr
 *            nonfinite(bb, rr) -> NONFINITE;  bb == 0 -> x = 0, rr = 0, CONVERGED;  rr <= thresh -> CONVERGED                    (0 iterations)
 *   cycle:   beta = sqrt(rr_cycle) (rr_cycle = rr at the start);  g_1 = beta;  v_1 = r * T(1 / beta)
 *   step j = 1 .. restart of the cycle, iteration k = 1, 2, ... of the call:
 *            z = Dinv*v_j (z = v_j without Dinv);  w = A*z                         -- the handle's multiply, spmv()'s bits
 *            c_i = <v_i,w>, i = 1..j (all of the same w);  a_i = T(c_i);  w = w - a_i*v_i by ascending i
 *            d_i = <v_i,w>, i = 1..j (all of the same w);  e_i = T(d_i);  w = w - e_i*v_i by ascending i;  ww = <w,w>
 *            h_i = double(a_i) + double(e_i);  hn = sqrt(ww)
 *            the rotations i = 1..j-1 by ascending i:  (h_i, h_(i+1)) = (c_i*h_i + s_i*h_(i+1),  c_i*h_(i+1) - s_i*h_i), of the old h_i and h_(i+1)
 *            d = sqrt(h_j*h_j + hn*hn)
 *            nonfinite(ww, any h_i before or after a rotation, d) -> NONFINITE;  d == 0 -> BREAKDOWN      (step not applied: iterations = k - 1)
 *            c_j = h_j / d;  s_j = hn / d;  g_(j+1) = -(s_j*g_j);  g_j = c_j*g_j (of the old g_j);  est = g_(j+1)*g_(j+1)
 *            nonfinite(c_j, s_j, g_j, est) -> NONFINITE                                                    (the same)
 *            h_j = d;  iterations = k;  rr = history[k] = est                      -- from here on the step is applied
 *            est <= thresh -> CONVERGED;  hn == 0 -> BREAKDOWN
 *            v_(j+1) = w * T(1 / hn)
 *   cycle end, behind step j = restart and when the loop has ended or k = max_iterations, over the n steps of the cycle that were applied:
 *            R y = g in fp64 with R the rotated columns: rows n .. 1; row i: sum = +0.0, then sum = sum + R_(i,c)*y_c by ascending c > i;
 *            y_i = (g_i - sum) / R_(i,i) (the unrounded y_c enter the later rows)
 *            u = T(y_1)*v_1, then u = u + T(y_i)*v_i by ascending i;  x = x + Dinv*u (x = x + u without Dinv)
 *   restart, behind every FULL cycle (also when k = max_iterations falls on it):
 *            r = B - A*x (the multiply, then a subtraction in T);  rr_cycle = <r,r>;  nonfinite -> NONFINITE;  rr_cycle == 0 -> CONVERGED
 *   k == max_iterations without a status -> MAX_ITERATIONS.
 *   Consequences: a run with max_iterations = k returns the iterate k of a longer run, restart boundaries included; Dinv = all ones gives
 *   exactly the bits of Dinv = NULL; X, iterations, rr and history are bit-identical run to run, for every check_every, for host or device
 *   pointers and every pointer alignment (unless the handle was created with option "deterministic" = 0). */
#define SPMV_HIP_GMRES_RESTART_MAX 32
int spmv_hip_gmres(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                   const void *Matrix_Val, const void *B, void *X, int restart,
                   const spmv_hip_cg_options *opt, spmv_hip_cg_result *res);

/* ---- mixed-precision conjugate gradients: an fp64 solution from fp32 iterations ------------------
 * Conjugate gradients with reliable updates (Clark et al., "Solving lattice QCD systems of equations using mixed precision solvers on GPUs",
 * 2010) on a PAIR of handles: `high` holds the matrix in fp64, `low` the same pattern with the values rounded to float; the caller created
 * both and keeps them in step (spmv_hip_update_values on each).  Every iteration is spmv_hip_cg's in float on `low`'s multiply and gathers a
 * partial solution y; when a SEGMENT of iterations ends, x + y goes through `high`'s fp64 multiply once, the true residual b - A (x + y)
 * replaces the recurrence's, and the search direction p is KEPT -- restarting it at every update (iterative refinement around an fp32 solve)
 * costs about twice the iterations.  B and X are fp64; every return carries the TRUE fp64 rr of the X it returns.
 *   - There are no CSR arguments: the call solves with the two RESIDENT matrices as they are.
 *   - B and X: m doubles; Dinv: m FLOATS; host or device pointers, staged through `high`'s buffers as spmv_hip_cg stages them; B and X must
 *     not overlap.  The call is synchronous and returns SPMV_HIP_OK whenever the solve ran.  rtol, atol, max_iterations, check_every, use_x0
 *     and history have spmv_hip_cg's meaning and validation; m = 0 and bb = 0 behave as there.
 *   - update_drop: a segment ends when the recurrence's rr has fallen to update_drop^2 times its value at the segment's start; 0 means
 *     SPMV_HIP_CG_MIXED_UPDATE_DROP.  update_every: a segment also ends after that many iterations; 0: no such cap.
 *   - status: spmv_hip_cg's four and SPMV_HIP_CG_STAGNATED: the narrowed residual is all zeros while rr is above the threshold, or an update
 *     that the recurrence called progress did not lower the true rr -- fp32 iterations cannot improve this x further (`low` may not be
 *     `high`'s matrix, or rtol is below what the fp64 multiply resolves).  `updates` counts the committed updates.
 *   - Workspace: xn, q64 (m doubles each), r, p, q, y (m floats each), six arrays of 1024 partial sums and the state in ONE block of
 *     2 * up256(8 m) + 4 * up256(4 m) + 6 * 8192 + 256 bytes (up256: rounded up to a multiple of 256), owned by `high`: allocated at the
 *     first call, freed at `high`'s destroy / clear / re-inspection, counted in `high`'s device_bytes; the history's device copy likewise.
 *     The other solvers' workspaces are not shared or grown.  `low` is not changed; its own spmv_hip_cg workspace is not used.
 *   - Errors (SPMV_HIP_E_ARG, X untouched): `high` not fp64 or `low` not fp32; m, n or nnz that differ between the handles, or m != n;
 *     handles on different devices or streams; either handle multi-GPU, host_rows or created with option "reorder"; NULL opt or res; NULL B
 *     or X when m > 0; spmv_hip_cg's option errors; update_drop outside [0, 1) or NaN; update_every < 0.  A cleared or failed handle on
 *     either side: SPMV_HIP_E_NOSTATE.
 *   - The narrowed residual is not scaled: elements of r64 below 2^-126 lose bits on narrowing, and one above FLT_MAX becomes an infinity
 *     (NONFINITE).
 *
 * The arithmetic contract -- bits, not a tolerance; tests/cg_mixed_cases.py restates it in numpy.  "dot" is spmv_hip_cg's dot over m fp64
 * elements, or over fp32 elements widened.  All scalars are fp64.  Every product, sum and quotient is separate (no fma).  "narrow" is
 * round-to-nearest-even to float; widening is exact.  thr = max(rtol^2 * bb, atol^2).
 *   start:     x = X (use_x0) or 0;  q64 = A_high*x through `high`'s own multiply (only with use_x0);  r64 = b - q64, or b;
 *              bb = dot(b,b);  rr = dot(r64,r64);  non-finite bb or rr -> NONFINITE;  bb == 0 -> X = 0, CONVERGED;  rr <= thr -> CONVERGED;
 *              max_iterations == 0 -> MAX_ITERATIONS;  else the first segment starts.
 *   segment start:  r = narrow(r64);  y = 0;  z = Dinv*r (an fp32 multiply; z = r without Dinv);  rz = dot(r,z);  rs = dot(r,r);  seg = rs;  n = 0;
 *              non-finite rs or rz -> NONFINITE;  rs == 0 -> STAGNATED;  rz <= 0 -> BREAKDOWN;
 *              p = z in the first segment and behind a segment that ended "exact"; otherwise p is KEPT as the last iteration left it.
 *   iteration (spmv_hip_cg's with T = float, on y in the place of x):
 *              q = A_low*p through `low`'s own multiply;  pq = dot(p,q);  non-finite pq or rz -> NONFINITE;  pq <= 0 -> BREAKDOWN;
 *              alpha = float(rz / pq), non-finite -> NONFINITE;  y = y + alpha*p;  r = r - alpha*q;  z as above;
 *              rzn = dot(r,z);  rs = dot(r,r);  iterations and n each increase by one;  then, in this order:
 *              1. non-finite rs or rzn -> NONFINITE;  2. rs == 0 ends the segment "exact", p untouched;  3. rzn <= 0 -> BREAKDOWN;
 *              4. beta = float(rzn / rz), non-finite -> NONFINITE;  5. p = z + beta*p;  rz = rzn;
 *              6. the segment ends on the first that holds: "estimate": rs <= thr;  "drop": rs <= (update_drop*update_drop)*seg;
 *                 "every": n == update_every;  "budget": iterations == max_iterations.
 *              BREAKDOWN or NONFINITE inside a segment ends the solve with X = x of the last committed update, y discarded, and rr that x's.
 *   update:    xn = x + widen(y), an fp64 add;  q64 = A_high*xn;  r64n = b - q64;  rrn = dot(r64n,r64n);
 *              non-finite rrn -> NONFINITE, x kept;  rrn >= rr behind a segment that ended "exact", "estimate" or "drop" -> STAGNATED, x and rr
 *              kept;  otherwise commit: x = xn, r64 = r64n, rr = rrn, updates + 1;  then rr <= thr -> CONVERGED;  else iterations ==
 *              max_iterations -> MAX_ITERATIONS;  else a new segment starts.
 *   history:   history[0] is the initial rr;  history[k] is rs after iteration k;  where a committed update follows iteration k, the
 *              committed rr overwrites history[k].
 *   Consequences: X, status, iterations, updates, rr and history are bit-identical run to run, for every check_every, for host or device
 *   pointers and every pointer alignment; Dinv = all ones gives the bits of Dinv = NULL; a run with max_iterations = k returns what a longer
 *   run held after iteration k plus one update (unless the handles were created with option "deterministic" = 0). */
enum { SPMV_HIP_CG_STAGNATED = 4 };   /* returned by spmv_hip_cg_mixed alone */
/* the default update_drop: tools/cg_mixed_bench.py's sweep over {0.5, 0.1, 0.01} */
#define SPMV_HIP_CG_MIXED_UPDATE_DROP 0.01
typedef struct spmv_hip_cg_mixed_options {
    double rtol, atol;        /* stop when the TRUE rr <= max(rtol^2 * bb, atol^2) */
    int max_iterations;       /* >= 0 */
    int check_every;          /* iterations enqueued between two looks at the device's state; 0 = default */
    int use_x0;               /* 0: start from x = 0 (X is only written); != 0: X holds the initial guess */
    const float *Dinv;        /* NULL, or m floats, host or device: z = Dinv .* r in the fp32 recurrence */
    double *history;          /* NULL, or HOST array of max_iterations + 1 doubles */
    double update_drop;       /* 0 = default; else 0 < update_drop < 1 */
    int update_every;         /* >= 0; 0 = no cap on a segment's length */
} spmv_hip_cg_mixed_options;
typedef struct spmv_hip_cg_mixed_result {
    int status;               /* SPMV_HIP_CG_CONVERGED 0, _MAX_ITERATIONS 1, _BREAKDOWN 2, _NONFINITE 3, _STAGNATED 4 */
    int iterations;           /* fp32 iterations applied */
    int updates;              /* fp64 updates committed */
    double rr, bb;            /* the TRUE <b - A x, b - A x> of the returned x, and <b,b> */
} spmv_hip_cg_mixed_result;
int spmv_hip_cg_mixed(spmv_Handle_t high, spmv_Handle_t low, const double *B, double *X,
                      const spmv_hip_cg_mixed_options *opt, spmv_hip_cg_mixed_result *res);

/* ---- LSQR on the device: least squares for a matrix of any shape ---------------------------------
 * LSQR (Paige and Saunders, "LSQR: an algorithm for sparse linear equations and sparse least squares", 1982) minimises
 * |A x - b|^2 + damp^2 |x|^2 for ANY m x n matrix: an overdetermined fit, the minimum-norm solution of an underdetermined system, a ridge
 * regression.  Per iteration the handle's own multiply q = A v -- spmv()'s schedule and bits --, the multiply qt = A^T u of the transpose
 * that spmv_hip_spmv_transpose uses -- its bits -- and four vector kernels.  The bidiagonalisation's alpha and beta, the rotations and the
 * stop tests are formed on the device; the host enqueues check_every iterations, then looks at a small state once.
 *   - Returns SPMV_HIP_OK whenever the solve RAN; synchronous, as spmv_hip_cg.  The CSR arguments follow spmv()'s rules, as in spmv_hip_cg.
 *   - B: m elements, X: n elements, of the handle's type, host or device pointers (host ones are staged through the buffers spmv_hip_cg's B and X
 *     use); they must not overlap.  use_x0 = 0: the solve starts from x = 0 and X is only written; otherwise X holds x0, the iterations run on
 *     r0 = B - A x0, and the damping acts on x - x0.  There is no Dinv.
 *   - The transpose is built at the first call, as by spmv_hip_prepare_transpose, counted in device_bytes and kept in step with
 *     spmv_hip_update_values and in-place value changes as spmv_hip_spmv_transpose keeps it.
 *   - Stop: rr <= max(rtol^2 * bb, atol^2) with rr the recurrence's ESTIMATE of |r|^2 + damp^2 |x - x0|^2 (spmv_hip_cg's rule) -> _CONVERGED;
 *     ar <= ls_tol * (anorm * sqrt(rr)) with ar the estimate of |A^T r - damp^2 (x - x0)| and anorm the running estimate of the Frobenius
 *     norm of [A; damp I] -> SPMV_HIP_LSQR_LEAST_SQUARES: x is a least-squares solution of a system that need not be consistent.
 *     _MAX_ITERATIONS and _NONFINITE (a NaN or infinity in a dot, a scalar of the chain or a factor of a vector) keep their meaning;
 *     _BREAKDOWN is never returned.  rtol = atol = ls_tol = 0 runs max_iterations iterations unless rr or ar reaches 0.
 *   - m = 0 or bb = 0: X is set to zeros, converged, 0 iterations.  ar and anorm are 0 at every end that comes before alpha is formed.
 *   - history (a HOST array of max_iterations + 1 doubles, or NULL) receives rr after iteration 0, 1, ..., iterations.
 *   - Workspace, the solver's own: u, q (m elements each), v, w, qt (n elements each), three arrays of 1024 partial sums and the state in ONE
 *     block of 2 * up256(m * sizeof(T)) + 3 * up256(n * sizeof(T)) + 3 * 8192 + 256 bytes, allocated at the first call; the history's device
 *     copy in another; freed and counted as spmv_hip_cg's.  The other solvers' workspaces are neither shared nor grown.
 *   - Errors (SPMV_HIP_E_ARG, X untouched): NULL opt or res; NULL B when m > 0, NULL X when n > 0; a negative or NaN rtol, atol, ls_tol or
 *     damp; max_iterations < 0, check_every < 0; multi-GPU handles, host_rows handles, handles created with option "reorder".  A cleared or
 *     failed handle: SPMV_HIP_E_NOSTATE.
 *
 * The arithmetic contract -- bits, not a tolerance; tests/lsqr_cases.py restates it in numpy.  Elements are of the handle's type T; all scalars
 * are fp64, with every product, sum, quotient and square root a separate operation; the square root is spmv_hip_gmres's, the correctly rounded
 * one.  dot(a,a) is spmv_hip_cg's dot over a's OWN length: P and L follow from m for B and u, from n for v.  A scalar that multiplies or divides
 * a vector is rounded to T once; the vector operations are in T, a multiply and then an add or a subtraction, never an fma; a division is a
 * division (not a multiplication by a reciprocal).  thr = max(rtol^2 * bb, atol^2).
 *   start:   x = 0 (or X);  u = B (or u = B - A*x through the handle's multiply);  bb = dot(B,B);  uu = dot(u,u)
 *            nonfinite(bb, uu) -> NONFINITE;  bb == 0 -> X = 0, rr = 0, CONVERGED;  rr = uu = history[0];  rr <= thr -> CONVERGED   (0 iterations)
 *            beta = sqrt(uu);  u = u / T(beta);  v = A^T*u -- the transpose's own multiply;  vv = dot(v,v);  nonfinite(vv) -> NONFINITE
 *            alpha = sqrt(vv);  alpha == 0 -> LEAST_SQUARES, ar = 0;  v = v / T(alpha);  w = v
 *            phibar = beta;  rhobar = alpha;  a2 = alpha*alpha;  psi2 = 0;  ar = alpha*beta;  anorm = sqrt(a2)
 *            max_iterations == 0 -> MAX_ITERATIONS
 *   iteration k = 1, 2, ...:
 *         1. q = A*v                                                            -- the handle's multiply, spmv()'s bits
 *         2. u = q - T(alpha)*u;  uu = dot(u,u);  nonfinite(uu) -> NONFINITE                                       (iterations = k - 1)
 *         3. beta = sqrt(uu);  beta > 0: u = u / T(beta)
 *         4. qt = A^T*u                                                         -- always enqueued
 *         5. v = qt - T(beta)*v;  vv = dot(v,v);  nonfinite(vv) -> NONFINITE                                       (iterations = k - 1)
 *         6. alpha = sqrt(vv);  alpha > 0: v = v / T(alpha)
 *         7. a2 = ((a2 + beta*beta) + alpha*alpha) + damp*damp
 *         8. rhobar1 = sqrt(rhobar*rhobar + damp*damp);  c1 = rhobar / rhobar1;  s1 = damp / rhobar1
 *         9. psi = s1*phibar;  phibar = c1*phibar;  psi2 = psi2 + psi*psi
 *        10. rho = sqrt(rhobar1*rhobar1 + beta*beta);  c = rhobar1 / rho;  s = beta / rho
 *        11. theta = s*alpha;  rhobar = -(c*alpha);  phi = c*phibar;  phibar = s*phibar (of the phibar of step 9);  tau = s*phi
 *        12. nonfinite(T(phi / rho)) or nonfinite(T(theta / rho)) -> NONFINITE                                     (iterations = k - 1)
 *        13. x = x + T(phi / rho)*w                                             -- from here on iterations = k
 *        14. rr = phibar*phibar + psi2 = history[k];  ar = alpha*|tau|;  anorm = sqrt(a2)
 *        15. in this order: nonfinite(rr, ar, a2) -> NONFINITE;  rr <= thr -> CONVERGED;  ar <= ls_tol*(sqrt(a2)*sqrt(rr)) -> LEAST_SQUARES
 *            (beta == 0 and alpha == 0 end here or at the test before it: ar is 0)
 *        16. otherwise w = v - T(theta / rho)*w
 *        17. k == max_iterations without a status -> MAX_ITERATIONS
 *   An end with iterations = k - 1 returns the x, rr, ar, anorm and history of iteration k - 1.
 *   Consequences: X, status, iterations, rr, ar, anorm and history are bit-identical run to run, for every check_every, for host or device
 *   pointers and every pointer alignment; a run with max_iterations = k returns the iterate k of a longer run; the handle's method changes the
 *   bits only as far as it changes spmv()'s and spmv_hip_spmv_transpose's (unless the handle was created with option "deterministic" = 0). */
enum { SPMV_HIP_LSQR_LEAST_SQUARES = 5 };   /* returned by spmv_hip_lsqr alone */
typedef struct spmv_hip_lsqr_options {
    double rtol, atol;        /* stop when rr <= max(rtol^2 * bb, atol^2) */
    double ls_tol;            /* stop when ar <= ls_tol * (anorm * sqrt(rr)) */
    double damp;              /* >= 0 */
    int max_iterations;       /* >= 0 */
    int check_every;          /* iterations enqueued between two looks at the device's state; 0 = default */
    int use_x0;               /* 0: start from x = 0 (X is only written); != 0: X holds the initial guess */
    double *history;          /* NULL, or HOST array of max_iterations + 1 doubles: rr after iteration 0, 1, ... */
} spmv_hip_lsqr_options;
typedef struct spmv_hip_lsqr_result {
    int status;               /* SPMV_HIP_CG_CONVERGED 0, _MAX_ITERATIONS 1, _NONFINITE 3, SPMV_HIP_LSQR_LEAST_SQUARES 5 */
    int iterations;           /* updates of x that were applied */
    double rr, bb;            /* the residual estimate of the returned x, and <b,b> */
    double ar;                /* the estimate of |A^T r - damp^2 x| */
    double anorm;             /* the running Frobenius estimate sqrt(a2) */
} spmv_hip_lsqr_result;
int spmv_hip_lsqr(spmv_Handle_t handle, BASIC_INT_TYPE m, const BASIC_INT_TYPE *RowPtr, const BASIC_INT_TYPE *ColIdx,
                  const void *Matrix_Val, const void *B, void *X,
                  const spmv_hip_lsqr_options *opt, spmv_hip_lsqr_result *res);

#endif /* SPMV_HIP_EXT_H */

#if defined(__cplusplus)
}
#endif
