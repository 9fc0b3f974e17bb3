// spmv_transpose.hip -- translation unit of the transpose builder's kernels (kernels/transpose.hpp).  Launches only: allocation, the scan
// between the radix passes, the child matrix and the error channel stay in spmv_shim.hip (shim/transpose.hpp).
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
#include "kernels/transpose.hpp"

namespace spmv {

hipError_t tr_rows_launch(int m, const int *rowptr, int *row_of, int cus, hipStream_t stream)
{
    if (m > 0) tr_rows_kernel<<<grid_for(m, kBlock / kWave, cus * 32), kBlock, 0, stream>>>(m, rowptr, row_of);
    return hipGetLastError();
}

hipError_t tr_hist_launch(long long nnz, int tiles, int shift, const int *keys, int *cnt, hipStream_t stream)
{
    if (tiles > 0) tr_hist_kernel<<<tiles, kBlock, 0, stream>>>(nnz, tiles, shift, keys, cnt);
    return hipGetLastError();
}

hipError_t tr_scatter_launch(long long nnz, int tiles, int shift, const int *keys, const int *vals, const int *off, int *keys_out, int *vals_out, hipStream_t stream)
{
    if (tiles > 0) tr_scatter_kernel<<<tiles, kBlock, 0, stream>>>(nnz, tiles, shift, keys, vals, off, keys_out, vals_out);
    return hipGetLastError();
}

hipError_t tr_rowptr_launch(int n, long long nnz, const int *sorted, int *rowptr_t, int cus, hipStream_t stream)
{
    tr_rowptr_kernel<<<grid_for((long long) n + 1, kBlock, cus * 8), kBlock, 0, stream>>>(n, nnz, sorted, rowptr_t);
    return hipGetLastError();
}

hipError_t tr_columns_launch(long long nnz, const int *perm, const int *row_of, int *colidx_t, int cus, hipStream_t stream)
{
    if (nnz > 0) tr_columns_kernel<<<grid_for(nnz, kBlock, cus * 16), kBlock, 0, stream>>>(nnz, perm, row_of, colidx_t);
    return hipGetLastError();
}

hipError_t tr_gather_launch(long long nnz, const int *perm, const void *val, void *val_t, bool f64, int cus, hipStream_t stream)
{
    if (nnz > 0) {
        if (f64) tr_gather_kernel<double><<<grid_for(nnz, kBlock, cus * 16), kBlock, 0, stream>>>(nnz, perm, (const double *) val, (double *) val_t);
        else tr_gather_kernel<float><<<grid_for(nnz, kBlock, cus * 16), kBlock, 0, stream>>>(nnz, perm, (const float *) val, (float *) val_t);
    }
    return hipGetLastError();
}

} // namespace spmv
