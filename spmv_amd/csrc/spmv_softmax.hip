// spmv_softmax.hip -- translation unit of the row reductions over nnz-sized arrays (kernels/row_softmax.hpp: the row softmax and its
// backward).  Launches only: the tables, staging and the error channel stay in spmv_shim.hip (shim/row_softmax.hpp), which calls
// row_reduce_launch once per call.
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
#include "kernels/row_softmax.hpp"

namespace spmv {

template <typename T, bool BWD>
static void row_reduce_launch_t(const RowReduceArgs &a, hipStream_t stream)
{
    constexpr int waves = kBlock / kWave;
    if (a.nb > 0)
        row_reduce_rows_kernel<T, BWD><<<(unsigned) ((a.nb + waves - 1) / waves), kBlock, 0, stream>>>(a.nb, a.split, a.rowptr, (const T *) a.a, (const T *) a.g, (T *) a.out);
    if (a.nlong > 0)
        row_reduce_long_kernel<T, BWD><<<grid_for(a.nlong, 1, a.cus * 8), kBlock, 0, stream>>>(a.nlong, a.longs, a.rowptr, (const T *) a.a, (const T *) a.g, (T *) a.out);
}

hipError_t row_reduce_launch(const RowReduceArgs &a, bool f64, hipStream_t stream)
{
    if (a.m <= 0) return hipSuccess;
    if (f64) { if (a.backward) row_reduce_launch_t<double, true>(a, stream); else row_reduce_launch_t<double, false>(a, stream); }
    else { if (a.backward) row_reduce_launch_t<float, true>(a, stream); else row_reduce_launch_t<float, false>(a, stream); }
    return hipGetLastError();
}

} // namespace spmv
