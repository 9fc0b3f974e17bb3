// spmv_spmm.hip -- translation unit of the k-right-hand-side executors (kernels/spmm.hpp).  Launches only: allocation, staging and the
// error channel stay in spmv_shim.hip (shim/spmm.hpp), which calls spmm_launch once per panel.
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
#include "kernels/spmm.hpp"

namespace spmv {

template <typename T, int CW, bool VEC>
static void spmm_launch_cw(const SpmmArgs &a, hipStream_t stream)
{
    const T *x = (const T *) a.x;
    T *y = (T *) a.y;
    constexpr int waves = kBlock / kWave;
    if (a.nb > 0)
        spmm_rows_kernel<T, CW, VEC><<<(a.nb + waves - 1) / waves, kBlock, 0, stream>>>(a.nb, a.split, a.rowptr, a.colidx, (const T *) a.val, a.kc, x, a.ldx, y, a.ldy);
    if (a.nlong > 0)
        spmm_long_kernel<T, CW, VEC><<<a.nlong < a.cus * 8 ? a.nlong : a.cus * 8, kBlock, 0, stream>>>(a.nlong, a.longs, a.rowptr, a.colidx, (const T *) a.val, a.kc, x,
                                                                                                  a.ldx, y, a.ldy);
}

template <typename T, bool VEC>
static void spmm_launch_t(const SpmmArgs &a, hipStream_t stream)
{
    constexpr int V = SpmmShape<T>::V;
    // the narrowest lane group that covers the panel's columns
    if (a.kc <= V) spmm_launch_cw<T, 1, VEC>(a, stream);
    else if (a.kc <= 2 * V) spmm_launch_cw<T, 2, VEC>(a, stream);
    else if (a.kc <= 4 * V) spmm_launch_cw<T, 4, VEC>(a, stream);
    else spmm_launch_cw<T, 8, VEC>(a, stream);
}

hipError_t spmm_launch(const SpmmArgs &a, bool f64, hipStream_t stream)
{
    if (f64) { if (a.vec) spmm_launch_t<double, true>(a, stream); else spmm_launch_t<double, false>(a, stream); }
    else { if (a.vec) spmm_launch_t<float, true>(a, stream); else spmm_launch_t<float, false>(a, stream); }
    return hipGetLastError();
}

} // namespace spmv
