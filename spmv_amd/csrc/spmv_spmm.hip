// spmv_spmm.hip -- translation unit of the k-right-hand-side executors (kernels/spmm.hpp).  Launches only: allocation, staging and the
// error channel stay in spmv_shim.hip (shim/spmm.hpp), which calls spmm_launch once per panel.
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
#include "kernels/dispatch.hpp"
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

hipError_t spmm_launch(const SpmmArgs &a, bool f64, hipStream_t stream)
{
    with_type_vec(f64, a.vec, [&](auto t, auto vec) {
        using T = decltype(t);
        // the narrowest lane group that covers the panel's columns
        with_width(panel_group_width<T>(a.kc), [&](auto CW) { spmm_launch_cw<T, decltype(CW)::value, decltype(vec)::value>(a, stream); });
    });
    return hipGetLastError();
}

} // namespace spmv
