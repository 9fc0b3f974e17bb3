// spmv_sddmm.hip -- translation unit of the sampled dense-dense product (kernels/sddmm.hpp).  Launches only: planning, staging and the
// error channel stay in spmv_shim.hip (shim/sddmm.hpp), which calls sddmm_launch once per call.
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
#include "kernels/dispatch.hpp"
#include "kernels/sddmm.hpp"

namespace spmv {

template <typename T, int CW, bool VEC>
static void sddmm_launch_cw(const SddmmArgs &a, hipStream_t stream)
{
    constexpr int waves = kBlock / kWave;
    const long long nw = (a.nnz + kSddmmWaveNnz - 1) / kSddmmWaveNnz;
    sddmm_kernel<T, CW, VEC><<<(unsigned) ((nw + waves - 1) / waves), kBlock, 0, stream>>>(a.m, a.nnz, a.rowptr, a.colidx, a.k, (const T *) a.u, a.ldu, (const T *) a.v, a.ldv,
                                                                                         (T *) a.out);
}

hipError_t sddmm_launch(const SddmmArgs &a, bool f64, hipStream_t stream)
{
    if (a.nnz <= 0 || a.m <= 0) return hipSuccess;
    with_type_vec(f64, a.vec, [&](auto t, auto vec) {
        using T = decltype(t);
        // lanes per entry: a function of k and the value type alone, it fixes the summation order
        with_width(panel_group_width<T>(a.k), [&](auto CW) { sddmm_launch_cw<T, decltype(CW)::value, decltype(vec)::value>(a, stream); });
    });
    return hipGetLastError();
}

} // namespace spmv
