// spmv_sddmm.hip -- translation unit of the sampled dense-dense product (kernels/sddmm.hpp).  Launches only: planning, staging and the
// error channel stay in spmv_shim.hip (shim/sddmm.hpp), which calls sddmm_launch once per call.
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
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

template <typename T, bool VEC>
static void sddmm_launch_t(const SddmmArgs &a, hipStream_t stream)
{
    switch (sddmm_group_width(a.k, SddmmShape<T>::W)) { // a function of k and the value type alone: it fixes the summation order
    case 1: sddmm_launch_cw<T, 1, VEC>(a, stream); break;
    case 2: sddmm_launch_cw<T, 2, VEC>(a, stream); break;
    case 4: sddmm_launch_cw<T, 4, VEC>(a, stream); break;
    default: sddmm_launch_cw<T, 8, VEC>(a, stream); break;
    }
}

hipError_t sddmm_launch(const SddmmArgs &a, bool f64, hipStream_t stream)
{
    if (a.nnz <= 0 || a.m <= 0) return hipSuccess;
    if (f64) { if (a.vec) sddmm_launch_t<double, true>(a, stream); else sddmm_launch_t<double, false>(a, stream); }
    else { if (a.vec) sddmm_launch_t<float, true>(a, stream); else sddmm_launch_t<float, false>(a, stream); }
    return hipGetLastError();
}

} // namespace spmv
