// spmv_vector.hip -- translation unit of the CSR-vector family's executors (kernels/csr_vector4.hpp, kernels/csr_vector_tile.hpp): the tile
// and pipe kernels of CSR-vector, the rows kernel of Balanced and of CSR-vector's wide form.  Launches only: which form runs is decided in
// spmv_shim.hip (shim/launch.hpp: vector_args), which calls vector_launch / rows_launch with the resolved VecArgs.  They return the launch's
// error without clearing it: the shim's launch() and autotune check hipGetLastError() after their launches, as for every other kernel.
// Seven lanes-per-row values x the forms x two value types are most of the library's device code: build.py compiles this file four
// times, SPMV_VEC_PART = 0 / 1 the tile and pipe kernels in fp64 / fp32, 2 / 3 the rows kernel in fp64 / fp32, side by side -- and a fifth time,
// SPMV_VEC_PART = 4, for the fp64 tile kernel over packed value planes (as much device code again as the fp64 tile kernel itself).
#include <hip/hip_runtime.h>

#include "kernels/common.hpp"
#include "kernels/csr_vector4.hpp"
#include "kernels/xwindows.hpp"
#include "kernels/csr_vector_tile.hpp"

#ifndef SPMV_VEC_PART
#error "spmv_vector.hip is compiled with -DSPMV_VEC_PART=0..4"
#endif

namespace spmv {

// the staged x windows of the largest tile + the zero slot, in whole KiB
template <typename T> static size_t vec_lds_bytes(const VecArgs &a) { return xwin_lds_bytes(a.maxspan, sizeof(T)); }

template <typename F>
static void with_lanes(int lanes, F f)
{
    switch (lanes) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 8: f(std::integral_constant<int, 8>()); break;
    case 16: f(std::integral_constant<int, 16>()); break;
    case 32: f(std::integral_constant<int, 32>()); break;
    default: f(std::integral_constant<int, 64>()); break;
    }
}

#if SPMV_VEC_PART < 2 || SPMV_VEC_PART == 4
// One workgroup per kVecNB * (256/L) consecutive rows, dispatched in row order: measured on the
// config-2 shape a plain in-order grid beats a persistent grid-stride loop by ~10 %.
constexpr int kVecNB = 4;

#if SPMV_VEC_PART == 4
// fp64 tiles with packed value planes (VecArgs::pk_e): the same kernel with the PACK flag, two or four steps in flight
template <int L, int DEPTH, bool PRE>
static void launch_tile_packed(const VecArgs &a, const double *x, double *y)
{
    const size_t lds = vec_lds_bytes<double>(a);
    ensure_lds<csr_vector_tile_kernel<double, L, DEPTH, PRE, true>>(a.device, lds);
    csr_vector_tile_kernel<double, L, DEPTH, PRE, true><<<a.tiles, kVecTileThreads, lds, a.stream>>>(a.m, a.long_thr, a.rowptr, a.colidx, a.col, (const double *) a.val, a.wins,
                                                                                                    a.rowslot, a.col8, a.tmpl, a.rowtid, x, y, a.pk_lo, a.pk_hi, a.pk_e);
}

hipError_t vector_launch_packed(const VecArgs &a, const double *x, double *y)
{
    with_lanes(a.lanes, [&](auto L) {
        constexpr int LL = decltype(L)::value;
        if (a.depth == 4) { if (a.pre) launch_tile_packed<LL, 4, true>(a, x, y); else launch_tile_packed<LL, 4, false>(a, x, y); }
        else { if (a.pre) launch_tile_packed<LL, 2, true>(a, x, y); else launch_tile_packed<LL, 2, false>(a, x, y); }
    });
    return hipPeekAtLastError();
}
#else
template <typename T, int L, int DEPTH, bool PRE>
static void launch_tile(const VecArgs &a, const T *x, T *y)
{
    const size_t lds = vec_lds_bytes<T>(a);
    ensure_lds<csr_vector_tile_kernel<T, L, DEPTH, PRE>>(a.device, lds);
    csr_vector_tile_kernel<T, L, DEPTH, PRE><<<a.tiles, kVecTileThreads, lds, a.stream>>>(a.m, a.long_thr, a.rowptr, a.colidx, a.col, (const T *) a.val, a.wins,
                                                                                          a.rowslot, a.col8, a.tmpl, a.rowtid, x, y);
}

template <typename T, int L>
static void launch_vector(const VecArgs &a, const T *x, T *y)
{
    if (a.kernel == kVecTileKernel) {
        if (a.depth == 8) launch_tile<T, L, 8, true>(a, x, y);
        else if (a.depth == 4) { if (a.pre) launch_tile<T, L, 4, true>(a, x, y); else launch_tile<T, L, 4, false>(a, x, y); }
        else { if (a.pre) launch_tile<T, L, 2, true>(a, x, y); else launch_tile<T, L, 2, false>(a, x, y); }
        return;
    }
    constexpr int rows = kBlock / L * kVecNB;
    csr_vector_pipe_kernel<T, L, kVecNB><<<grid_for(a.m, rows, INT_MAX), kBlock, 0, a.stream>>>(a.m, a.long_thr, a.rowptr, a.colidx, (const T *) a.val, x, y);
}

using Val = std::conditional<SPMV_VEC_PART == 0, double, float>::type;
hipError_t vector_launch(const VecArgs &a, const Val *x, Val *y)
{
#if SPMV_VEC_PART == 0
    if (a.kernel == kVecTileKernel && a.pk_e && a.depth != 8) return vector_launch_packed(a, x, y);
#endif
    with_lanes(a.lanes, [&](auto L) { launch_vector<Val, decltype(L)::value>(a, x, y); });
    return hipPeekAtLastError();
}
#endif
#else
template <typename T, int L, int DEPTH, bool WIDE>
static void launch_rows(const VecArgs &a, const T *x, T *y)
{
    const size_t lds = vec_lds_bytes<T>(a);
    ensure_lds<csr_vector_rows_kernel<T, L, DEPTH, WIDE>>(a.device, lds);
    csr_vector_rows_kernel<T, L, DEPTH, WIDE><<<a.tiles, kVecTileThreads, lds, a.stream>>>(a.long_thr, a.split, a.rows, a.m, a.rowptr, a.colidx, a.col, (const T *) a.val,
                                                                                          a.wins, a.rowslot, a.col8, a.tmpl, a.rowtid, x, y);
}

template <typename T, int L>
static void launch_rows_form(const VecArgs &a, const T *x, T *y)
{
    if (a.depth == 2) { if (a.wide) launch_rows<T, L, 2, true>(a, x, y); else launch_rows<T, L, 2, false>(a, x, y); }
    else { if (a.wide) launch_rows<T, L, 4, true>(a, x, y); else launch_rows<T, L, 4, false>(a, x, y); }
}

using Val = std::conditional<SPMV_VEC_PART == 2, double, float>::type;
hipError_t rows_launch(const VecArgs &a, const Val *x, Val *y)
{
    with_lanes(a.lanes, [&](auto L) { launch_rows_form<Val, decltype(L)::value>(a, x, y); });
    return hipPeekAtLastError();
}
#endif

} // namespace spmv
