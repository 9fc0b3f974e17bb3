// storage16.hpp -- the 16-bit STORAGE types of the panel blocks (kernels/sddmm.hpp, kernels/row_blocks.hpp): IEEE binary16 and bfloat16 as
// what an operand is in memory, beside the arithmetic type float that every register holds.  A block that takes a storage type S beside its
// arithmetic type T loads S, widens in registers and runs T's code unchanged; S = T (the default everywhere) is the code from before.
//
// The conversions are written out here and nowhere else:
//   widen   bf16 -> fp32 is a 16-bit shift; fp16 -> fp32 is the hardware conversion (v_cvt_f32_f16).  Both are exact: subnormals keep their
//           values (the kernels run in the default mode, which flushes nothing), infinities and NaN stay what they are.
//   narrow  fp32 -> fp16 (v_cvt_f16_f32) and fp32 -> bf16 (v_cvt_pk_bf16_f32) round to nearest, ties to even: overflow gives +-inf, NaN stays
//           NaN, the sign of zero is kept, results below the smallest normal are subnormals.
//   a lane's segment of 4 columns is 8 bytes: one 8-byte access where the address allows (st16_load4 / st16_store4), 2-byte accesses otherwise.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace spmv {

struct f16_t { unsigned short bits; };  // IEEE binary16
struct bf16_t { unsigned short bits; }; // bfloat16: the upper half of a binary32

template <typename S> inline constexpr bool is_storage16 = std::is_same_v<S, f16_t> || std::is_same_v<S, bf16_t>;

__device__ __forceinline__ float st16_widen(f16_t s) { return (float) __builtin_bit_cast(_Float16, s.bits); }
__device__ __forceinline__ float st16_widen(bf16_t s) { return __builtin_bit_cast(float, (unsigned) s.bits << 16); }

template <typename S> __device__ __forceinline__ S st16_narrow(float x)
{
    if constexpr (std::is_same_v<S, f16_t>) return f16_t{__builtin_bit_cast(unsigned short, (_Float16) x)};
    else return bf16_t{__builtin_bit_cast(unsigned short, (__bf16) x)};
}

// 4 consecutive elements from an 8-byte aligned address: one 8-byte load
template <typename S> __device__ __forceinline__ void st16_load4(const S *p, float (&o)[4])
{
    static_assert(is_storage16<S>, "a 16-bit storage type");
    unsigned w[2];
    __builtin_memcpy(w, __builtin_assume_aligned(p, 8), 8);
    o[0] = st16_widen(S{(unsigned short) (w[0] & 0xffffu)});
    o[1] = st16_widen(S{(unsigned short) (w[0] >> 16)});
    o[2] = st16_widen(S{(unsigned short) (w[1] & 0xffffu)});
    o[3] = st16_widen(S{(unsigned short) (w[1] >> 16)});
}

// 4 consecutive elements to an 8-byte aligned address, each rounded once: one 8-byte store
template <typename S> __device__ __forceinline__ void st16_store4(S *p, const float (&a)[4])
{
    static_assert(is_storage16<S>, "a 16-bit storage type");
    unsigned w[2];
    w[0] = (unsigned) st16_narrow<S>(a[0]).bits | ((unsigned) st16_narrow<S>(a[1]).bits << 16);
    w[1] = (unsigned) st16_narrow<S>(a[2]).bits | ((unsigned) st16_narrow<S>(a[3]).bits << 16);
    __builtin_memcpy(__builtin_assume_aligned(p, 8), w, 8);
}

} // namespace spmv
