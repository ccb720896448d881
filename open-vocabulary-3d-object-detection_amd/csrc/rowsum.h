// Helpers of the channels-last row kernels (bnrows.hip, resnorm.hip, lngemm.hip, encpost.hip): a
// lane's 8 channels to and from memory (ld8f, st8f, st8h, pack8), and the row sum over 32 lanes
// (a 256-channel row at 8 channels a lane) of the LayerNorm row kernels (resnorm.hip,
// lngemm.hip, encpost.hip).  The xor butterfly in ascending order (1, 2, 4, 8, 16)
// on VALU lane moves: quad permutes for 1 and 2, the 8- / 16-lane mirrors for 4 and 8 (equal
// to the xor partner once the value is uniform over the smaller group), v_permlane16_swap for
// 16.  Every lane ends with the same sum (IEEE addition is commutative); the moves cost a few
// cycles each where a ds_bpermute / ds_swizzle round trip through the LDS pipe costs ~100.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma.h"

// 8 consecutive channels of a row: fp32 as two 16-byte pieces, bf16 as one (one rounding)
__device__ __forceinline__ void ld8f(const float* p, float* v) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void st8f(float* p, const float* v) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ void st8f(float* p, long long off, const float* v) { st8f(p + off, v); }
__device__ __forceinline__ bf16x8 pack8(const float* v) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16)v[j];
    return o;
}
__device__ __forceinline__ void st8h(bf16* p, long long off, const float* v) {
    *reinterpret_cast<bf16x8*>(p + off) = pack8(v);
}

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF,
                                                              0xF, true));
}

__device__ __forceinline__ float row_sum32_lanes(float v) {
    v += dpp_mov<0xB1>(v);    // quad_perm(1, 0, 3, 2): lane ^ 1
    v += dpp_mov<0x4E>(v);    // quad_perm(2, 3, 0, 1): lane ^ 2
    v += dpp_mov<0x141>(v);   // row_half_mirror: the other quad of the 8
    v += dpp_mov<0x140>(v);   // row_mirror: the other 8 of the 16
    const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(uint32_t, v),
                                                    __builtin_bit_cast(uint32_t, v), false, false);
    return __builtin_bit_cast(float, (uint32_t)r[0]) + __builtin_bit_cast(float, (uint32_t)r[1]);
}
