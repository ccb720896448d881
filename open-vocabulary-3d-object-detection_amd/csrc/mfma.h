// Fragment types and MFMA primitives shared by the matrix kernels (gfx950 / CDNA4, wave64).
// Only what compiles to the same code wherever it is used lives here: the vector typedefs, the
// matrix builtins, the transposed LDS read, the operand join.  LDS addressing, swizzles, staging
// and K-loops stay with the kernel that tuned them ("Shared device headers").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16;
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint8_t u8x8 __attribute__((ext_vector_type(8)));

// 32x32x16 bf16: a lane holds 8 k-values of one row (A) / column (B), 16 accumulators
__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// 16x16x32 bf16: 4 accumulators; the i32x4 form takes fragments as ds_read_b128 delivers them
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(i32x4 a, i32x4 b, f32x4 c) {
    return mfma16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c);
}

// ds_read_b64_tr_b16: 4 bf16 of the transposed 16 x 16 block that the 16 lanes' pointers name
__device__ __forceinline__ bf16x4 tr16(const bf16* p) {
    s16x4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
    return __builtin_bit_cast(bf16x4, r);
}

// the two 4-element halves of an 8-element operand
__device__ __forceinline__ bf16x8 join8(bf16x4 lo, bf16x4 hi) {
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// two fp32 -> two bf16 in one dword (one v_cvt_pk_bf16_f32), a in the low half
__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){a, b}, bf16x2));
}

// ---- buffer / LDS-DMA (gemm256.hip, rows256.hip) ----

// raw buffer resource over [base, base + bytes), clamped to 2 GB: offsets past it load 0
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, long long bytes) {
    const uint32_t n = bytes > 0x7fffffffLL ? 0x7fffffffu : (uint32_t)(bytes > 0 ? bytes : 0);
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)n, 0x00020000);
}
// wait for the asm LDS reads (the kernels' lds128) that produced a[0..7]; naming them as
// in-out operands keeps their uses behind the wait
__device__ __forceinline__ void lgkm_wait8(i32x4 (&a)[8]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]),
                   "+v"(a[6]), "+v"(a[7])
                 :
                 : "memory");
}
