// The two 16-bit storage types of the opt-in h16 inference route (conv_h16.hip, glue_h16.hip): what differs between float16 and
// bfloat16 — the conversions and the MFMA builtin — and nothing else.  fp32 -> T is round-to-nearest-even with IEEE overflow to
// infinity (no saturation), as tensor.to(torch.float16 / torch.bfloat16) rounds; T -> fp32 is exact.
#pragma once
#include "common.h"

namespace vatl {

typedef float h16_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned h16_u32x4 __attribute__((ext_vector_type(4)));     // eight T as the MFMA and the LDS move them
typedef _Float16 h16_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 h16_bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kH16F16 = 0, kH16BF16 = 1;       // the `dtype` argument of every vatl_*_h16 entry point

struct F16 {
    static __device__ __forceinline__ unsigned short from_f32(float f) {
        const _Float16 h = (_Float16)f;          // v_cvt_f16_f32: round to nearest even, overflow -> inf
        return __builtin_bit_cast(unsigned short, h);
    }
    static __device__ __forceinline__ float to_f32(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
    static __device__ __forceinline__ h16_f32x4 mfma(h16_u32x4 a, h16_u32x4 b, h16_f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16_f16x8, a), __builtin_bit_cast(h16_f16x8, b), c, 0, 0, 0);
    }
};

struct BF16 {
    static __device__ __forceinline__ unsigned short from_f32(float f) {
        unsigned u = __builtin_bit_cast(unsigned, f);
        if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (unsigned short)((u >> 16) | 0x0040u);      // NaN stays NaN (quiet)
        u += 0x7FFFu + ((u >> 16) & 1u);         // round to nearest even on the 16 dropped bits; a carry out of the exponent gives inf
        return (unsigned short)(u >> 16);
    }
    static __device__ __forceinline__ float to_f32(unsigned short b) { return __builtin_bit_cast(float, (unsigned)b << 16); }
    static __device__ __forceinline__ h16_f32x4 mfma(h16_u32x4 a, h16_u32x4 b, h16_f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(h16_bf16x8, a), __builtin_bit_cast(h16_bf16x8, b), c, 0, 0, 0);
    }
};

// eight T in one 16-byte word <-> eight floats
template <typename T>
__device__ __forceinline__ void h16_unpack8(uint4 v, float* f) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[2 * j] = T::to_f32((unsigned short)(w[j] & 0xFFFFu));
        f[2 * j + 1] = T::to_f32((unsigned short)(w[j] >> 16));
    }
}
template <typename T>
__device__ __forceinline__ uint4 h16_pack8(const float* f) {
    unsigned w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = (unsigned)T::from_f32(f[2 * j]) | ((unsigned)T::from_f32(f[2 * j + 1]) << 16);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

static inline bool h16_dtype_ok(int dtype) { return dtype == kH16F16 || dtype == kH16BF16; }
static inline bool h16_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace vatl
