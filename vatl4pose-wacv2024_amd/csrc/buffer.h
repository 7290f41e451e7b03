// One spelling of raw buffer access for the matrix-core kernels (gfx950).
#pragma once
#include "common.h"

namespace vatl {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;          // destination of buffer_load ... lds (LDS-DMA)

// Word 3 of the buffer descriptor: DATA_FORMAT (bits 15-18) = 4 = 32-bit, every other field zero — no swizzle, no index stride,
// identity destination select.  With stride 0 this is a raw buffer: the hardware checks offset + access size against `bytes`
// (out-of-range loads read 0, LDS-DMA loads write 0, stores are dropped).  The value cdna_hip_programming.md's recipes use for gfx9 / CDNA.
constexpr int kBufRsrcFlags = 0x00020000;

// Descriptor of `bytes` bytes at p.  Build it from wave-uniform values only.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, kBufRsrcFlags);
}

__device__ __forceinline__ f32x4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0));
}
__device__ __forceinline__ void buf_store4(__amdgpu_buffer_rsrc_t r, unsigned byte_off, f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, byte_off, 0, 0);
}
__device__ __forceinline__ float buf_load1(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
}
__device__ __forceinline__ void buf_store1(__amdgpu_buffer_rsrc_t r, unsigned byte_off, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, byte_off, 0, 0);
}

}  // namespace vatl
