// Pieces that more than one scorer family uses (decode.hip, localpeak.hip, heatmap_criteria.hip, pose_feature.hip): one copy each.
// A piece that a single family uses sits at the top of that family's file.
#pragma once
#include "common.h"

namespace vatl {

// --------------------------------------------------------------------------
// wave-per-plane route: a plane of exactly 64 * NV float4 (64x48 -> NV = 12, 96x72 -> NV = 27) at a 16-byte aligned base is held in
// registers by ONE wave (NV float4 per lane, every load in flight at once, no LDS, no block barrier); four planes per 256-thread block
// --------------------------------------------------------------------------
// NV of the wave route, 0 = take the block kernel.  The wave kernels take the plane count as an int.
static inline int wave_route_nv(const float* hm, long long planes, int H, int W) {
    if ((((uintptr_t)hm) & 15) != 0 || planes > 0x7FFFFFFF) return 0;
    return H * W == 64 * 12 * 4 ? 12 : (H * W == 64 * 27 * 4 ? 27 : 0);
}

__device__ __forceinline__ long long wave_plane() { return (long long)blockIdx.x * 4 + (threadIdx.x >> 6); }

// lane's share of the plane: float4 number k * 64 + lane, k = 0 .. NV - 1 (element 4 * (k * 64 + lane) + e)
template <int NV>
__device__ __forceinline__ void load_plane(const float* src, int lane, f32x4 (&v)[NV]) {
    const f32x4* src4 = reinterpret_cast<const f32x4*>(src) + lane;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = src4[k * 64];
}

// --------------------------------------------------------------------------
// four-wave (256-thread) block combines.  The kernel owns the 4-entry LDS array and the barrier:
//     v = wave_sum(v);  block4_put(sh, v);  __syncthreads();  total = block4_sum(sh);
// so that several values share one barrier and a kernel whose thread 0 alone needs the result can leave before the reads.
// --------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void block4_put(T* sh, T wave_value) {
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = wave_value;
}
__device__ __forceinline__ float block4_max(const float* sh) { return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3])); }
__device__ __forceinline__ double block4_sum(const double* sh) { return sh[0] + sh[1] + sh[2] + sh[3]; }
__device__ __forceinline__ int block4_sum(const int* sh) { return sh[0] + sh[1] + sh[2] + sh[3]; }

// --------------------------------------------------------------------------
// (value, index) arg-max: larger value first, equal values by lower index.  Two rules for NaN, on purpose:
//   NAN_IS_MAX = true   np.argmax on a raw heat-map plane (decode): NaN is the maximum and the FIRST NaN wins.
//   NAN_IS_MAX = false  candidate lists of peaks5, whose entries are plane values that passed `v == window max && v > plane min`
//                       or -inf: a NaN never gets in, -inf entries never win, so the rule is the plain ordering and costs
//                       three comparisons less per merge.
// --------------------------------------------------------------------------
template <bool NAN_IS_MAX>
__device__ __forceinline__ void argmax_merge(float& v, int& i, float ov, int oi) {
    if (NAN_IS_MAX) {
        if (ov > v || (ov == v && oi < i) || (ov != ov && (v == v || oi < i))) { v = ov; i = oi; }
    } else {
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

template <bool NAN_IS_MAX>
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        argmax_merge<NAN_IS_MAX>(v, i, ov, oi);
    }
}

// after wave_argmax, block4_put of value and index and a barrier
template <bool NAN_IS_MAX>
__device__ __forceinline__ void block4_argmax(const float* sv, const int* si, float& v, int& i) {
    v = sv[0]; i = si[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) argmax_merge<NAN_IS_MAX>(v, i, sv[w], si[w]);
}

}  // namespace vatl
