// MaxPool2d(3, 2, 1) on NHWC: the geometry and the winner rule that every pool kernel (pool.hip) and the fused stem tail
// (bn_train.hip) share.  The winner of a window is its FIRST maximum in row-major scan order (ATen's rule), recorded as the tap
// index 0..8; the backward passes gather: an input pixel collects dy of the <= 4 windows covering it whose winner it is.
#pragma once
#include "glue_common.h"

namespace vatl {

static inline int pool_out(int H) { return (H + 2 - 3) / 2 + 1; }

// input row / column of tap t = 0..2 of output row / column o, and the tap index of input pixel (iy, ix) inside window (oy, ox)
__device__ __forceinline__ int pool_in(int o, int t) { return 2 * o - 1 + t; }
__device__ __forceinline__ int pool_tap(int iy, int ix, int oy, int ox) { return (iy - pool_in(oy, 0)) * 3 + (ix - pool_in(ox, 0)); }

// one step of the scan over the taps k = 0..8 that lie inside the image, in order: does v take over from the best so far?  The
// first maximum wins (bk = winning tap so far, 255: none yet)
__device__ __forceinline__ bool pool_takes(float v, float best, int bk) { return v > best || bk == 255; }
__device__ __forceinline__ bool pool_takes(double v, double best, int bk) { return v > best || bk == 255; }

// gradient of input pixel (n, iy, ix), channels V*cv .. V*cv + V - 1: sum over the covering windows whose winner is this pixel.
// V = 4: float4 / uchar4 per window; V = 1: one channel (channel counts that are no multiple of 4).  Same sums, same order.
template <int V> using f32v = float __attribute__((ext_vector_type(V)));
template <int V>
__device__ __forceinline__ f32v<V> pool_gather(const float* __restrict__ dy, const uint8_t* __restrict__ idx, long long n, int iy, int ix, int cv,
                                               int Cv, int Ho, int Wo) {
    f32v<V> acc = 0.f;
    const int oy0 = iy >> 1, oy1 = (iy + 1) >> 1, ox0 = ix >> 1, ox1 = (ix + 1) >> 1;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int oy = a ? oy1 : oy0;
        if ((a && oy1 == oy0) || oy >= Ho) continue;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int ox = b ? ox1 : ox0;
            if ((b && ox1 == ox0) || ox >= Wo) continue;
            const long long o = ((n * Ho + oy) * Wo + ox) * Cv + cv;
            const unsigned kk = V == 4 ? *reinterpret_cast<const unsigned*>(idx + o * 4) : (unsigned)idx[o];
            const f32v<V> d = *reinterpret_cast<const f32v<V>*>(dy + o * V);
            const unsigned k = (unsigned)pool_tap(iy, ix, oy, ox);
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] += ((kk >> (8 * e)) & 255u) == k ? d[e] : 0.f;
        }
    }
    return acc;
}

}  // namespace vatl
