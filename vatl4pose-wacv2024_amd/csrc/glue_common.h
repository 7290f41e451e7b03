// What the HBM-bound glue kernels around the convolutions share (layout.hip, pack.hip, pool.hip, fusion.hip, bn_train.hip): each
// formula below exists once, so that the passes that must agree bit for bit — the ReLU masks of forward and backward, the winner
// rule of the max-pool (pool.h) — cannot drift apart.
#pragma once
#include "common.h"

namespace vatl {

// grid of the element-wise kernels: 256 threads per block, at most 4096 blocks (their loops stride over the grid)
static inline int ew_grid(long long n) { long long g = (n + 255) / 256; if (g > 4096) g = 4096; if (g < 1) g = 1; return (int)g; }

// ReLU backward: v where the rectified output y was positive
__device__ __forceinline__ float relu_mask(float y, float v) { return y > 0.f ? v : 0.f; }
__device__ __forceinline__ f32x4 relu_mask(f32x4 y, f32x4 v) {
    v[0] = relu_mask(y[0], v[0]); v[1] = relu_mask(y[1], v[1]); v[2] = relu_mask(y[2], v[2]); v[3] = relu_mask(y[3], v[3]);
    return v;
}
// ... of a layer without a skip input, recomputed from z exactly as scale_bias_act_kernel produced y (same fmaf): no read of y
__device__ __forceinline__ bool relu_on(float z, float sc, float bi) { return fmaf(z, sc, bi) > 0.f; }
__device__ __forceinline__ f32x4 relu_mask(f32x4 z, f32x4 sc, f32x4 bi, f32x4 v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = relu_on(z[e], sc[e], bi[e]) ? v[e] : 0.f;
    return v;
}

__device__ __forceinline__ float sigmoidf(float g) { return 1.f / (1.f + expf(-g)); }
// finish of the SE gate gradient: sum_hw (dy*[y>0]*u) times sigmoid'(gate)
__device__ __forceinline__ float se_gate_grad(float sum, float gate) { const float sg = sigmoidf(gate); return sum * sg * (1.f - sg); }

// flat index of an (N, H, W, C4) tensor -> (n, y, x, c4), the channel group fastest
struct Nyxc { long long n; int y, x, c4; };
__device__ __forceinline__ Nyxc nyxc(long long i, int H, int W, int C4) {
    Nyxc p;
    p.c4 = (int)(i % C4);
    long long t = i / C4;
    p.x = (int)(t % W); t /= W;
    p.y = (int)(t % H);
    p.n = t / H;
    return p;
}

// Column reductions of the bf16 and float64 training glue (train_glue_h16.hip, train_glue_f64.hip): a block owns kRowsPerBlock consecutive
// rows and writes partial[(rb * C + c) * 2 + {0, 1}] in double
constexpr int kRowsPerBlock = 512;
static inline int tg_row_blocks(long long M) { return (int)((M + kRowsPerBlock - 1) / kRowsPerBlock); }
// ... and a wave per channel sums them: lane l adds the row blocks l, l + 64, ... in ascending order, then the fixed xor tree
__device__ __forceinline__ void tg_sum_partials(const double* __restrict__ partial, int nrb, int C, int c, int lane, double& s, double& q) {
    s = 0.0;
    q = 0.0;
    if (c < C)
        for (int rb = lane; rb < nrb; rb += 64) { s += partial[((long long)rb * C + c) * 2]; q += partial[((long long)rb * C + c) * 2 + 1]; }
    s = wave_sum(s);
    q = wave_sum(q);
}

// pool.hip's per-item pixel reductions of small batches (mode 0: average pool, 1: SE gate gradient); false = not one of their shapes
__attribute__((visibility("hidden"))) bool hw_reduce_try(int mode, const float* a, const float* y, const float* u, const float* gate, float* out, int N, int HW,
                                                         int C, hipStream_t st);

}  // namespace vatl
