// Element-wise block tails on NHWC: the SE gate (forward and both backward stages), HRNet's up-sample-and-add fusion with its
// backward, and the plain ReLU backward.
#include "glue_common.h"

namespace vatl {

// SE gate + residual + ReLU: y = relu(x * sigmoid(g[b][c]) + res)   (SE_module.py:20-24, SE_Resnet.py:125-135)
__global__ void se_scale_add_relu_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ res,
                                         float* __restrict__ y, int N, int HW, int C) {
    const int C4 = C >> 2;
    const long long total = (long long)N * HW * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        const long long n = i / ((long long)HW * C4);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + n * C + c4 * 4);
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + i * 4);
        const f32x4 rv = *reinterpret_cast<const f32x4*>(res + i * 4);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaxf(xv[e] * sigmoidf(gv[e]) + rv[e], 0.f);
        *reinterpret_cast<f32x4*>(y + i * 4) = o;
    }
}

// SE block backward, stage 1 (per item and channel): gm = dy*[y>0];  dgate[n][c] = sig'(g) * sum_hw gm*u.  Large batches; small
// ones take pool.hip's hw_reduce_kernel<1>, which sums in another order.
__global__ void se_bwd_gate_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ u,
                                   const float* __restrict__ gate, float* __restrict__ dgate, int N, int HW, int C) {
    const long long total = (long long)N * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / C;
        const int c = (int)(i - n * C);
        const long long base = n * HW * C + c;
        float s = 0.f;
        for (int k = 0; k < HW; ++k) {
            const long long o = base + (long long)k * C;
            if (y[o] > 0.f) s += dy[o] * u[o];
        }
        dgate[i] = se_gate_grad(s, gate[i]);
    }
}

// SE block backward, stage 2: gm = dy*[y>0] (gradient of the shortcut), du = gm*sigmoid(g) + dpool[n][c]/HW
__global__ void se_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ gate,
                                    const float* __restrict__ dpool, float* __restrict__ du, float* __restrict__ gm, int N, int HW, int C) {
    const int C4 = C >> 2;
    const long long total = (long long)N * HW * C4;
    const float inv = 1.f / (float)HW;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        const long long n = i / ((long long)HW * C4);
        const f32x4 g = *reinterpret_cast<const f32x4*>(gate + n * C + c4 * 4);
        const f32x4 dp = *reinterpret_cast<const f32x4*>(dpool + n * C + c4 * 4);
        const f32x4 d = *reinterpret_cast<const f32x4*>(dy + i * 4);
        const f32x4 yy = *reinterpret_cast<const f32x4*>(y + i * 4);
        f32x4 o, m;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            m[e] = relu_mask(yy[e], d[e]);
            o[e] = m[e] * sigmoidf(g[e]) + dp[e] * inv;
        }
        *reinterpret_cast<f32x4*>(du + i * 4) = o;
        *reinterpret_cast<f32x4*>(gm + i * 4) = m;
    }
}

// HRNet fuse: y = act(base + sum_k nearest_up(z_k, 2^shift_k)); up to 3 low-resolution sources (hrnet.py:242-260)
struct FuseUpArgs { const float* z[3]; int shift[3]; int n; };
__global__ void fuse_up_kernel(const float* __restrict__ base, FuseUpArgs a, float* __restrict__ y, int N, int H, int W, int C, int relu) {
    const int C4 = C >> 2;
    const long long total = (long long)N * H * W * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc p = nyxc(i, H, W, C4);
        f32x4 v = *reinterpret_cast<const f32x4*>(base + i * 4);
        for (int k = 0; k < a.n; ++k) {
            const int s = a.shift[k];
            const int h2 = H >> s, w2 = W >> s;
            const f32x4 z = *reinterpret_cast<const f32x4*>(a.z[k] + (((p.n * h2 + (p.y >> s)) * w2 + (p.x >> s)) * C4 + p.c4) * 4);
            v[0] += z[0]; v[1] += z[1]; v[2] += z[2]; v[3] += z[3];
        }
        if (relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
        *reinterpret_cast<f32x4*>(y + i * 4) = v;
    }
}

// backward of the nearest up-sampling inside the HRNet fusion: dz[n][y][x][c] = sum over the 2^s x 2^s block of
// g = dy * [yact > 0] (yact = the fused, rectified output; NULL = no mask)
__global__ void upsample_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ yact, float* __restrict__ dz, int N, int H, int W,
                                    int C, int s) {
    const int C4 = C >> 2, h2 = H >> s, w2 = W >> s, f = 1 << s;
    const long long total = (long long)N * h2 * w2 * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc p = nyxc(i, h2, w2, C4);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int a = 0; a < f; ++a)
            for (int b = 0; b < f; ++b) {
                const long long o = (((p.n * H + (p.y * f + a)) * W + (p.x * f + b)) * C4 + p.c4) * 4;
                f32x4 g = *reinterpret_cast<const f32x4*>(dy + o);
                if (yact) g = relu_mask(*reinterpret_cast<const f32x4*>(yact + o), g);
                acc[0] += g[0]; acc[1] += g[1]; acc[2] += g[2]; acc[3] += g[3];
            }
        *reinterpret_cast<f32x4*>(dz + i * 4) = acc;
    }
}

// dx = dy * [y > 0]   (ReLU backward on a flat fp32 span)
__global__ void relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dx, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dx[i] = y[i] > 0.f ? dy[i] : 0.f;      // relu_mask() spelled out: as an argument dy[i] would be loaded where y <= 0 too, and the loop unrolled around that
}

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_se_scale_add_relu(const float* x, const float* gate, const float* residual, float* y, int N, int HW, int C, void* stream) {
    if (!x || !gate || !residual || !y || (C & 3)) return fail(VATL_EINVAL, "se_scale_add_relu: bad arguments");
    hipLaunchKernelGGL(se_scale_add_relu_kernel, dim3(ew_grid((long long)N * HW * (C / 4))), dim3(256), 0, (hipStream_t)stream, x, gate, residual, y, N, HW, C);
    return check_launch("se_scale_add_relu");
}

extern "C" int vatl_se_bwd(const float* dy, const float* y, const float* u, const float* gate, const float* dpool_or_null,
                           float* dgate_or_null, float* du_or_null, float* gm_or_null, int N, int HW, int C, void* stream) {
    if (!dy || !y || !gate || (C & 3)) return fail(VATL_EINVAL, "se_bwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (dgate_or_null) {
        if (!u) return fail(VATL_EINVAL, "se_bwd: stage 1 needs u");
        if (!hw_reduce_try(1, dy, y, u, gate, dgate_or_null, N, HW, C, st))
            hipLaunchKernelGGL(se_bwd_gate_kernel, dim3(ew_grid((long long)N * C)), dim3(256), 0, st, dy, y, u, gate, dgate_or_null, N, HW, C);
    }
    if (du_or_null) {
        if (!dpool_or_null || !gm_or_null) return fail(VATL_EINVAL, "se_bwd: stage 2 needs dpool and gm");
        hipLaunchKernelGGL(se_bwd_apply_kernel, dim3(ew_grid((long long)N * HW * (C / 4))), dim3(256), 0, st, dy, y, gate, dpool_or_null, du_or_null, gm_or_null, N, HW, C);
    }
    return check_launch("se_bwd");
}

extern "C" int vatl_fuse_upsample_add(const float* base, const float* z0, int shift0, const float* z1, int shift1, const float* z2, int shift2,
                                      float* y, int N, int H, int W, int C, int relu, void* stream) {
    if (!base || !y || (C & 3)) return fail(VATL_EINVAL, "fuse_upsample_add: bad arguments");
    FuseUpArgs a{};
    const float* zs[3] = {z0, z1, z2};
    const int sh[3] = {shift0, shift1, shift2};
    for (int k = 0; k < 3; ++k) {
        if (!zs[k]) continue;
        if (sh[k] < 1 || (H & ((1 << sh[k]) - 1)) || (W & ((1 << sh[k]) - 1)))
            return fail(VATL_EINVAL, "fuse_upsample_add: %dx%d is not divisible by 2^%d", H, W, sh[k]);
        a.z[a.n] = zs[k]; a.shift[a.n] = sh[k]; ++a.n;
    }
    hipLaunchKernelGGL(fuse_up_kernel, dim3(ew_grid((long long)N * H * W * (C / 4))), dim3(256), 0, (hipStream_t)stream, base, a, y, N, H, W, C, relu);
    return check_launch("fuse_upsample_add");
}

extern "C" int vatl_upsample_nearest_bwd(const float* dy, const float* yact_or_null, float* dz, int N, int H, int W, int C, int shift, void* stream) {
    if (!dy || !dz || (C & 3)) return fail(VATL_EINVAL, "upsample_nearest_bwd: bad arguments");
    if (shift < 1 || shift > 5 || (H & ((1 << shift) - 1)) || (W & ((1 << shift) - 1)))
        return fail(VATL_EINVAL, "upsample_nearest_bwd: %dx%d is not divisible by 2^%d", H, W, shift);
    if (N <= 0) return 0;
    hipLaunchKernelGGL(upsample_bwd_kernel, dim3(ew_grid((long long)N * (H >> shift) * (W >> shift) * (C / 4))), dim3(256), 0, (hipStream_t)stream,
                       dy, yact_or_null, dz, N, H, W, C, shift);
    return check_launch("upsample_nearest_bwd");
}

extern "C" int vatl_relu_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream) {
    if (!dy || !y || !dx) return fail(VATL_EINVAL, "relu_bwd: null pointer");
    if (n <= 0) return 0;
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, dy, y, dx, (long long)n);
    return check_launch("relu_bwd");
}
