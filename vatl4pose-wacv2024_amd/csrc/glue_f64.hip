// Float64 glue of the device reference forward (csrc/conv_f64.hip): what sits between the convolutions of the three pose networks,
// restated for NHWC float64 tensors with ANY channel count — layout changes at the ends, MaxPool2d(3,2,1), the global average pool,
// PixelShuffle(2), the SE gate with skip and ReLU, HRNet's nearest up-sampling + add.  One thread per output element; every sum has
// one fixed order (pixels ascending, sources in argument order).  The fp32 kernels of layout.hip / pool.hip / fusion.hip are not
// touched: their bits are pinned.
#include "glue_common.h"
#include "pool.h"

namespace vatl {

// NCHW (fp32 or float64) -> NHWC float64; the conversion from fp32 is exact
template <typename T>
__global__ void nchw_to_nhwc_f64_kernel(const T* __restrict__ src, double* __restrict__ dst, long long N, int C, int HW) {
    const long long total = N * HW * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long long pix = i / C;
        const long long n = pix / HW;
        const int px = (int)(pix - n * HW);
        dst[i] = (double)src[(n * C + c) * HW + px];
    }
}

__global__ void nhwc_to_nchw_f64_kernel(const double* __restrict__ src, double* __restrict__ dst, long long N, int C, int HW) {
    const long long total = N * C * HW;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int px = (int)(i % HW);
        const long long nc = i / HW;
        const int c = (int)(nc % C);
        const long long n = nc / C;
        dst[i] = src[(n * HW + px) * C + c];
    }
}

// MaxPool2d(3, 2, 1): padding behaves as -inf (window geometry: pool.h)
__global__ void maxpool3x3s2_f64_kernel(const double* __restrict__ x, double* __restrict__ y, long long N, int H, int W, int C, int Ho, int Wo) {
    const long long total = N * Ho * Wo * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc o = nyxc(i, Ho, Wo, C);
        double m = -INFINITY;
        for (int dy = 0; dy < 3; ++dy) {
            const int iy = pool_in(o.y, dy);
            if ((unsigned)iy >= (unsigned)H) continue;
            for (int dx = 0; dx < 3; ++dx) {
                const int ix = pool_in(o.x, dx);
                if ((unsigned)ix >= (unsigned)W) continue;
                m = fmax(m, x[((o.n * H + iy) * W + ix) * C + o.c4]);
            }
        }
        y[i] = m;
    }
}

// global average pool: thread per (n, c), pixels in order, one division
__global__ void gap_f64_kernel(const double* __restrict__ x, double* __restrict__ y, long long N, int HW, int C) {
    const long long total = N * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / C;
        const int c = (int)(i - n * C);
        const double* p = x + n * HW * C + c;
        double s = 0.0;
        for (int k = 0; k < HW; ++k) s += p[(long long)k * C];
        y[i] = s / (double)HW;
    }
}

// PixelShuffle(2) on NHWC: out[b][2y+i][2x+j][c] = in[b][y][x][4c + 2i + j]; thread per input element
__global__ void pixelshuffle2_f64_kernel(const double* __restrict__ x, double* __restrict__ y, long long N, int H, int W, int C) {
    const int Co = C >> 2;
    const long long total = N * H * W * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc p = nyxc(i, H, W, C);
        const int c = p.c4 >> 2, di = (p.c4 >> 1) & 1, dj = p.c4 & 1;
        y[((p.n * 2 * H + 2 * p.y + di) * 2 * W + 2 * p.x + dj) * Co + c] = x[i];
    }
}

// SE gate + skip + ReLU: y = relu(x * sigmoid(g[n][c]) + res), g the pre-sigmoid output of the second Linear
__global__ void se_scale_add_relu_f64_kernel(const double* __restrict__ x, const double* __restrict__ g, const double* __restrict__ res,
                                             double* __restrict__ y, long long N, int HW, int C) {
    const long long total = N * HW * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long long n = i / ((long long)HW * C);
        const double sg = 1.0 / (1.0 + exp(-g[n * C + c]));
        y[i] = fmax(x[i] * sg + res[i], 0.0);
    }
}

// HRNet fuse: y = act(base + sum_k nearest_up(z_k, 2^shift_k)), sources added in argument order
struct FuseUpF64Args { const double* z[3]; int shift[3]; int n; };
__global__ void fuse_up_f64_kernel(const double* __restrict__ base, FuseUpF64Args a, double* __restrict__ y, long long N, int H, int W, int C, int relu) {
    const long long total = N * H * W * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc p = nyxc(i, H, W, C);
        double v = base[i];
        for (int k = 0; k < a.n; ++k) {
            const int s = a.shift[k];
            const int h2 = H >> s, w2 = W >> s;
            v += a.z[k][((p.n * h2 + (p.y >> s)) * w2 + (p.x >> s)) * C + p.c4];
        }
        y[i] = relu ? fmax(v, 0.0) : v;
    }
}

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_nchw_to_nhwc_f64(const void* src, int src_is_f64, double* dst, int N, int C, int H, int W, void* stream) {
    if (!src || !dst || N < 0 || C < 1 || H < 1 || W < 1) return fail(VATL_EINVAL, "nchw_to_nhwc_f64: bad arguments");
    if (N == 0) return 0;
    const int grid = ew_grid((long long)N * C * H * W);
    if (src_is_f64)
        hipLaunchKernelGGL(nchw_to_nhwc_f64_kernel<double>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const double*)src, dst, (long long)N, C, H * W);
    else
        hipLaunchKernelGGL(nchw_to_nhwc_f64_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)src, dst, (long long)N, C, H * W);
    return check_launch("nchw_to_nhwc_f64");
}

extern "C" int vatl_nhwc_to_nchw_f64(const double* src, double* dst, int N, int C, int H, int W, void* stream) {
    if (!src || !dst || N < 0 || C < 1 || H < 1 || W < 1) return fail(VATL_EINVAL, "nhwc_to_nchw_f64: bad arguments");
    if (N == 0) return 0;
    hipLaunchKernelGGL(nhwc_to_nchw_f64_kernel, dim3(ew_grid((long long)N * C * H * W)), dim3(256), 0, (hipStream_t)stream, src, dst, (long long)N, C, H * W);
    return check_launch("nhwc_to_nchw_f64");
}

extern "C" int vatl_maxpool3x3s2_fwd_f64(const double* x, double* y, int N, int H, int W, int C, void* stream) {
    if (!x || !y || N < 0 || C < 1 || H < 1 || W < 1) return fail(VATL_EINVAL, "maxpool3x3s2_fwd_f64: bad arguments");
    if (N == 0) return 0;
    const int Ho = pool_out(H), Wo = pool_out(W);
    hipLaunchKernelGGL(maxpool3x3s2_f64_kernel, dim3(ew_grid((long long)N * Ho * Wo * C)), dim3(256), 0, (hipStream_t)stream, x, y, (long long)N, H, W, C, Ho, Wo);
    return check_launch("maxpool3x3s2_fwd_f64");
}

extern "C" int vatl_gap_fwd_f64(const double* x, double* y, int N, int HW, int C, void* stream) {
    if (!x || !y || N < 0 || C < 1 || HW < 1) return fail(VATL_EINVAL, "gap_fwd_f64: bad arguments");
    if (N == 0) return 0;
    hipLaunchKernelGGL(gap_f64_kernel, dim3(ew_grid((long long)N * C)), dim3(256), 0, (hipStream_t)stream, x, y, (long long)N, HW, C);
    return check_launch("gap_fwd_f64");
}

extern "C" int vatl_pixelshuffle2_fwd_f64(const double* x, double* y, int N, int H, int W, int C, void* stream) {
    if (!x || !y || N < 0 || C < 4 || (C & 3) || H < 1 || W < 1) return fail(VATL_EINVAL, "pixelshuffle2_fwd_f64: C %d must be a multiple of 4", C);
    if (N == 0) return 0;
    hipLaunchKernelGGL(pixelshuffle2_f64_kernel, dim3(ew_grid((long long)N * H * W * C)), dim3(256), 0, (hipStream_t)stream, x, y, (long long)N, H, W, C);
    return check_launch("pixelshuffle2_fwd_f64");
}

extern "C" int vatl_se_scale_add_relu_f64(const double* x, const double* gate, const double* residual, double* y, int N, int HW, int C, void* stream) {
    if (!x || !gate || !residual || !y || N < 0 || C < 1 || HW < 1) return fail(VATL_EINVAL, "se_scale_add_relu_f64: bad arguments");
    if (N == 0) return 0;
    hipLaunchKernelGGL(se_scale_add_relu_f64_kernel, dim3(ew_grid((long long)N * HW * C)), dim3(256), 0, (hipStream_t)stream, x, gate, residual, y, (long long)N, HW, C);
    return check_launch("se_scale_add_relu_f64");
}

extern "C" int vatl_fuse_upsample_add_f64(const double* base, const double* z0, int shift0, const double* z1, int shift1, const double* z2, int shift2,
                                          double* y, int N, int H, int W, int C, int relu, void* stream) {
    if (!base || !y || N < 0 || C < 1 || H < 1 || W < 1) return fail(VATL_EINVAL, "fuse_upsample_add_f64: bad arguments");
    FuseUpF64Args a{};
    const double* zs[3] = {z0, z1, z2};
    const int sh[3] = {shift0, shift1, shift2};
    for (int k = 0; k < 3; ++k) {
        if (!zs[k]) continue;
        if (sh[k] < 1 || sh[k] > 5 || (H & ((1 << sh[k]) - 1)) || (W & ((1 << sh[k]) - 1)))
            return fail(VATL_EINVAL, "fuse_upsample_add_f64: %dx%d is not divisible by 2^%d", H, W, sh[k]);
        a.z[a.n] = zs[k]; a.shift[a.n] = sh[k]; ++a.n;
    }
    if (N == 0) return 0;
    hipLaunchKernelGGL(fuse_up_f64_kernel, dim3(ew_grid((long long)N * H * W * C)), dim3(256), 0, (hipStream_t)stream, base, a, y, (long long)N, H, W, C, relu);
    return check_launch("fuse_upsample_add_f64");
}
