// Glue of the opt-in 16-bit inference route (csrc/conv_h16.hip): what sits between the convolutions of the three pose networks, for
// NHWC tensors of a storage type T in {float16, bfloat16} whose channel count is a multiple of 8 — a thread moves eight channels as
// one 16-byte word.  Layout changes at the ends (fp32 NCHW in, with the channels padded to 8 by zeros; fp32 NCHW out), MaxPool2d(3,2,1),
// the global average pool (fp32 out), PixelShuffle(2), the SE gate with skip and ReLU (gate in fp32), HRNet's nearest up-sampling +
// add.  Every sum is taken in fp32 in one fixed order (pixels ascending, sources in argument order) and rounded ONCE to T.  The list
// and the argument order are glue_f64.hip's; the fp32 kernels of layout.hip / pool.hip / fusion.hip are not touched.
#include "glue_common.h"
#include "h16.h"
#include "pool.h"

namespace vatl {

// (N,C,H,W) fp32 -> (N,H,W,C8) T: thread per (pixel, group of eight channels), channels >= C are exact zeros
template <typename T>
__global__ void nchw_to_nhwc_h16_kernel(const float* __restrict__ src, uint4* __restrict__ dst, long long N, int C, int C8, int HW) {
    const int G = C8 >> 3;
    const long long total = N * HW * G;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int gq = (int)(i % G);
        const long long pix = i / G;
        const long long n = pix / HW;
        const int px = (int)(pix - n * HW);
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = 8 * gq + j;
            f[j] = c < C ? src[(n * C + c) * HW + px] : 0.f;
        }
        dst[i] = h16_pack8<T>(f);
    }
}

// (N,H,W,C) T -> (N,C,H,W) fp32 (exact): thread per output element
template <typename T>
__global__ void nhwc_to_nchw_h16_kernel(const unsigned short* __restrict__ src, float* __restrict__ dst, long long N, int C, int HW) {
    const long long total = N * C * HW;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int px = (int)(i % HW);
        const long long nc = i / HW;
        const int c = (int)(nc % C);
        const long long n = nc / C;
        dst[i] = T::to_f32(src[(n * HW + px) * C + c]);
    }
}

// MaxPool2d(3, 2, 1): padding behaves as -inf (window geometry: pool.h); the maximum of T values is a T value
template <typename T>
__global__ void maxpool3x3s2_h16_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, long long N, int H, int W, int G, int Ho, int Wo) {
    const long long total = N * Ho * Wo * G;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc o = nyxc(i, Ho, Wo, G);
        float m[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
        for (int dy = 0; dy < 3; ++dy) {
            const int iy = pool_in(o.y, dy);
            if ((unsigned)iy >= (unsigned)H) continue;
            for (int dx = 0; dx < 3; ++dx) {
                const int ix = pool_in(o.x, dx);
                if ((unsigned)ix >= (unsigned)W) continue;
                float f[8];
                h16_unpack8<T>(x[((o.n * H + iy) * W + ix) * G + o.c4], f);
#pragma unroll
                for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], f[j]);
            }
        }
        y[i] = h16_pack8<T>(m);
    }
}

// global average pool -> fp32: thread per (n, c), pixels summed in fp32 in order, one division
template <typename T>
__global__ void gap_h16_kernel(const unsigned short* __restrict__ x, float* __restrict__ y, long long N, int HW, int C) {
    const long long total = N * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / C;
        const int c = (int)(i - n * C);
        const unsigned short* p = x + n * HW * C + c;
        float s = 0.f;
        for (int k = 0; k < HW; ++k) s += T::to_f32(p[(long long)k * C]);
        y[i] = s / (float)HW;
    }
}

// PixelShuffle(2) on NHWC: out[b][2y+i][2x+j][c] = in[b][y][x][4c + 2i + j]; a move of 16-bit words, thread per input element
__global__ void pixelshuffle2_h16_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ y, long long N, int H, int W, int C) {
    const int Co = C >> 2;
    const long long total = N * H * W * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc p = nyxc(i, H, W, C);
        const int c = p.c4 >> 2, di = (p.c4 >> 1) & 1, dj = p.c4 & 1;
        y[((p.n * 2 * H + 2 * p.y + di) * 2 * W + 2 * p.x + dj) * Co + c] = x[i];
    }
}

// SE gate + skip + ReLU: y = relu(x * sigmoid(g[n][c]) + res), g fp32, the pre-sigmoid output of the second Linear
template <typename T>
__global__ void se_scale_add_relu_h16_kernel(const uint4* __restrict__ x, const float* __restrict__ g, const uint4* __restrict__ res,
                                             uint4* __restrict__ y, long long N, int HW, int G) {
    const long long total = N * HW * G;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int gq = (int)(i % G);
        const long long n = i / ((long long)HW * G);
        float a[8], r[8];
        h16_unpack8<T>(x[i], a);
        h16_unpack8<T>(res[i], r);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = fmaxf(fmaf(a[j], sigmoidf(g[(n * G + gq) * 8 + j]), r[j]), 0.f);
        y[i] = h16_pack8<T>(a);
    }
}

// HRNet fuse: y = act(base + sum_k nearest_up(z_k, 2^shift_k)), sources added in fp32 in argument order
struct FuseUpH16Args { const uint4* z[3]; int shift[3]; int n; };
template <typename T>
__global__ void fuse_up_h16_kernel(const uint4* __restrict__ base, FuseUpH16Args a, uint4* __restrict__ y, long long N, int H, int W, int G, int relu) {
    const long long total = N * H * W * G;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc p = nyxc(i, H, W, G);
        float v[8], f[8];
        h16_unpack8<T>(base[i], v);
        for (int k = 0; k < a.n; ++k) {
            const int s = a.shift[k];
            const int h2 = H >> s, w2 = W >> s;
            h16_unpack8<T>(a.z[k][((p.n * h2 + (p.y >> s)) * w2 + (p.x >> s)) * G + p.c4], f);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += f[j];
        }
        if (relu) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
        }
        y[i] = h16_pack8<T>(v);
    }
}

// the arguments every T NHWC kernel above needs: a known dtype, channels in groups of eight, 16-byte aligned tensors
static int glue_h16_contract(const char* what, int dtype, int C, const void* a, const void* b, const void* c = nullptr) {
    if (!h16_dtype_ok(dtype)) return fail(VATL_EINVAL, "%s: dtype %d is neither float16 (0) nor bfloat16 (1)", what, dtype);
    if (C < 8 || (C & 7)) return fail(VATL_EINVAL, "%s: C %d is not a multiple of 8", what, C);
    if (!h16_aligned16(a) || !h16_aligned16(b) || !h16_aligned16(c)) return fail(VATL_EINVAL, "%s: tensors must be 16-byte aligned", what);
    return 0;
}

}  // namespace vatl

using namespace vatl;

#define H16_LAUNCH(kernel, dtype, grid, stream, ...)                                                                  \
    do {                                                                                                              \
        if ((dtype) == kH16F16) hipLaunchKernelGGL(kernel<F16>, dim3(grid), dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel<BF16>, dim3(grid), dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__);          \
    } while (0)

extern "C" int vatl_nchw_to_nhwc_h16(const float* src, void* dst, int N, int C, int H, int W, int dtype, void* stream) {
    if (!src || !dst || N < 0 || C < 1 || H < 1 || W < 1) return fail(VATL_EINVAL, "nchw_to_nhwc_h16: bad arguments");
    const int C8 = (C + 7) & ~7;
    if (const int rc = glue_h16_contract("nchw_to_nhwc_h16", dtype, C8, dst, nullptr)) return rc;
    if (N == 0) return 0;
    H16_LAUNCH(nchw_to_nhwc_h16_kernel, dtype, ew_grid((long long)N * H * W * (C8 >> 3)), stream, src, (uint4*)dst, (long long)N, C, C8, H * W);
    return check_launch("nchw_to_nhwc_h16");
}

extern "C" int vatl_nhwc_to_nchw_h16(const void* src, float* dst, int N, int C, int H, int W, int dtype, void* stream) {
    if (!src || !dst || N < 0 || C < 1 || H < 1 || W < 1 || !h16_dtype_ok(dtype)) return fail(VATL_EINVAL, "nhwc_to_nchw_h16: bad arguments");
    if (N == 0) return 0;
    H16_LAUNCH(nhwc_to_nchw_h16_kernel, dtype, ew_grid((long long)N * C * H * W), stream, (const unsigned short*)src, dst, (long long)N, C, H * W);
    return check_launch("nhwc_to_nchw_h16");
}

extern "C" int vatl_maxpool3x3s2_fwd_h16(const void* x, void* y, int N, int H, int W, int C, int dtype, void* stream) {
    if (!x || !y || N < 0 || H < 1 || W < 1) return fail(VATL_EINVAL, "maxpool3x3s2_fwd_h16: bad arguments");
    if (const int rc = glue_h16_contract("maxpool3x3s2_fwd_h16", dtype, C, x, y)) return rc;
    if (N == 0) return 0;
    const int Ho = pool_out(H), Wo = pool_out(W);
    H16_LAUNCH(maxpool3x3s2_h16_kernel, dtype, ew_grid((long long)N * Ho * Wo * (C >> 3)), stream, (const uint4*)x, (uint4*)y, (long long)N, H, W, C >> 3, Ho, Wo);
    return check_launch("maxpool3x3s2_fwd_h16");
}

extern "C" int vatl_gap_fwd_h16(const void* x, float* y, int N, int HW, int C, int dtype, void* stream) {
    if (!x || !y || N < 0 || C < 1 || HW < 1 || !h16_dtype_ok(dtype)) return fail(VATL_EINVAL, "gap_fwd_h16: bad arguments");
    if (N == 0) return 0;
    H16_LAUNCH(gap_h16_kernel, dtype, ew_grid((long long)N * C), stream, (const unsigned short*)x, y, (long long)N, HW, C);
    return check_launch("gap_fwd_h16");
}

extern "C" int vatl_pixelshuffle2_fwd_h16(const void* x, void* y, int N, int H, int W, int C, int dtype, void* stream) {
    if (!x || !y || N < 0 || C < 4 || (C & 3) || H < 1 || W < 1 || !h16_dtype_ok(dtype))
        return fail(VATL_EINVAL, "pixelshuffle2_fwd_h16: C %d must be a multiple of 4", C);
    if (N == 0) return 0;
    hipLaunchKernelGGL(pixelshuffle2_h16_kernel, dim3(ew_grid((long long)N * H * W * C)), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x,
                       (unsigned short*)y, (long long)N, H, W, C);
    return check_launch("pixelshuffle2_fwd_h16");
}

extern "C" int vatl_se_scale_add_relu_h16(const void* x, const float* gate, const void* residual, void* y, int N, int HW, int C, int dtype, void* stream) {
    if (!x || !gate || !residual || !y || N < 0 || HW < 1) return fail(VATL_EINVAL, "se_scale_add_relu_h16: bad arguments");
    if (const int rc = glue_h16_contract("se_scale_add_relu_h16", dtype, C, x, residual, y)) return rc;
    if (N == 0) return 0;
    H16_LAUNCH(se_scale_add_relu_h16_kernel, dtype, ew_grid((long long)N * HW * (C >> 3)), stream, (const uint4*)x, gate, (const uint4*)residual, (uint4*)y,
               (long long)N, HW, C >> 3);
    return check_launch("se_scale_add_relu_h16");
}

extern "C" int vatl_fuse_upsample_add_h16(const void* base, const void* z0, int shift0, const void* z1, int shift1, const void* z2, int shift2, void* y, int N,
                                          int H, int W, int C, int relu, int dtype, void* stream) {
    if (!base || !y || N < 0 || H < 1 || W < 1) return fail(VATL_EINVAL, "fuse_upsample_add_h16: bad arguments");
    if (const int rc = glue_h16_contract("fuse_upsample_add_h16", dtype, C, base, y)) return rc;
    FuseUpH16Args a{};
    const void* zs[3] = {z0, z1, z2};
    const int sh[3] = {shift0, shift1, shift2};
    for (int k = 0; k < 3; ++k) {
        if (!zs[k]) continue;
        if (sh[k] < 1 || sh[k] > 5 || (H & ((1 << sh[k]) - 1)) || (W & ((1 << sh[k]) - 1)))
            return fail(VATL_EINVAL, "fuse_upsample_add_h16: %dx%d is not divisible by 2^%d", H, W, sh[k]);
        if (!h16_aligned16(zs[k])) return fail(VATL_EINVAL, "fuse_upsample_add_h16: tensors must be 16-byte aligned");
        a.z[a.n] = (const uint4*)zs[k]; a.shift[a.n] = sh[k]; ++a.n;
    }
    if (N == 0) return 0;
    H16_LAUNCH(fuse_up_h16_kernel, dtype, ew_grid((long long)N * H * W * (C >> 3)), stream, (const uint4*)base, a, (uint4*)y, (long long)N, H, W, C >> 3, relu);
    return check_launch("fuse_upsample_add_h16");
}
