// Layout changes on fp32 activations: the NCHW <-> NHWC transposes at the ends of a network, PixelShuffle(2) and its inverse.
#include "glue_common.h"

namespace vatl {

// Cpad % 4 == 0, Cpad > 4 (the 17 -> 32 channel gradient of the heat-map head): one thread per (pixel, four channels), the channel
// group fastest, so a wave writes 1 KB of contiguous NHWC rows (the per-pixel version below wrote 4 bytes per lane 128 bytes apart:
// 165 us for 120 x 17 x 64 x 48 at 0.44 TB/s)
__global__ void nchw_to_nhwc_c4_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int C, int HW, int Cpad) {
    const int G = Cpad >> 2;
    const long long total = (long long)N * HW * G;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int g = (int)(i % G);
        const long long pix = i / G;
        const long long n = pix / HW;
        const int px = (int)(pix - n * HW);
        const float* s = src + (n * C + 4 * g) * HW + px;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * g + k < C) v[k] = s[(long long)k * HW];
        *reinterpret_cast<f32x4*>(dst + i * 4) = v;
    }
}

// one thread per destination pixel; Cpad floats written contiguously
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int C, int HW, int Cpad) {
    const long long total = (long long)N * HW;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / HW;
        const int px = (int)(i - n * HW);
        const float* s = src + n * C * HW + px;
        float* d = dst + i * Cpad;
        if (Cpad == 4) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            for (int c = 0; c < C && c < 4; ++c) v[c] = s[(long long)c * HW];
            *reinterpret_cast<f32x4*>(d) = v;
        } else {
            for (int c = 0; c < Cpad; ++c) d[c] = c < C ? s[(long long)c * HW] : 0.f;
        }
    }
}

// one thread per destination element (n,c,pixel): reads stride C (L2 absorbs it; test/debug path)
__global__ void nhwc_to_nchw_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int C, int HW) {
    const long long total = (long long)N * C * HW;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int px = (int)(i % HW);
        const long long nc = i / HW;
        const int c = (int)(nc % C);
        const long long n = nc / C;
        dst[i] = src[(n * HW + px) * C + c];
    }
}

// PixelShuffle(2) on NHWC: out[b][2y+i][2x+j][c] = in[b][y][x][4c + 2i + j]
// thread per (input pixel, 4 input channels = one output channel c at the 4 sub-positions)
__global__ void pixelshuffle2_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W, int C) {
    const int C4 = C >> 2;
    const long long total = (long long)N * H * W * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc p = nyxc(i, H, W, C4);
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + i * 4);
        float* o = y + ((p.n * 2 * H + 2 * p.y) * 2 * W + 2 * p.x) * C4 + p.c4;
        o[0] = v[0];
        o[C4] = v[1];
        o[(long long)2 * W * C4] = v[2];
        o[(long long)2 * W * C4 + C4] = v[3];
    }
}

// inverse of PixelShuffle(2) on NHWC (its backward): in (N,2H,2W,C/4) -> out (N,H,W,C), out[y][x][4c+2i+j] = in[2y+i][2x+j][c]
__global__ void pixelunshuffle2_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W, int C) {
    const int C4 = C >> 2;
    const long long total = (long long)N * H * W * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc p = nyxc(i, H, W, C4);
        const float* s = x + ((p.n * 2 * H + 2 * p.y) * 2 * W + 2 * p.x) * C4 + p.c4;
        f32x4 v;
        v[0] = s[0]; v[1] = s[C4]; v[2] = s[(long long)2 * W * C4]; v[3] = s[(long long)2 * W * C4 + C4];
        *reinterpret_cast<f32x4*>(y + i * 4) = v;
    }
}

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_nchw_to_nhwc(const float* src, float* dst, int N, int C, int H, int W, int Cpad, void* stream) {
    if (!src || !dst || Cpad < C) return fail(VATL_EINVAL, "nchw_to_nhwc: bad arguments");
    if (Cpad > 4 && (Cpad & 3) == 0 && ((uintptr_t)dst & 15) == 0)
        hipLaunchKernelGGL(nchw_to_nhwc_c4_kernel, dim3(ew_grid((long long)N * H * W * (Cpad / 4))), dim3(256), 0, (hipStream_t)stream, src, dst, N, C, H * W, Cpad);
    else
        hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(ew_grid((long long)N * H * W)), dim3(256), 0, (hipStream_t)stream, src, dst, N, C, H * W, Cpad);
    return check_launch("nchw_to_nhwc");
}

extern "C" int vatl_nhwc_to_nchw(const float* src, float* dst, int N, int C, int H, int W, void* stream) {
    if (!src || !dst) return fail(VATL_EINVAL, "nhwc_to_nchw: null pointer");
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(ew_grid((long long)N * C * H * W)), dim3(256), 0, (hipStream_t)stream, src, dst, N, C, H * W);
    return check_launch("nhwc_to_nchw");
}

extern "C" int vatl_pixelshuffle2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream) {
    if (!x || !y || (C & 15)) return fail(VATL_EINVAL, "pixelshuffle2_fwd: C %d must be a multiple of 16", C);
    hipLaunchKernelGGL(pixelshuffle2_kernel, dim3(ew_grid((long long)N * H * W * (C / 4))), dim3(256), 0, (hipStream_t)stream, x, y, N, H, W, C);
    return check_launch("pixelshuffle2_fwd");
}

extern "C" int vatl_pixelunshuffle2(const float* x, float* y, int N, int H, int W, int C, void* stream) {
    if (!x || !y || (C & 15)) return fail(VATL_EINVAL, "pixelunshuffle2: C %d must be a multiple of 16", C);
    hipLaunchKernelGGL(pixelunshuffle2_kernel, dim3(ew_grid((long long)N * H * W * (C / 4))), dim3(256), 0, (hipStream_t)stream, x, y, N, H, W, C);
    return check_launch("pixelunshuffle2");
}
