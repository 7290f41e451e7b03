// Pooling on NHWC: MaxPool2d(3, 2, 1) — inference forward, training forward with recorded winners (plain, or with the BatchNorm
// affine and ReLU of the stem applied on load), backward by recomputation or from the winners — and the global average pool with
// the per-item pixel reductions of small batches.  Geometry and winner rule: pool.h.
#include "pool.h"

namespace vatl {

// inference forward: thread per (n, oy, ox, 4 channels); padding behaves as -inf
__global__ void maxpool3x3s2_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W, int C, int Ho, int Wo) {
    const int C4 = C >> 2;
    const long long total = (long long)N * Ho * Wo * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc o = nyxc(i, Ho, Wo, C4);
        f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int iy = pool_in(o.y, dy);
            if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int ix = pool_in(o.x, dx);
                if ((unsigned)ix >= (unsigned)W) continue;
                const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((o.n * H + iy) * W + ix) * C + o.c4 * 4);
                m[0] = fmaxf(m[0], v[0]); m[1] = fmaxf(m[1], v[1]); m[2] = fmaxf(m[2], v[2]); m[3] = fmaxf(m[3], v[3]);
            }
        }
        *reinterpret_cast<f32x4*>(y + i * 4) = m;
    }
}

// backward by recomputation (no recorded winners; any C): each input pixel rescans the windows covering it
__global__ void maxpool3x3s2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                        int N, int H, int W, int C, int Ho, int Wo) {
    const long long total = (long long)N * H * W * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc p = nyxc(i, H, W, C);
        float acc = 0.f;
        for (int oy = (p.y >> 1); oy <= ((p.y + 1) >> 1); ++oy) {
            if (oy >= Ho) continue;
            for (int ox = (p.x >> 1); ox <= ((p.x + 1) >> 1); ++ox) {
                if (ox >= Wo) continue;
                float best = -INFINITY; int bk = 255;
                for (int k = 0; k < 9; ++k) {
                    const int yy = pool_in(oy, k / 3), xx = pool_in(ox, k % 3);
                    if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
                    const float v = x[((p.n * H + yy) * W + xx) * C + p.c4];
                    if (pool_takes(v, best, bk)) { best = v; bk = k; }
                }
                if (bk == pool_tap(p.y, p.x, oy, ox)) acc += dy[((p.n * Ho + oy) * Wo + ox) * C + p.c4];
            }
        }
        dx[i] = acc;
    }
}

// training forward that also records which of the 9 window taps won; one channel per thread (C % 4 != 0)
__global__ void maxpool3x3s2_fwd_idx_kernel(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ idx,
                                            int N, int H, int W, int C, int Ho, int Wo) {
    const long long total = (long long)N * Ho * Wo * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc o = nyxc(i, Ho, Wo, C);
        float best = -INFINITY; int bk = 255;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int yy = pool_in(o.y, k / 3), xx = pool_in(o.x, k % 3);
            if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
            const float v = x[((o.n * H + yy) * W + xx) * C + o.c4];
            if (pool_takes(v, best, bk)) { best = v; bk = k; }
        }
        y[i] = best;
        idx[i] = (uint8_t)bk;
    }
}

// ... four channels per thread (float4 / uchar4).  AFFINE: the stem tail of the ResNet trunks in training mode (Resnet.py:171-172:
// bn1 -> relu -> maxpool), relu(z*scale + bias) applied to z on load and never stored — the same fmaf as scale_bias_act_kernel, so
// values and winners are those of the unfused pair of passes, bit for bit.  Its backward: bn_train.hip, pool_bn_bwd_*_kernel.
template <bool AFFINE>
__global__ __launch_bounds__(256) void maxpool3x3s2_fwd_idx4_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ bias,
                                                                   float* __restrict__ y, uint8_t* __restrict__ idx, int N, int H, int W, int C4, int Ho, int Wo) {
    const long long total = (long long)N * Ho * Wo * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc o = nyxc(i, Ho, Wo, C4);
        f32x4 sc = {1.f, 1.f, 1.f, 1.f}, bi = {0.f, 0.f, 0.f, 0.f};
        if (AFFINE) { sc = *reinterpret_cast<const f32x4*>(scale + o.c4 * 4); bi = *reinterpret_cast<const f32x4*>(bias + o.c4 * 4); }
        f32x4 v[9];
        bool ok[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {                      // all nine loads in flight together
            const int yy = pool_in(o.y, k / 3), xx = pool_in(o.x, k % 3);
            ok[k] = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            v[k] = ok[k] ? *reinterpret_cast<const f32x4*>(x + (((o.n * H + yy) * W + xx) * C4 + o.c4) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int bk[4] = {255, 255, 255, 255};
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (!ok[k]) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float a = AFFINE ? fmaxf(fmaf(v[k][e], sc[e], bi[e]), 0.f) : v[k][e];
                if (pool_takes(a, best[e], bk[e])) { best[e] = a; bk[e] = k; }
            }
        }
        *reinterpret_cast<f32x4*>(y + i * 4) = best;
        *reinterpret_cast<unsigned*>(idx + i * 4) = (unsigned)bk[0] | ((unsigned)bk[1] << 8) | ((unsigned)bk[2] << 16) | ((unsigned)bk[3] << 24);
    }
}

// backward from the recorded winners (4 byte loads per pixel instead of 36 float loads); V channels per thread
template <int V>
__global__ __launch_bounds__(256) void maxpool3x3s2_bwd_idx_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ idx, float* __restrict__ dx,
                                                                  int N, int H, int W, int Cv, int Ho, int Wo) {
    const long long total = (long long)N * H * W * Cv;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc p = nyxc(i, H, W, Cv);
        *reinterpret_cast<f32v<V>*>(dx + i * V) = pool_gather<V>(dy, idx, p.n, p.y, p.x, p.c4, Cv, Ho, Wo);
    }
}

// global average pool: thread per (n, c), coalesced across c
__global__ void gap_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int HW, int C) {
    const long long total = (long long)N * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / C;
        const int c = (int)(i - n * C);
        const float* p = x + n * HW * C + c;
        float s = 0.f;
        for (int k = 0; k < HW; ++k) s += p[(long long)k * C];
        y[i] = s / (float)HW;
    }
}

// Per-item reductions over the pixels of an NHWC tensor for small batches (fine-tune steps: N = 32..120, where one thread per
// (item, channel) leaves most of the chip idle and walks thousands of pixels one load at a time).  A block owns `cols` float4
// channel columns of one item; its 256 threads take 256 / cols pixels at a time with four pixels in flight each and combine
// their partial sums through LDS in a fixed order (deterministic, no workspace, no atomics).
//   MODE 0: global average pool            out[n][c] = sum_hw x / HW
//   MODE 1: SE gate gradient               out[n][c] = sig'(gate) * sum_hw dy*[y>0]*u
// (gap_kernel and fusion.hip's se_bwd_gate_kernel, the large-batch routes, sum in pixel order: they round differently on purpose.)
template <int MODE>
__global__ __launch_bounds__(256) void hw_reduce_kernel(const float* __restrict__ a, const float* __restrict__ y, const float* __restrict__ u,
                                                        const float* __restrict__ gate, float* __restrict__ out, int HW, int C, int cols) {
    __shared__ f32x4 sh[256];
    const int C4 = C >> 2, groups = C4 / cols;
    const int n = blockIdx.x / groups, c4 = (blockIdx.x - n * groups) * cols + (threadIdx.x % cols);
    const int rlane = threadIdx.x / cols, rstep = 256 / cols;
    const long long base = (long long)n * HW * C4 + c4;
    const f32x4* a4 = reinterpret_cast<const f32x4*>(a) + base;
    const f32x4* y4 = reinterpret_cast<const f32x4*>(y) + base;
    const f32x4* u4 = reinterpret_cast<const f32x4*>(u) + base;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    auto fold = [&](f32x4 v, f32x4 yy, f32x4 uu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += MODE == 0 ? v[e] : (yy[e] > 0.f ? v[e] * uu[e] : 0.f);      // relu_mask() with the product formed only where it is used
    };
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    int k = rlane;
    for (; k + 3 * rstep < HW; k += 4 * rstep) {
        f32x4 v[4], yy[4], uu[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long long o = (long long)(k + q * rstep) * C4;
            v[q] = a4[o];
            yy[q] = MODE == 1 ? y4[o] : zero;
            uu[q] = MODE == 1 ? u4[o] : zero;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) fold(v[q], yy[q], uu[q]);
    }
    for (; k < HW; k += rstep) {
        const long long o = (long long)k * C4;
        fold(a4[o], MODE == 1 ? y4[o] : zero, MODE == 1 ? u4[o] : zero);
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    if (rlane == 0) {
        f32x4 t = sh[threadIdx.x];
        for (int r = 1; r < rstep; ++r) {
            const f32x4 w = sh[r * cols + threadIdx.x];
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] += w[e];
        }
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = MODE == 0 ? t[e] / (float)HW : se_gate_grad(t[e], gate[(long long)n * C + c4 * 4 + e]);
        *reinterpret_cast<f32x4*>(out + (long long)n * C + c4 * 4) = o;
    }
}

// float4 columns per block for hw_reduce_kernel: the widest power of two (8 = 128-byte segments at least) that still gives >= 512
// blocks; 0 = use the thread-per-(item, channel) kernels
static int hw_reduce_cols(int N, int HW, int C) {
    if ((C & 31) || HW < 64) return 0;                          // few pixels per item: the thread-per-(item, channel) kernels are fine
    const int C4 = C >> 2;
    if (C4 & (C4 - 1)) return 0;
    int cols = 8;
    while (cols * 2 <= C4 && cols * 2 <= 256 && (long long)N * (C4 / (cols * 2)) >= 512) cols *= 2;
    return cols;
}

bool hw_reduce_try(int mode, const float* a, const float* y, const float* u, const float* gate, float* out, int N, int HW, int C, hipStream_t st) {
    const int cols = hw_reduce_cols(N, HW, C);
    if (!cols) return false;
    const dim3 grid((unsigned)(N * ((C >> 2) / cols)));
    if (mode == 0) hipLaunchKernelGGL(hw_reduce_kernel<0>, grid, dim3(256), 0, st, a, y, u, gate, out, HW, C, cols);
    else           hipLaunchKernelGGL(hw_reduce_kernel<1>, grid, dim3(256), 0, st, a, y, u, gate, out, HW, C, cols);
    return true;
}

// backward of the global average pool: dx[n][p][c] = dy[n][c] / HW
__global__ void gap_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int N, int HW, int C, float inv) {
    const int C4 = C >> 2;
    const long long total = (long long)N * HW * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        const long long n = i / ((long long)HW * C4);
        f32x4 g = *reinterpret_cast<const f32x4*>(dy + (n * C4 + c4) * 4);
        g[0] *= inv; g[1] *= inv; g[2] *= inv; g[3] *= inv;
        *reinterpret_cast<f32x4*>(dx + i * 4) = g;
    }
}

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_maxpool3x3s2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream) {
    if (!x || !y || (C & 3)) return fail(VATL_EINVAL, "maxpool3x3s2_fwd: C %d must be a multiple of 4", C);
    const int Ho = pool_out(H), Wo = pool_out(W);
    hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3(ew_grid((long long)N * Ho * Wo * (C / 4))), dim3(256), 0, (hipStream_t)stream, x, y, N, H, W, C, Ho, Wo);
    return check_launch("maxpool3x3s2_fwd");
}

extern "C" int vatl_maxpool3x3s2_bwd(const float* x, const float* dy, float* dx, int N, int H, int W, int C, void* stream) {
    if (!x || !dy || !dx) return fail(VATL_EINVAL, "maxpool3x3s2_bwd: null pointer");
    const int Ho = pool_out(H), Wo = pool_out(W);
    hipLaunchKernelGGL(maxpool3x3s2_bwd_kernel, dim3(ew_grid((long long)N * H * W * C)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, N, H, W, C, Ho, Wo);
    return check_launch("maxpool3x3s2_bwd");
}

static int maxpool_fwd_idx_impl(const float* x, const float* scale, const float* bias, float* y, uint8_t* idx, int N, int H, int W, int C, void* stream) {
    if (!x || !y || !idx) return fail(VATL_EINVAL, "maxpool3x3s2_fwd_idx: null pointer");
    const int Ho = pool_out(H), Wo = pool_out(W);
    if ((C & 3) == 0) {
        const dim3 grid(ew_grid((long long)N * Ho * Wo * (C / 4)));
        if (scale) hipLaunchKernelGGL(maxpool3x3s2_fwd_idx4_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, scale, bias, y, idx, N, H, W, C / 4, Ho, Wo);
        else       hipLaunchKernelGGL(maxpool3x3s2_fwd_idx4_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, scale, bias, y, idx, N, H, W, C / 4, Ho, Wo);
        return check_launch("maxpool3x3s2_fwd_idx");
    }
    if (scale) return fail(VATL_EINVAL, "maxpool3x3s2_fwd_idx_affine: C %d must be a multiple of 4", C);
    hipLaunchKernelGGL(maxpool3x3s2_fwd_idx_kernel, dim3(ew_grid((long long)N * Ho * Wo * C)), dim3(256), 0, (hipStream_t)stream, x, y, idx, N, H, W, C, Ho, Wo);
    return check_launch("maxpool3x3s2_fwd_idx");
}

extern "C" int vatl_maxpool3x3s2_fwd_idx(const float* x, float* y, uint8_t* idx, int N, int H, int W, int C, void* stream) {
    return maxpool_fwd_idx_impl(x, nullptr, nullptr, y, idx, N, H, W, C, stream);
}

// BatchNorm-affine + ReLU + MaxPool2d(3,2,1) in one pass over the conv output z (Resnet.py:171-172 in training mode):
// y = pool(relu(z*scale + bias)), idx = winning taps; relu(z*scale + bias) itself is never stored.
extern "C" int vatl_maxpool3x3s2_fwd_idx_affine(const float* z, const float* scale, const float* bias, float* y, uint8_t* idx, int N, int H, int W, int C,
                                                void* stream) {
    if (!scale || !bias) return fail(VATL_EINVAL, "maxpool3x3s2_fwd_idx_affine: null scale / bias");
    return maxpool_fwd_idx_impl(z, scale, bias, y, idx, N, H, W, C, stream);
}

extern "C" int vatl_maxpool3x3s2_bwd_idx(const float* dy, const uint8_t* idx, float* dx, int N, int H, int W, int C, void* stream) {
    if (!dy || !idx || !dx) return fail(VATL_EINVAL, "maxpool3x3s2_bwd_idx: null pointer");
    const int Ho = pool_out(H), Wo = pool_out(W);
    if ((C & 3) == 0) hipLaunchKernelGGL(maxpool3x3s2_bwd_idx_kernel<4>, dim3(ew_grid((long long)N * H * W * (C / 4))), dim3(256), 0, (hipStream_t)stream, dy, idx, dx, N, H, W, C / 4, Ho, Wo);
    else hipLaunchKernelGGL(maxpool3x3s2_bwd_idx_kernel<1>, dim3(ew_grid((long long)N * H * W * C)), dim3(256), 0, (hipStream_t)stream, dy, idx, dx, N, H, W, C, Ho, Wo);
    return check_launch("maxpool3x3s2_bwd_idx");
}

extern "C" int vatl_gap_fwd(const float* x, float* y, int N, int HW, int C, void* stream) {
    if (!x || !y) return fail(VATL_EINVAL, "gap_fwd: null pointer");
    if (!hw_reduce_try(0, x, x, x, nullptr, y, N, HW, C, (hipStream_t)stream))
        hipLaunchKernelGGL(gap_kernel, dim3(ew_grid((long long)N * C)), dim3(256), 0, (hipStream_t)stream, x, y, N, HW, C);
    return check_launch("gap_fwd");
}

extern "C" int vatl_gap_bwd(const float* dy, float* dx, int N, int HW, int C, void* stream) {
    if (!dy || !dx || (C & 3) || HW < 1) return fail(VATL_EINVAL, "gap_bwd: bad arguments");
    if (N <= 0) return 0;
    hipLaunchKernelGGL(gap_bwd_kernel, dim3(ew_grid((long long)N * HW * (C / 4))), dim3(256), 0, (hipStream_t)stream, dy, dx, N, HW, C, 1.0f / (float)HW);
    return check_launch("gap_bwd");
}
