// Training-mode glue of the opt-in bf16 fine-tune step (alphapose/models/hip_train_h16.py; convolutions: conv_h16.hip, wgrad_h16.hip):
// BatchNorm2d(train) forward and backward and the MaxPool2d(3,2,1) backward on NHWC tensors of a 16-bit storage type T in
// {float16, bfloat16} whose channel count is a multiple of 8 (a thread moves eight channels as one 16-byte word).
// Arithmetic contract:
//   * z (conv output), y (BatchNorm (+ residual) (+ ReLU) output) and every gradient with respect to them are stored as T; a value is
//     converted to fp32 exactly, everything is computed in fp32 and rounded ONCE to T where it is stored;
//   * batch statistics, the backward sums, (scale, bias), dgamma, dbeta and the running statistics are fp32 (the per-channel totals are
//     formed in double from fp32 partials, with the formulas of bn_train.hip: mean = s / M, biased variance = q / M - mean^2 for the
//     normalisation, unbiased into running_var, momentum as nn.BatchNorm2d);
//   * every reduction has one fixed order and no atomics: a block owns kRowsPerBlock consecutive rows (boundaries: the row count only),
//     a thread adds every eighth row of them in ascending order, the eight row lanes are combined in lane order, the row blocks in
//     ascending order per wave lane and through a fixed xor tree.  A step is bit-reproducible run to run;
//   * the ReLU mask is taken from the STORED y (y > 0); the max-pool gradient goes to the FIRST maximum of a window in scan order
//     (torch's tie rule: post-ReLU planes are full of tied zeros), gathered per input pixel over its <= 4 windows in window order.
#include "glue_common.h"
#include "h16.h"
#include "pool.h"

namespace vatl {

// Column reduction over the M rows of an NHWC tensor: block (rb, slab of 32 channel groups), thread = channel group t & 31, row lane t >> 5.
// MODE 0: (sum z, sum z^2).  MODE 1: (sum g, sum g * xhat), g = dy * [y > 0] (y NULL: no mask), xhat = (z - mean) * invstd.
// partial[(rb * C + c) * 2 + {0, 1}] in double: the layout bn_train.hip's finalize kernels read.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void tg_col_reduce_kernel(const uint4* __restrict__ a, const uint4* __restrict__ y, const uint4* __restrict__ z,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd, double* __restrict__ partial,
                                                            long long M, int C) {
    __shared__ float sh[2][8][32][9];          // [sum][row lane][channel group][channel], rows padded to 9 floats
    const int G = C >> 3;
    const int cgl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int cg = blockIdx.y * 32 + cgl;
    const long long r0 = (long long)blockIdx.x * kRowsPerBlock;
    const long long r1 = r0 + kRowsPerBlock < M ? r0 + kRowsPerBlock : M;
    float s[8], q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = q[e] = 0.f;
    if (cg < G) {
        float mu[8], is[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { mu[e] = MODE == 1 ? mean[8 * cg + e] : 0.f; is[e] = MODE == 1 ? invstd[8 * cg + e] : 0.f; }
        for (long long r = r0 + rl; r < r1; r += 8) {
            float v[8];
            h16_unpack8<T>(a[r * G + cg], v);
            if (MODE == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) { s[e] += v[e]; q[e] = fmaf(v[e], v[e], q[e]); }
            } else {
                float zz[8];
                h16_unpack8<T>(z[r * G + cg], zz);
                if (y) {
                    float yy[8];
                    h16_unpack8<T>(y[r * G + cg], yy);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = relu_mask(yy[e], v[e]);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) { s[e] += v[e]; q[e] = fmaf(v[e], (zz[e] - mu[e]) * is[e], q[e]); }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { sh[0][rl][cgl][e] = s[e]; sh[1][rl][cgl][e] = q[e]; }
    __syncthreads();
    const int e = threadIdx.x >> 5;             // thread -> channel e of group cgl: the eight row lanes in order, in double
    if (cg < G) {
        double ds = 0.0, dq = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) { ds += (double)sh[0][k][cgl][e]; dq += (double)sh[1][k][cgl][e]; }
        double* dst = partial + ((long long)blockIdx.x * C + 8 * cg + e) * 2;
        dst[0] = ds;
        dst[1] = dq;
    }
}

// (sum g, sum g*xhat) -> dgamma, dbeta and the coefficients of dz = A*g + B*z + Cc (bn_train.hip's formulas): a wave per channel
__global__ __launch_bounds__(256) void tg_bn_bwd_finalize_kernel(const double* __restrict__ partial, int nrb, long long M, int C, const float* __restrict__ gamma,
                                                                 const float* __restrict__ mean, const float* __restrict__ invstd, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta, float* __restrict__ coef) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    double sg, sgx;
    tg_sum_partials(partial, nrb, C, c, lane, sg, sgx);
    if (c >= C || lane != 0) return;
    if (dbeta) dbeta[c] = (float)sg;
    if (dgamma) dgamma[c] = (float)sgx;
    const double s = (double)(gamma ? gamma[c] : 1.f) * (double)invstd[c];
    const double kb = -s * (double)invstd[c] * sgx / (double)M;
    coef[c] = (float)s;
    coef[C + c] = (float)kb;
    coef[2 * C + c] = (float)(-s * sg / (double)M - kb * (double)mean[c]);
}

// y = act(z * scale[c] + bias[c] (+ residual)) -> T
template <typename T>
__global__ void tg_bn_apply_kernel(const uint4* __restrict__ z, const float* __restrict__ scale, const float* __restrict__ bias, const uint4* __restrict__ res,
                                   uint4* __restrict__ y, long long total, int G, int relu) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c0 = 8 * (int)(i % G);
        float v[8];
        h16_unpack8<T>(z[i], v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaf(v[e], scale[c0 + e], bias[c0 + e]);
        if (res) {
            float r[8];
            h16_unpack8<T>(res[i], r);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += r[e];
        }
        if (relu) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        y[i] = h16_pack8<T>(v);
    }
}

// dz = A[c]*g + B[c]*z + Cc[c] -> T, g = dy * [y > 0]; optionally g itself (the gradient of a skip connection: T values, stored exactly)
template <typename T>
__global__ void tg_bn_bwd_apply_kernel(const uint4* __restrict__ dy, const uint4* __restrict__ y, const uint4* __restrict__ z, const float* __restrict__ coef, int C,
                                       uint4* __restrict__ dz, uint4* __restrict__ gout, long long total, int G) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c0 = 8 * (int)(i % G);
        float g[8], zz[8], o[8];
        h16_unpack8<T>(dy[i], g);
        h16_unpack8<T>(z[i], zz);
        if (y) {
            float yy[8];
            h16_unpack8<T>(y[i], yy);
#pragma unroll
            for (int e = 0; e < 8; ++e) g[e] = relu_mask(yy[e], g[e]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = coef[c0 + e] * g[e] + coef[C + c0 + e] * zz[e] + coef[2 * C + c0 + e];
        dz[i] = h16_pack8<T>(o);
        if (gout) gout[i] = h16_pack8<T>(g);
    }
}

// MaxPool2d(3,2,1) backward in gather form: dx of input pixel (iy, ix) = sum, over the <= 4 windows that cover it in window order, of dpool
// where this pixel is the window's FIRST maximum in scan order (rows, then columns, padding skipped) — recomputed from x, no index tensor
template <typename T>
__global__ void tg_maxpool_bwd_kernel(const uint4* __restrict__ dpool, const uint4* __restrict__ x, uint4* __restrict__ dx, long long N, int H, int W, int G, int Ho,
                                      int Wo) {
    const long long total = N * H * W * G;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc p = nyxc(i, H, W, G);
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        // windows oy with pool_in(oy, 0) <= iy <= pool_in(oy, 2): oy in [iy / 2, (iy + 1) / 2]
        for (int oy = p.y >> 1; oy <= (p.y + 1) >> 1; ++oy) {
            if (oy >= Ho) continue;
            for (int ox = p.x >> 1; ox <= (p.x + 1) >> 1; ++ox) {
                if (ox >= Wo) continue;
                float best[8];
                int bk[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) { best[e] = 0.f; bk[e] = 255; }
                for (int k = 0; k < 9; ++k) {
                    const int wy = pool_in(oy, k / 3), wx = pool_in(ox, k % 3);
                    if ((unsigned)wy >= (unsigned)H || (unsigned)wx >= (unsigned)W) continue;
                    float v[8];
                    h16_unpack8<T>(x[((p.n * H + wy) * W + wx) * G + p.c4], v);
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (pool_takes(v[e], best[e], bk[e])) { best[e] = v[e]; bk[e] = k; }
                }
                const int mine = pool_tap(p.y, p.x, oy, ox);
                float d[8];
                h16_unpack8<T>(dpool[((p.n * Ho + oy) * Wo + ox) * G + p.c4], d);
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (bk[e] == mine) acc[e] += d[e];
            }
        }
        dx[i] = h16_pack8<T>(acc);
    }
}

static int tg_contract(const char* what, int dtype, long long M, int C, const void* a, const void* b, const void* c = nullptr, const void* d = nullptr) {
    if (!h16_dtype_ok(dtype)) return fail(VATL_EINVAL, "%s: dtype %d is neither float16 (0) nor bfloat16 (1)", what, dtype);
    if (C < 8 || (C & 7)) return fail(VATL_EINVAL, "%s: C %d is not a multiple of 8", what, C);
    if (M < 1 || M * C >= (1LL << 40)) return fail(VATL_EINVAL, "%s: bad row count", what);
    if (!h16_aligned16(a) || !h16_aligned16(b) || !h16_aligned16(c) || !h16_aligned16(d)) return fail(VATL_EINVAL, "%s: tensors must be 16-byte aligned", what);
    return 0;
}

}  // namespace vatl

using namespace vatl;

#define TG_LAUNCH(kernel, dtype, grid, stream, ...)                                                                          \
    do {                                                                                                                     \
        if ((dtype) == kH16F16) hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<F16>), grid, dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__); \
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<BF16>), grid, dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__);      \
    } while (0)
#define TG_LAUNCH_MODE(kernel, mode, dtype, grid, stream, ...)                                                                       \
    do {                                                                                                                             \
        if ((dtype) == kH16F16) hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<F16, mode>), grid, dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__); \
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<BF16, mode>), grid, dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__);        \
    } while (0)

extern "C" int64_t vatl_bn_h16_workspace_doubles(int64_t M, int C) { return M < 1 ? 0 : 2 * (int64_t)tg_row_blocks(M) * C; }

extern "C" int vatl_bn_train_fwd_stats_h16(const void* z, int64_t M, int C, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                           float momentum, float eps, float* save_mean, float* save_invstd, float* scale, float* bias, double* workspace,
                                           int dtype, void* stream) {
    if (!z || !save_mean || !save_invstd || !scale || !bias || !workspace) return fail(VATL_EINVAL, "bn_train_fwd_stats_h16: null pointer");
    if (const int rc = tg_contract("bn_train_fwd_stats_h16", dtype, M, C, z, nullptr)) return rc;
    const int nrb = tg_row_blocks(M);
    TG_LAUNCH_MODE(tg_col_reduce_kernel, 0, dtype, dim3(nrb, cdiv(C >> 3, 32)), stream, (const uint4*)z, (const uint4*)nullptr, (const uint4*)nullptr,
                   (const float*)nullptr, (const float*)nullptr, workspace, (long long)M, C);
    if (const int rc = check_launch("bn_train_fwd_stats_h16")) return rc;
    // totals, (scale, bias) and the running statistics: bn_train.hip's finalize, the fp32 trainer's
    return vatl_bn_train_finalize(workspace, nrb, M, C, gamma, beta, running_mean, running_var, momentum, eps, save_mean, save_invstd, scale, bias, stream);
}

extern "C" int vatl_bn_apply_h16(const void* z, const float* scale, const float* bias, const void* residual, void* y, int64_t M, int C, int relu, int dtype,
                                 void* stream) {
    if (!z || !scale || !bias || !y) return fail(VATL_EINVAL, "bn_apply_h16: null pointer");
    if (const int rc = tg_contract("bn_apply_h16", dtype, M, C, z, residual, y)) return rc;
    const long long total = M * (C >> 3);
    TG_LAUNCH(tg_bn_apply_kernel, dtype, dim3(ew_grid(total)), stream, (const uint4*)z, scale, bias, (const uint4*)residual, (uint4*)y, total, C >> 3, relu);
    return check_launch("bn_apply_h16");
}

extern "C" int vatl_bn_train_bwd_h16(const void* dy, const void* y_or_null, const void* z, const float* gamma, const float* save_mean, const float* save_invstd,
                                     void* dz, void* g_out_or_null, float* dgamma, float* dbeta, int64_t M, int C, float* coef3C, double* workspace, int dtype,
                                     void* stream) {
    if (!dy || !z || !save_mean || !save_invstd || !dz || !coef3C || !workspace) return fail(VATL_EINVAL, "bn_train_bwd_h16: null pointer");
    if (const int rc = tg_contract("bn_train_bwd_h16", dtype, M, C, dy, y_or_null, z, dz)) return rc;
    if (!h16_aligned16(g_out_or_null)) return fail(VATL_EINVAL, "bn_train_bwd_h16: tensors must be 16-byte aligned");
    const int nrb = tg_row_blocks(M);
    hipStream_t st = (hipStream_t)stream;
    TG_LAUNCH_MODE(tg_col_reduce_kernel, 1, dtype, dim3(nrb, cdiv(C >> 3, 32)), stream, (const uint4*)dy, (const uint4*)y_or_null, (const uint4*)z, save_mean,
                   save_invstd, workspace, (long long)M, C);
    if (const int rc = check_launch("bn_train_bwd_h16 (reduction)")) return rc;
    hipLaunchKernelGGL(tg_bn_bwd_finalize_kernel, dim3(cdiv(C, 4)), dim3(256), 0, st, workspace, nrb, (long long)M, C, gamma, save_mean, save_invstd, dgamma, dbeta,
                       coef3C);
    if (const int rc = check_launch("bn_train_bwd_h16 (finalize)")) return rc;
    const long long total = M * (C >> 3);
    TG_LAUNCH(tg_bn_bwd_apply_kernel, dtype, dim3(ew_grid(total)), stream, (const uint4*)dy, (const uint4*)y_or_null, (const uint4*)z, coef3C, C, (uint4*)dz,
              (uint4*)g_out_or_null, total, C >> 3);
    return check_launch("bn_train_bwd_h16 (apply)");
}

extern "C" int vatl_maxpool3x3s2_bwd_h16(const void* dpool, const void* x, void* dx, int N, int H, int W, int C, int dtype, void* stream) {
    if (!dpool || !x || !dx || N < 1 || H < 1 || W < 1) return fail(VATL_EINVAL, "maxpool3x3s2_bwd_h16: bad arguments");
    if (const int rc = tg_contract("maxpool3x3s2_bwd_h16", dtype, (long long)N * H * W, C, dpool, x, dx)) return rc;
    const long long total = (long long)N * H * W * (C >> 3);
    TG_LAUNCH(tg_maxpool_bwd_kernel, dtype, dim3(ew_grid(total)), stream, (const uint4*)dpool, (const uint4*)x, (uint4*)dx, (long long)N, H, W, C >> 3, pool_out(H),
              pool_out(W));
    return check_launch("maxpool3x3s2_bwd_h16");
}
