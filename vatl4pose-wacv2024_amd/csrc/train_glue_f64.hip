// Training-mode glue of the float64 REFERENCE step (alphapose/models/hip_train_f64.py; convolutions: conv_f64.hip, wgrad_f64.hip):
// BatchNorm2d(train) forward and backward, the MaxPool2d(3,2,1) backward and a column sum on NHWC float64 tensors with ANY channel
// count.  A yardstick, not a timed route: no knob, no FLOP meter, one thread per element where that is enough.
//   * everything is float64: statistics, (scale, bias), dgamma, dbeta, the running statistics a step WOULD write (returned, never
//     written to the module).  Formulas of bn_train.hip: mean = s / M, biased variance = max(q / M - mean^2, 0) for the normalisation,
//     unbiased (M > 1) into the running variance, momentum as nn.BatchNorm2d;
//   * every reduction has one fixed order and no atomics: a block owns kRowsPerBlock consecutive rows (boundaries: the row count
//     only), a thread adds every eighth row of them in ascending order, the eight row lanes are combined in lane order, the row blocks
//     in ascending order per wave lane and through a fixed xor tree;
//   * the ReLU mask is taken from the STORED y (y > 0); the max-pool gradient goes to the FIRST maximum of a window in scan order
//     (torch's tie rule), gathered per input pixel over its <= 4 windows in window order.
#include "glue_common.h"
#include "pool.h"

namespace vatl {

// Column reduction over the M rows: block (rb, slab of 32 channels), thread = channel t & 31, row lane t >> 5.
// MODE 0: (sum a, sum a^2).  MODE 1: (sum g, sum g * xhat), g = a * [y > 0] (y NULL: no mask), xhat = (z - mean) * invstd.
// partial[(rb * C + c) * 2 + {0, 1}]
template <int MODE>
__global__ __launch_bounds__(256) void tg64_col_reduce_kernel(const double* __restrict__ a, const double* __restrict__ y, const double* __restrict__ z,
                                                              const double* __restrict__ mean, const double* __restrict__ invstd, double* __restrict__ partial,
                                                              long long M, int C) {
    __shared__ double sh[2][8][33];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = blockIdx.y * 32 + cl;
    const long long r0 = (long long)blockIdx.x * kRowsPerBlock;
    const long long r1 = r0 + kRowsPerBlock < M ? r0 + kRowsPerBlock : M;
    double s = 0.0, q = 0.0;
    if (c < C) {
        const double mu = MODE == 1 ? mean[c] : 0.0, is = MODE == 1 ? invstd[c] : 0.0;
        for (long long r = r0 + rl; r < r1; r += 8) {
            double v = a[r * C + c];
            if (MODE == 0) {
                s += v;
                q = fma(v, v, q);
            } else {
                if (y && !(y[r * C + c] > 0.0)) v = 0.0;
                s += v;
                q = fma(v, (z[r * C + c] - mu) * is, q);
            }
        }
    }
    sh[0][rl][cl] = s;
    sh[1][rl][cl] = q;
    __syncthreads();
    if (rl == 0 && c < C) {                     // the eight row lanes in order
        double ds = 0.0, dq = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) { ds += sh[0][k][cl]; dq += sh[1][k][cl]; }
        double* dst = partial + ((long long)blockIdx.x * C + c) * 2;
        dst[0] = ds;
        dst[1] = dq;
    }
}

// out: seven rows of C doubles — mean, biased variance, invstd, scale, bias, would-be running mean, would-be running variance
__global__ __launch_bounds__(256) void tg64_bn_fwd_finalize_kernel(const double* __restrict__ partial, int nrb, long long M, int C, const double* __restrict__ gamma,
                                                                   const double* __restrict__ beta, const double* __restrict__ running_mean,
                                                                   const double* __restrict__ running_var, double momentum, double eps, double* __restrict__ out) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    double s, q;
    tg_sum_partials(partial, nrb, C, c, lane, s, q);
    if (c >= C || lane != 0) return;
    const double mean = s / (double)M;
    double var;
    {
#pragma clang fp contract(off)                                // the square is rounded on its own, as q's terms are: M = 1 gives exactly 0
        const double m2 = mean * mean;
        var = q / (double)M - m2;
    }
    if (var < 0.0) var = 0.0;
    const double invstd = 1.0 / sqrt(var + eps);
    const double g = gamma ? gamma[c] : 1.0, b = beta ? beta[c] : 0.0;
    const double scale = g * invstd;
    out[c] = mean;
    out[C + c] = var;
    out[2 * C + c] = invstd;
    out[3 * C + c] = scale;
    out[4 * C + c] = b - mean * scale;
    const double unbiased = M > 1 ? var * (double)M / (double)(M - 1) : var;
    out[5 * C + c] = running_mean ? (1.0 - momentum) * running_mean[c] + momentum * mean : mean;
    out[6 * C + c] = running_var ? (1.0 - momentum) * running_var[c] + momentum * unbiased : unbiased;
}

__global__ __launch_bounds__(256) void tg64_bn_bwd_finalize_kernel(const double* __restrict__ partial, int nrb, int C, double* __restrict__ dgamma,
                                                                   double* __restrict__ dbeta) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    double sg, sgx;
    tg_sum_partials(partial, nrb, C, c, lane, sg, sgx);
    if (c >= C || lane != 0) return;
    dbeta[c] = sg;
    dgamma[c] = sgx;
}

__global__ __launch_bounds__(256) void tg64_col_sum_finalize_kernel(const double* __restrict__ partial, int nrb, int C, double* __restrict__ out) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    double s, q;
    tg_sum_partials(partial, nrb, C, c, lane, s, q);
    if (c >= C || lane != 0) return;
    out[c] = s;
}

// y = act(z * scale[c] + bias[c] (+ residual))
__global__ void tg64_bn_apply_kernel(const double* __restrict__ z, const double* __restrict__ scale, const double* __restrict__ bias, const double* __restrict__ res,
                                     double* __restrict__ y, long long total, int C, int relu) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        double v = fma(z[i], scale[c], bias[c]);
        if (res) v += res[i];
        if (relu) v = fmax(v, 0.0);
        y[i] = v;
    }
}

// dz = gamma*invstd*(g - dbeta/M - xhat*dgamma/M), g = dy * [y > 0]; optionally g itself (the gradient of a skip connection)
__global__ void tg64_bn_bwd_apply_kernel(const double* __restrict__ dy, const double* __restrict__ y, const double* __restrict__ z, const double* __restrict__ gamma,
                                         const double* __restrict__ mean, const double* __restrict__ invstd, const double* __restrict__ dgamma,
                                         const double* __restrict__ dbeta, double* __restrict__ dz, double* __restrict__ gout, long long total, int C, double inv_m) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        double g = dy[i];
        if (y && !(y[i] > 0.0)) g = 0.0;
        const double xhat = (z[i] - mean[c]) * invstd[c];
        dz[i] = (gamma ? gamma[c] : 1.0) * invstd[c] * (g - dbeta[c] * inv_m - xhat * (dgamma[c] * inv_m));
        if (gout) gout[i] = g;
    }
}

// MaxPool2d(3,2,1) backward in gather form: dx of input pixel (iy, ix) = sum, over the <= 4 windows that cover it in window order, of dpool
// where this pixel is the window's FIRST maximum in scan order (rows, then columns, padding skipped) — recomputed from x, no index tensor
__global__ void tg64_maxpool_bwd_kernel(const double* __restrict__ dpool, const double* __restrict__ x, double* __restrict__ dx, long long N, int H, int W, int C,
                                        int Ho, int Wo) {
    const long long total = N * H * W * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Nyxc p = nyxc(i, H, W, C);
        double acc = 0.0;
        // windows oy with pool_in(oy, 0) <= iy <= pool_in(oy, 2): oy in [iy / 2, (iy + 1) / 2]
        for (int oy = p.y >> 1; oy <= (p.y + 1) >> 1; ++oy) {
            if (oy >= Ho) continue;
            for (int ox = p.x >> 1; ox <= (p.x + 1) >> 1; ++ox) {
                if (ox >= Wo) continue;
                double best = 0.0;
                int bk = 255;
                for (int k = 0; k < 9; ++k) {
                    const int wy = pool_in(oy, k / 3), wx = pool_in(ox, k % 3);
                    if ((unsigned)wy >= (unsigned)H || (unsigned)wx >= (unsigned)W) continue;
                    const double v = x[((p.n * H + wy) * W + wx) * C + p.c4];
                    if (pool_takes(v, best, bk)) { best = v; bk = k; }
                }
                if (bk == pool_tap(p.y, p.x, oy, ox)) acc += dpool[((p.n * Ho + oy) * Wo + ox) * C + p.c4];
            }
        }
        dx[i] = acc;
    }
}

static int tg64_contract(const char* what, long long M, int C) {
    if (C < 1) return fail(VATL_EINVAL, "%s: C %d", what, C);
    if (M < 1 || M * C >= (1LL << 40)) return fail(VATL_EINVAL, "%s: bad row count", what);
    return 0;
}

}  // namespace vatl

using namespace vatl;

extern "C" int64_t vatl_bn_f64_workspace_doubles(int64_t M, int C) { return M < 1 || C < 1 ? 0 : 2 * (int64_t)tg_row_blocks(M) * C; }

extern "C" int vatl_bn_train_fwd_stats_f64(const double* z, int64_t M, int C, const double* gamma, const double* beta, const double* running_mean,
                                           const double* running_var, double momentum, double eps, double* stats7C, double* workspace, void* stream) {
    const char* what = "bn_train_fwd_stats_f64";
    if (!z || !stats7C || !workspace) return fail(VATL_EINVAL, "%s: null pointer", what);
    if ((running_mean == nullptr) != (running_var == nullptr)) return fail(VATL_EINVAL, "%s: running mean and variance come together", what);
    if (const int rc = tg64_contract(what, M, C)) return rc;
    const int nrb = tg_row_blocks(M);
    hipLaunchKernelGGL(tg64_col_reduce_kernel<0>, dim3(nrb, cdiv(C, 32)), dim3(256), 0, (hipStream_t)stream, z, (const double*)nullptr, (const double*)nullptr,
                       (const double*)nullptr, (const double*)nullptr, workspace, (long long)M, C);
    if (const int rc = check_launch("bn_train_fwd_stats_f64 (reduction)")) return rc;
    hipLaunchKernelGGL(tg64_bn_fwd_finalize_kernel, dim3(cdiv(C, 4)), dim3(256), 0, (hipStream_t)stream, workspace, nrb, (long long)M, C, gamma, beta, running_mean,
                       running_var, momentum, eps, stats7C);
    return check_launch("bn_train_fwd_stats_f64 (finalize)");
}

extern "C" int vatl_bn_apply_f64(const double* z, const double* scale, const double* bias, const double* residual, double* y, int64_t M, int C, int relu,
                                 void* stream) {
    if (!z || !scale || !bias || !y) return fail(VATL_EINVAL, "bn_apply_f64: null pointer");
    if (const int rc = tg64_contract("bn_apply_f64", M, C)) return rc;
    const long long total = M * C;
    hipLaunchKernelGGL(tg64_bn_apply_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, z, scale, bias, residual, y, total, C, relu);
    return check_launch("bn_apply_f64");
}

extern "C" int vatl_bn_train_bwd_f64(const double* dy, const double* y_or_null, const double* z, const double* gamma, const double* save_mean,
                                     const double* save_invstd, double* dz, double* g_out_or_null, double* dgamma, double* dbeta, int64_t M, int C,
                                     double* workspace, void* stream) {
    if (!dy || !z || !save_mean || !save_invstd || !dz || !dgamma || !dbeta || !workspace) return fail(VATL_EINVAL, "bn_train_bwd_f64: null pointer");
    if (const int rc = tg64_contract("bn_train_bwd_f64", M, C)) return rc;
    const int nrb = tg_row_blocks(M);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tg64_col_reduce_kernel<1>, dim3(nrb, cdiv(C, 32)), dim3(256), 0, st, dy, y_or_null, z, save_mean, save_invstd, workspace, (long long)M, C);
    if (const int rc = check_launch("bn_train_bwd_f64 (reduction)")) return rc;
    hipLaunchKernelGGL(tg64_bn_bwd_finalize_kernel, dim3(cdiv(C, 4)), dim3(256), 0, st, workspace, nrb, C, dgamma, dbeta);
    if (const int rc = check_launch("bn_train_bwd_f64 (finalize)")) return rc;
    const long long total = M * C;
    hipLaunchKernelGGL(tg64_bn_bwd_apply_kernel, dim3(ew_grid(total)), dim3(256), 0, st, dy, y_or_null, z, gamma, save_mean, save_invstd, (const double*)dgamma,
                       (const double*)dbeta, dz, g_out_or_null, total, C, 1.0 / (double)M);
    return check_launch("bn_train_bwd_f64 (apply)");
}

extern "C" int vatl_maxpool3x3s2_bwd_f64(const double* dpool, const double* x, double* dx, int N, int H, int W, int C, void* stream) {
    if (!dpool || !x || !dx || N < 1 || H < 1 || W < 1) return fail(VATL_EINVAL, "maxpool3x3s2_bwd_f64: bad arguments");
    if (const int rc = tg64_contract("maxpool3x3s2_bwd_f64", (long long)N * H * W, C)) return rc;
    const long long total = (long long)N * H * W * C;
    hipLaunchKernelGGL(tg64_maxpool_bwd_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, dpool, x, dx, (long long)N, H, W, C, pool_out(H),
                       pool_out(W));
    return check_launch("maxpool3x3s2_bwd_f64");
}

extern "C" int vatl_col_sum_f64(const double* x, int64_t M, int C, double* out, double* workspace, void* stream) {
    if (!x || !out || !workspace) return fail(VATL_EINVAL, "col_sum_f64: null pointer");
    if (const int rc = tg64_contract("col_sum_f64", M, C)) return rc;
    const int nrb = tg_row_blocks(M);
    hipLaunchKernelGGL(tg64_col_reduce_kernel<0>, dim3(nrb, cdiv(C, 32)), dim3(256), 0, (hipStream_t)stream, x, (const double*)nullptr, (const double*)nullptr,
                       (const double*)nullptr, (const double*)nullptr, workspace, (long long)M, C);
    if (const int rc = check_launch("col_sum_f64 (reduction)")) return rc;
    hipLaunchKernelGGL(tg64_col_sum_finalize_kernel, dim3(cdiv(C, 4)), dim3(256), 0, (hipStream_t)stream, workspace, nrb, C, out);
    return check_launch("col_sum_f64 (finalize)");
}
