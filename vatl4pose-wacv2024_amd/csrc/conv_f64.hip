// Float64 REFERENCE convolutions on v_mfma_f64_16x16x4_f64: one generic NHWC implicit GEMM (M = N*Ho*Wo pixels, N = Cout,
// K = R*S*Cin) that serves every conv of the three pose networks — the 3-channel stems, the 17-joint heads, the SE gates' Linear
// layers as 1x1 convs on 1x1 planes — and, as four 2x2 output phases, ConvTranspose2d(4,2,1).  It is the yardstick the fp32 routes
// are measured against, not a timed route: it feeds no FLOP meter, has no tuning knob and is never chosen by a product plan.
//   * operands are float64 (filters converted exactly from the module's fp32 tensors by the packers below);
//   * K runs in ONE fixed order — tap-major, channels ascending, sixteen at a time — with no split-K and no atomics; taps outside
//     the image and the padding of the last k-tile contribute exact zeros.  A pixel's bits therefore depend on its own receptive
//     field only: not on the batch it sits in, not on its place in a tile;
//   * write-out: fma(acc, scale[c], bias[c]) (+ residual) (ReLU), NHWC or NCHW.
// Block = 256 threads = 2 x 2 waves, tile 64 pixels x 64 channels, a wave owns 32 x 32 (2 x 2 MFMA tiles).  Both operands are staged
// through LDS one 16-deep k-tile at a time, the next tile's loads in flight while the current one is multiplied.  MFMA operands (one
// f64 per lane): A[row lane&15][k lane>>4], B[k lane>>4][col lane&15]; result col lane&15, row (lane>>4) + 4*reg (csrc/kmeans.hip).
#include "dgrad_phase.h"

namespace vatl {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kF64BM = 64, kF64BN = 64, kF64BK = 16;
constexpr int kF64Ld = kF64BM + 2;          // LDS row stride in doubles: the sixteen k-rows a staging store touches fall on different banks

__global__ __launch_bounds__(256) void conv_f64_kernel(const double* __restrict__ x, const double* __restrict__ w, const double* __restrict__ scale,
                                                       const double* __restrict__ bias, const double* __restrict__ residual, double* __restrict__ y,
                                                       ConvGeom g) {
    __shared__ double As[kF64BK][kF64Ld];
    __shared__ double Bs[kF64BK][kF64Ld];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const long long m0 = (long long)blockIdx.x * kF64BM;
    const int n0 = blockIdx.y * kF64BN;
    const int K = g.R * g.S * g.Cin;

    // staging: thread -> k column tid & 15 of the k-tile, rows / filters (tid >> 4) + 16 i
    const int kq = tid & 15, rq = tid >> 4;
    const double* xrow[4];
    int iy0[4], ix0[4];
    const double* wrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long m = m0 + rq + 16 * i;
        if (m < g.M) {
            const int ox = (int)(m % g.Wo);
            const long long t = m / g.Wo;
            const int oy = (int)(t % g.Ho);
            const long long n = t / g.Ho;
            xrow[i] = x + n * g.H * g.W * g.Cin;
            iy0[i] = oy * g.stride - g.pad_y;
            ix0[i] = ox * g.stride - g.pad_x;
        } else {
            xrow[i] = nullptr; iy0[i] = 0; ix0[i] = 0;
        }
        const int co = n0 + rq + 16 * i;
        wrow[i] = co < g.Cout ? w + (long long)co * K : nullptr;
    }
    // (r, s, c) of this thread's k, advanced by 16 per k-tile without a division
    int kc = kq % g.Cin, ktap = kq / g.Cin;
    int ks = ktap % g.S, kr = ktap / g.S;
    int k = kq;

    double ra[4], rb[4];
    auto fetch = [&]() {
        const bool kin = k < K;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int iy = iy0[i] + kr, ix = ix0[i] + ks;
            const bool ok = kin && xrow[i] && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
            ra[i] = ok ? xrow[i][((long long)iy * g.W + ix) * g.Cin + kc] : 0.0;
            rb[i] = kin && wrow[i] ? wrow[i][k] : 0.0;
        }
        k += kF64BK;
        kc += kF64BK;
        while (kc >= g.Cin) {
            kc -= g.Cin;
            if (++ks == g.S) { ks = 0; ++kr; }
        }
    };

    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};

    const int l16 = lane & 15, lg = lane >> 4;
    fetch();
    for (int k0 = 0; k0 < K; k0 += kF64BK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            As[kq][rq + 16 * i] = ra[i];
            Bs[kq][rq + 16 * i] = rb[i];
        }
        __syncthreads();
        if (k0 + kF64BK < K) fetch();
#pragma unroll
        for (int kk = 0; kk < kF64BK; kk += 4) {
            double av[2], bv[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) av[a] = As[kk + lg][wm * 32 + a * 16 + l16];
#pragma unroll
            for (int b = 0; b < 2; ++b) bv[b] = Bs[kk + lg][wn * 32 + b * 16 + l16];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }

    // write-out: lane holds channel col lane&15, pixels (lane>>4) + 4 reg of each 16 x 16 tile
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int c = n0 + wn * 32 + b * 16 + l16;
        if (c >= g.Cout) continue;
        const double sc = scale ? scale[c] : 1.0, bi = bias ? bias[c] : 0.0;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long m = m0 + wm * 32 + a * 16 + lg + 4 * r;
                if (m >= g.M) continue;
                const int ox = (int)(m % g.Wo);
                const long long t = m / g.Wo;
                const int oy = (int)(t % g.Ho);
                const long long n = t / g.Ho;
                const long long py = (long long)oy * g.osy + g.ooy, px = (long long)ox * g.osx + g.oox;
                const long long o = g.out_nchw ? ((n * g.Cout + c) * g.OH + py) * g.OW + px : ((n * g.OH + py) * g.OW + px) * g.Cout + c;
                double v = fma(acc[a][b][r], sc, bi);
                if (residual) v += residual[o];
                if (g.relu) v = fmax(v, 0.0);
                y[o] = v;
            }
    }
}

static int launch_conv_f64(const char* what, const double* x, const double* w, const double* scale, const double* bias, const double* residual, double* y,
                           const ConvGeom& g, int N, hipStream_t st) {
    if (g.M <= 0) return 0;
    const long long gx = (g.M + kF64BM - 1) / kF64BM;
    if (gx > 0x7FFFFFFFLL || (long long)N * g.OH * g.OW * g.Cout >= (1LL << 40) || (long long)N * g.H * g.W * g.Cin >= (1LL << 40))
        return fail(VATL_EINVAL, "%s: tensor too large", what);
    hipLaunchKernelGGL(conv_f64_kernel, dim3((unsigned)gx, (unsigned)cdiv(g.Cout, kF64BN)), dim3(256), 0, st, x, w, scale, bias, residual, y, g);
    return check_launch(what);
}

// OIHW fp32 -> [Cout][R][S][Cin] float64
__global__ void pack_conv_weight_f64_kernel(const float* __restrict__ src, double* __restrict__ dst, int Cout, int Cin, int R, int S) {
    const long long total = (long long)Cout * R * S * Cin;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        dst[i] = (double)src[conv_weight_src<false>(i, Cin, Cin, R, S)];
    }
}

// ConvTranspose2d(4,2,1) weight (Cin,Cout,4,4) fp32 -> [phase = py*2+px][Cout][ty][tx][Cin] float64, ky = 3-py-2ty, kx = 3-px-2tx
__global__ void pack_deconv_weight_f64_kernel(const float* __restrict__ src, double* __restrict__ dst, int Cin, int Cout) {
    const long long total = 16LL * Cout * Cin;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        dst[i] = (double)src[deconv_weight_src<false>(i, Cin, Cin, Cout)];
    }
}

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_pack_conv_weight_f64(const float* w_oihw, double* w_packed, int Cout, int Cin, int R, int S, void* stream) {
    if (!w_oihw || !w_packed || Cout < 1 || Cin < 1 || R < 1 || S < 1) return fail(VATL_EINVAL, "pack_conv_weight_f64: bad arguments");
    hipLaunchKernelGGL(pack_conv_weight_f64_kernel, dim3(pack_grid((long long)Cout * Cin * R * S)), dim3(256), 0, (hipStream_t)stream, w_oihw, w_packed, Cout, Cin, R, S);
    return check_launch("pack_conv_weight_f64");
}

extern "C" int vatl_pack_deconv4x4s2_weight_f64(const float* w_iohw, double* w_packed, int Cin, int Cout, void* stream) {
    if (!w_iohw || !w_packed || Cout < 1 || Cin < 1) return fail(VATL_EINVAL, "pack_deconv4x4s2_weight_f64: bad arguments");
    hipLaunchKernelGGL(pack_deconv_weight_f64_kernel, dim3(pack_grid(16LL * Cout * Cin)), dim3(256), 0, (hipStream_t)stream, w_iohw, w_packed, Cin, Cout);
    return check_launch("pack_deconv4x4s2_weight_f64");
}

extern "C" int vatl_conv2d_fwd_f64(const double* x, const double* w, const double* scale, const double* bias, const double* residual, double* y, int N, int H,
                                   int W, int Cin, int Cout, int R, int S, int stride, int pad, int relu, int out_nchw, void* stream) {
    if (!x || !w || !y) return fail(VATL_EINVAL, "conv2d_fwd_f64: null pointer");
    if (const int rc = conv_shape_contract("conv2d_fwd_f64", "->", false, N, H, W, Cin, Cout, R, S, stride, pad)) return rc;
    return launch_conv_f64("conv2d_fwd_f64", x, w, scale, bias, residual, y, conv_fwd_geom(N, H, W, Cin, Cout, R, S, stride, pad, relu, out_nchw), N,
                           (hipStream_t)stream);
}

extern "C" int vatl_deconv4x4s2_fwd_f64(const double* x, const double* w, const double* scale, const double* bias, double* y, int N, int H, int W, int Cin,
                                        int Cout, int relu, void* stream) {
    if (!x || !w || !y) return fail(VATL_EINVAL, "deconv4x4s2_fwd_f64: null pointer");
    if (N < 0 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return fail(VATL_EINVAL, "deconv4x4s2_fwd_f64: bad shape");
    for (int ph = 0; ph < 4; ++ph) {
        const int rc = launch_conv_f64("deconv4x4s2_fwd_f64", x, w + (long long)ph * Cout * 4 * Cin, scale, bias, nullptr, y,
                                       deconv_phase_geom(N, H, W, Cin, Cout, ph, relu), N, (hipStream_t)stream);
        if (rc) return rc;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------
// DATA GRADIENT of the float64 reference step (alphapose/models/hip_train_f64.py): dx = conv(dz, filter with the two channel counts
// exchanged), launch logic on conv_f64_kernel as it is — stride 1 is one launch with the flipped, transposed filter, stride 2 one
// launch per input-pixel phase that writes every other pixel (phase geometry: dgrad_phase.h).  The skip gradient of a bottleneck
// rides in the write-out's residual.  The data gradient of ConvTranspose2d(4,2,1) needs nothing new: it is vatl_conv2d_fwd_f64
// (4x4, stride 2, pad 1) of dz with vatl_pack_conv_weight_f64 applied to the (Cin,Cout,4,4) parameter as if it were OIHW.
namespace vatl {

// OIHW fp32 -> the phases one after the other, each [Cin][ty][tx][Cout] float64 (exact): the kernel's [rows][K] filter with rows = Cin
__global__ void pack_dgrad_weight_f64_kernel(const float* __restrict__ src, double* __restrict__ dst, int Cout, int Cin, int R, int S, int stride, int pad) {
    const long long cc = (long long)Cin * Cout;
    for (int phase = 0; phase < stride * stride; ++phase) {
        const DgradAxis ay = dgrad_axis(R, stride, pad, phase / stride), ax = dgrad_axis(S, stride, pad, phase % stride);
        double* out = dst + dgrad_phase_offset(R, S, stride, pad, phase, cc);
        const long long total = cc * ay.taps * ax.taps;
        for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
            out[i] = (double)src[dgrad_weight_src<false>(i, ay, ax, Cout, Cin, Cout, R, S, stride)];
        }
    }
}

// the pixels of a phase no tap reaches: dx = residual, or +0.0
__global__ void dgrad_fill_phase_f64_kernel(const double* __restrict__ residual, double* __restrict__ dx, long long N, int H, int W, int C, int stride, int py,
                                            int px, int Hp, int Wp) {
    const long long total = N * Hp * Wp * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long long t = i / C;
        const int jx = (int)(t % Wp); t /= Wp;
        const int jy = (int)(t % Hp);
        const long long o = (((t / Hp) * H + (long long)jy * stride + py) * W + (long long)jx * stride + px) * C + c;
        dx[o] = residual ? residual[o] : 0.0;
    }
}

}  // namespace vatl

extern "C" int vatl_pack_conv_weight_dgrad_f64(const float* w_oihw, double* w_packed, int Cout, int Cin, int R, int S, int stride, int pad, void* stream) {
    if (!w_oihw || !w_packed || Cout < 1 || Cin < 1 || R < 1 || S < 1 || R > 7 || S > 7 || (stride != 1 && stride != 2) || pad < 0)
        return fail(VATL_EINVAL, "pack_conv_weight_dgrad_f64: bad arguments");
    hipLaunchKernelGGL(pack_dgrad_weight_f64_kernel, dim3(pack_grid((long long)Cin * Cout * R * S)), dim3(256), 0, (hipStream_t)stream, w_oihw, w_packed, Cout, Cin,
                       R, S, stride, pad);
    return check_launch("pack_conv_weight_dgrad_f64");
}

extern "C" int vatl_conv2d_dgrad_f64(const double* dz, const double* w_dgrad, const double* residual, double* dx, int N, int H, int W, int Cin, int Cout, int R,
                                     int S, int stride, int pad, void* stream) {
    const char* what = "conv2d_dgrad_f64";
    if (!dz || !w_dgrad || !dx) return fail(VATL_EINVAL, "%s: null pointer", what);
    if (const int rc = conv_shape_contract(what, "<-", true, N, H, W, Cin, Cout, R, S, stride, pad)) return rc;
    if (N == 0) return 0;
    for (int phase = 0; phase < stride * stride; ++phase) {
        const DgradPhase p = dgrad_phase_geom(N, H, W, Cin, Cout, R, S, stride, pad, phase);
        if (p.Hp == 0 || p.Wp == 0) continue;
        if (p.ay.taps == 0 || p.ax.taps == 0) {
            hipLaunchKernelGGL(dgrad_fill_phase_f64_kernel, dim3(pack_grid((long long)N * p.Hp * p.Wp * Cin)), dim3(256), 0, (hipStream_t)stream, residual, dx,
                               (long long)N, H, W, Cin, stride, p.py, p.px, p.Hp, p.Wp);
            if (const int rc = check_launch(what)) return rc;
            continue;
        }
        if (const int rc = launch_conv_f64(what, dz, w_dgrad + p.w_off, nullptr, nullptr, residual, dx, p.g, N, (hipStream_t)stream)) return rc;
    }
    return 0;
}
