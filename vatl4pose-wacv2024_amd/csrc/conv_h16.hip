// Opt-in 16-bit inference convolutions on v_mfma_f32_16x16x32_{f16,bf16}: one generic NHWC implicit GEMM (M = N*Ho*Wo pixels,
// N = Cout, K = R*S*Cin) over a storage type T in {float16, bfloat16} that serves every conv of the three pose networks — the stems
// (3 channels padded to 8 by the input converter), the 17-joint heads, the SE gates' Linear layers as 1x1 convs on 1x1 planes — and,
// as four 2x2 output phases, ConvTranspose2d(4,2,1).  It stands beside the fp32 routes like conv_f64.hip does: it feeds no FLOP meter,
// has no tuning knob, reads no environment variable and is never chosen by a product plan.
//   * operands and stored activations are T; every product is accumulated in fp32 by the MFMA (a product of two T values is exact
//     in fp32);
//   * K runs in ONE fixed order — tap-major, channels ascending, 64 at a time — with no split-K and no atomics; taps outside the
//     image and the padding of the last k-tile contribute exact zeros.  A pixel's bits therefore depend on its own receptive field
//     only: not on the batch it sits in, not on its place in a tile;
//   * write-out in fp32: fmaf(acc, scale[c], bias[c]) (+ residual, stored as T) (ReLU), rounded ONCE to T (NHWC), or left fp32 and
//     stored NCHW for the heads and whatever a scorer reads.
// Contract: Cin % 8 == 0 (a lane's eight k-elements are one 16-byte load and never straddle a tap), Cout % 8 == 0 for T output, any
// Cout for fp32 NCHW output; everything else is refused before a launch.
// Block = 256 threads = 2 x 2 waves, tile 128 pixels x BN channels (BN = 128, or 64 for the narrow layers: the same template), a wave
// owns 64 pixels x BN/2 channels.  The filter is the MFMA's A operand and the pixels its B operand, and the filters are staged in LDS in
// MFMA-row order, so a lane ends up with BN/8 CONSECUTIVE channels of one pixel: 16-byte NHWC residual loads and stores (128 contiguous
// bytes per pixel and wave), or sixteen lanes on sixteen consecutive pixels of an NCHW plane.
// Both operands go global -> registers (16-byte loads) -> LDS one 64-deep k-tile at a time, the next tile's loads in flight while the
// current one is multiplied.  LDS rows are padded from 128 to 144 bytes: the sixteen rows a fragment read touches at one k-group fall
// on sixteen different 16-byte bank groups.
// Operand lane maps: A[row lane&15][k 8(lane>>4)+j], B[k 8(lane>>4)+j][col lane&15]; result col lane&15, row 4(lane>>4)+reg.
#include "dgrad_phase.h"
#include "h16.h"

namespace vatl {

constexpr int kH16BM = 128, kH16BK = 64;
constexpr int kH16Ld = kH16BK + 8;              // LDS row stride in elements (144 bytes)

template <typename T, int BN>
__global__ __launch_bounds__(256) void conv_h16_kernel(const unsigned short* __restrict__ x, const unsigned short* __restrict__ w,
                                                       const float* __restrict__ scale, const float* __restrict__ bias,
                                                       const unsigned short* __restrict__ residual, void* __restrict__ y, ConvGeom g) {
    constexpr int NB = BN / 32;                 // filters staged per thread
    constexpr int CT = BN / 32, PT = 4;         // 16 x 16 MFMA tiles of a wave: channels x pixels
    constexpr int HB = BN / 2;                  // channels of a wave
    static_assert(CT >= 2 && CT % 2 == 0, "a lane stores whole groups of eight channels");
    __shared__ __attribute__((aligned(16))) unsigned short Xs[kH16BM][kH16Ld];
    __shared__ __attribute__((aligned(16))) unsigned short Ws[BN][kH16Ld];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const long long m0 = (long long)blockIdx.x * kH16BM;
    const int n0 = blockIdx.y * BN;
    const int K = g.R * g.S * g.Cin;

    // staging: thread -> k-group tid & 7 (eight elements, one tap) of the k-tile, pixels / filters (tid >> 3) + 32 i
    const int gq = tid & 7, rq = tid >> 3;
    const unsigned short* xrow[4];
    int iy0[4], ix0[4];
    const unsigned short* wrow[NB];
    int wlds[NB];                               // LDS row of staged filter i (see the write-out for the order)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long m = m0 + rq + 32 * i;
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
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int f = rq + 32 * i, co = n0 + f;
        wrow[i] = co < g.Cout ? w + (long long)co * K : nullptr;
        // Filters sit in LDS in MFMA-row order: channel ch = q * 4CT + 4a + r of a wave's half goes to row 16a + 4q + r, so that result
        // register r of tile a in lane group q is channel q * 4CT + 4a + r — a lane ends up with 4CT CONSECUTIVE channels of its pixel.
        const int ch = f % HB;
        wlds[i] = f - ch + ((ch % (4 * CT)) >> 2) * 16 + (ch / (4 * CT)) * 4 + (ch & 3);
    }
    // (r, s, c) of this thread's k-group, advanced by 64 per k-tile without a division
    int k = 8 * gq;
    int kc = k % g.Cin, ktap = k / g.Cin;
    int ks = ktap % g.S, kr = ktap / g.S;

    const h16_u32x4 zero = {0u, 0u, 0u, 0u};
    h16_u32x4 ra[4], rb[NB];
    auto fetch = [&]() {
        const bool kin = k < K;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int iy = iy0[i] + kr, ix = ix0[i] + ks;
            const bool ok = kin && xrow[i] && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
            ra[i] = ok ? *reinterpret_cast<const h16_u32x4*>(xrow[i] + ((long long)iy * g.W + ix) * g.Cin + kc) : zero;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) rb[i] = kin && wrow[i] ? *reinterpret_cast<const h16_u32x4*>(wrow[i] + k) : zero;
        k += kH16BK;
        kc += kH16BK;
        while (kc >= g.Cin) {
            kc -= g.Cin;
            if (++ks == g.S) { ks = 0; ++kr; }
        }
    };

    h16_f32x4 acc[CT][PT];
#pragma unroll
    for (int a = 0; a < CT; ++a)
#pragma unroll
        for (int b = 0; b < PT; ++b) acc[a][b] = (h16_f32x4){0.f, 0.f, 0.f, 0.f};

    const int l16 = lane & 15, lg = lane >> 4;
    fetch();
    for (int k0 = 0; k0 < K; k0 += kH16BK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<h16_u32x4*>(&Xs[rq + 32 * i][8 * gq]) = ra[i];
#pragma unroll
        for (int i = 0; i < NB; ++i) *reinterpret_cast<h16_u32x4*>(&Ws[wlds[i]][8 * gq]) = rb[i];
        __syncthreads();
        if (k0 + kH16BK < K) fetch();
#pragma unroll
        for (int step = 0; step < kH16BK / 32; ++step) {
            const int kg = 8 * (4 * step + lg);
            h16_u32x4 af[CT], bf[PT];
#pragma unroll
            for (int a = 0; a < CT; ++a) af[a] = *reinterpret_cast<const h16_u32x4*>(&Ws[wn * (BN / 2) + a * 16 + l16][kg]);
#pragma unroll
            for (int b = 0; b < PT; ++b) bf[b] = *reinterpret_cast<const h16_u32x4*>(&Xs[wm * 64 + b * 16 + l16][kg]);
#pragma unroll
            for (int a = 0; a < CT; ++a)
#pragma unroll
                for (int b = 0; b < PT; ++b) acc[a][b] = T::mfma(af[a], bf[b], acc[a][b]);
        }
        __syncthreads();
    }

    // write-out: lane holds pixel lane&15 and the 4CT consecutive channels cbase .. of its lane group (tile a, register r = channel cbase + 4a + r):
    // 16-byte residual loads and stores, 128 contiguous bytes per pixel and wave on the wide tile
    const int cbase = n0 + wn * HB + lg * (4 * CT);
#pragma unroll
    for (int b = 0; b < PT; ++b) {
        const long long m = m0 + wm * 64 + b * 16 + l16;
        if (m >= g.M || cbase >= g.Cout) continue;
        const int ox = (int)(m % g.Wo);
        const long long t = m / g.Wo;
        const int oy = (int)(t % g.Ho);
        const long long n = t / g.Ho;
        const long long py = (long long)oy * g.osy + g.ooy, px = (long long)ox * g.osx + g.oox;
        const long long pix = (n * g.OH + py) * g.OW + px;
        float v[4 * CT];
#pragma unroll
        for (int e = 0; e < 4 * CT; ++e) {
            const bool in = cbase + e < g.Cout;
            const float sc = scale && in ? scale[cbase + e] : 1.f, bi = bias && in ? bias[cbase + e] : 0.f;
            v[e] = fmaf(acc[e >> 2][b][e & 3], sc, bi);
        }
        if (g.out_nchw) {
            float* yf = reinterpret_cast<float*>(y);
#pragma unroll
            for (int e = 0; e < 4 * CT; ++e) {
                if (cbase + e >= g.Cout) continue;
                float o = v[e];
                if (residual) o += T::to_f32(residual[pix * g.Cout + cbase + e]);
                yf[((n * g.Cout + cbase + e) * g.OH + py) * g.OW + px] = g.relu ? fmaxf(o, 0.f) : o;
            }
        } else {                                // Cout % 8 == 0 and cbase % 8 == 0: whole groups of eight channels, 16-byte aligned
#pragma unroll
            for (int j = 0; j < CT / 2; ++j) {
                if (cbase + 8 * j >= g.Cout) continue;
                const long long o = pix * g.Cout + cbase + 8 * j;
                if (residual) {
                    float rf[8];
                    h16_unpack8<T>(*reinterpret_cast<const uint4*>(residual + o), rf);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[8 * j + e] += rf[e];
                }
                if (g.relu) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[8 * j + e] = fmaxf(v[8 * j + e], 0.f);
                }
                *reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(y) + o) = h16_pack8<T>(v + 8 * j);
            }
        }
    }
}

template <typename T>
static void launch_conv_h16_t(const void* x, const void* w, const float* scale, const float* bias, const void* residual, void* y, const ConvGeom& g,
                              hipStream_t st) {
    const unsigned gx = (unsigned)((g.M + kH16BM - 1) / kH16BM);
    const unsigned short *xs = (const unsigned short*)x, *ws = (const unsigned short*)w, *rs = (const unsigned short*)residual;
    if (g.Cout <= 64)                           // the narrow layers (17, 32, 64 channels) do not pay for a 128-wide channel tile
        hipLaunchKernelGGL((conv_h16_kernel<T, 64>), dim3(gx, (unsigned)cdiv(g.Cout, 64)), dim3(256), 0, st, xs, ws, scale, bias, rs, y, g);
    else
        hipLaunchKernelGGL((conv_h16_kernel<T, 128>), dim3(gx, (unsigned)cdiv(g.Cout, 128)), dim3(256), 0, st, xs, ws, scale, bias, rs, y, g);
}

static int launch_conv_h16(const char* what, const void* x, const void* w, const float* scale, const float* bias, const void* residual, void* y,
                           const ConvGeom& g, int N, int dtype, hipStream_t st) {
    if (g.M <= 0) return 0;
    const long long gx = (g.M + kH16BM - 1) / kH16BM;
    if (gx > 0x7FFFFFFFLL || (long long)N * g.OH * g.OW * g.Cout >= (1LL << 40) || (long long)N * g.H * g.W * g.Cin >= (1LL << 40))
        return fail(VATL_EINVAL, "%s: tensor too large", what);
    if (dtype == kH16F16) launch_conv_h16_t<F16>(x, w, scale, bias, residual, y, g, st);
    else launch_conv_h16_t<BF16>(x, w, scale, bias, residual, y, g, st);
    return check_launch(what);
}

// what every conv entry point refuses before anything is launched
static int conv_h16_contract(const char* what, const void* x, const void* w, const void* residual, const void* y, int Cin, int Cout, int out_f32_nchw,
                             int dtype) {
    if (!x || !w || !y) return fail(VATL_EINVAL, "%s: null pointer", what);
    if (!h16_dtype_ok(dtype)) return fail(VATL_EINVAL, "%s: dtype %d is neither float16 (0) nor bfloat16 (1)", what, dtype);
    if (Cin < 8 || (Cin & 7)) return fail(VATL_EINVAL, "%s: Cin %d is not a multiple of 8 (pad the input and the filter with zero channels)", what, Cin);
    if (Cout < 1 || (!out_f32_nchw && (Cout & 7)))
        return fail(VATL_EINVAL, "%s: Cout %d is not a multiple of 8: only the fp32 NCHW write-out serves it", what, Cout);
    if (!h16_aligned16(x) || !h16_aligned16(w) || !h16_aligned16(residual) || (reinterpret_cast<uintptr_t>(y) & (out_f32_nchw ? 3u : 15u)))
        return fail(VATL_EINVAL, "%s: 16-bit tensors must be 16-byte aligned", what);
    return 0;
}

// OIHW fp32 -> [Cout][R][S][Cin8] T, the channels Cin .. Cin8-1 zero
template <typename T>
__global__ void pack_conv_weight_h16_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, int Cout, int Cin, int Cin8, int R, int S) {
    const long long total = (long long)Cout * R * S * Cin8;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long j = conv_weight_src<true>(i, Cin, Cin8, R, S);
        dst[i] = j >= 0 ? T::from_f32(src[j]) : (unsigned short)0;
    }
}

// ConvTranspose2d(4,2,1) weight (Cin,Cout,4,4) fp32 -> [phase = py*2+px][Cout][ty][tx][Cin8] T, ky = 3-py-2ty, kx = 3-px-2tx
template <typename T>
__global__ void pack_deconv_weight_h16_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, int Cin, int Cin8, int Cout) {
    const long long total = 16LL * Cout * Cin8;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long j = deconv_weight_src<true>(i, Cin, Cin8, Cout);
        dst[i] = j >= 0 ? T::from_f32(src[j]) : (unsigned short)0;
    }
}

// DATA GRADIENT of the bf16 fine-tune step: dx = conv(dz, filter with the two channel counts exchanged), on conv_h16_kernel as it is.
// The phase geometry (dgrad_phase.h) is shared with the float64 reference.
template <typename T>
__global__ void pack_dgrad_weight_h16_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, int Cout, int Cin, int Cout8, int Cin8, int R, int S,
                                             int stride, int pad) {
    const long long cc = (long long)Cin8 * Cout8;
    for (int phase = 0; phase < stride * stride; ++phase) {
        const DgradAxis ay = dgrad_axis(R, stride, pad, phase / stride), ax = dgrad_axis(S, stride, pad, phase % stride);
        unsigned short* out = dst + dgrad_phase_offset(R, S, stride, pad, phase, cc);
        const long long total = cc * ay.taps * ax.taps;
        for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
            const long long j = dgrad_weight_src<true>(i, ay, ax, Cout, Cin, Cout8, R, S, stride);
            out[i] = j >= 0 ? T::from_f32(src[j]) : (unsigned short)0;
        }
    }
}

// the pixels of a phase no tap reaches: dx = residual, or +0.0 (eight channels per thread)
__global__ void dgrad_fill_phase_h16_kernel(const uint4* __restrict__ residual, uint4* __restrict__ dx, long long N, int H, int W, int G, int stride, int py,
                                            int px, int Hp, int Wp) {
    const long long total = N * Hp * Wp * G;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int gq = (int)(i % G);
        long long t = i / G;
        const int jx = (int)(t % Wp); t /= Wp;
        const int jy = (int)(t % Hp);
        const long long o = (((t / Hp) * H + (long long)jy * stride + py) * W + (long long)jx * stride + px) * G + gq;
        dx[o] = residual ? residual[o] : make_uint4(0u, 0u, 0u, 0u);
    }
}

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_pack_conv_weight_h16(const float* w_oihw, void* w_packed, int Cout, int Cin, int R, int S, int dtype, void* stream) {
    if (!w_oihw || !w_packed || Cout < 1 || Cin < 1 || R < 1 || S < 1 || !h16_dtype_ok(dtype)) return fail(VATL_EINVAL, "pack_conv_weight_h16: bad arguments");
    const int Cin8 = (Cin + 7) & ~7;
    const auto kernel = dtype == kH16F16 ? pack_conv_weight_h16_kernel<F16> : pack_conv_weight_h16_kernel<BF16>;
    hipLaunchKernelGGL(kernel, dim3(pack_grid((long long)Cout * Cin8 * R * S)), dim3(256), 0, (hipStream_t)stream, w_oihw, (unsigned short*)w_packed, Cout, Cin, Cin8, R,
                       S);
    return check_launch("pack_conv_weight_h16");
}

extern "C" int vatl_pack_deconv4x4s2_weight_h16(const float* w_iohw, void* w_packed, int Cin, int Cout, int dtype, void* stream) {
    if (!w_iohw || !w_packed || Cout < 1 || Cin < 1 || !h16_dtype_ok(dtype)) return fail(VATL_EINVAL, "pack_deconv4x4s2_weight_h16: bad arguments");
    const int Cin8 = (Cin + 7) & ~7;
    const auto kernel = dtype == kH16F16 ? pack_deconv_weight_h16_kernel<F16> : pack_deconv_weight_h16_kernel<BF16>;
    hipLaunchKernelGGL(kernel, dim3(pack_grid(16LL * Cout * Cin8)), dim3(256), 0, (hipStream_t)stream, w_iohw, (unsigned short*)w_packed, Cin, Cin8, Cout);
    return check_launch("pack_deconv4x4s2_weight_h16");
}

extern "C" int vatl_conv2d_fwd_h16(const void* x, const void* w, const float* scale, const float* bias, const void* residual, void* y, int N, int H, int W,
                                   int Cin, int Cout, int R, int S, int stride, int pad, int relu, int out_f32_nchw, int dtype, void* stream) {
    if (const int rc = conv_h16_contract("conv2d_fwd_h16", x, w, residual, y, Cin, Cout, out_f32_nchw != 0, dtype)) return rc;
    if (const int rc = conv_shape_contract("conv2d_fwd_h16", "->", false, N, H, W, Cin, Cout, R, S, stride, pad)) return rc;
    return launch_conv_h16("conv2d_fwd_h16", x, w, scale, bias, residual, y, conv_fwd_geom(N, H, W, Cin, Cout, R, S, stride, pad, relu, out_f32_nchw), N, dtype,
                           (hipStream_t)stream);
}

extern "C" int vatl_deconv4x4s2_fwd_h16(const void* x, const void* w, const float* scale, const float* bias, void* y, int N, int H, int W, int Cin, int Cout,
                                        int relu, int dtype, void* stream) {
    if (const int rc = conv_h16_contract("deconv4x4s2_fwd_h16", x, w, nullptr, y, Cin, Cout, 0, dtype)) return rc;
    if (N < 0 || H < 1 || W < 1) return fail(VATL_EINVAL, "deconv4x4s2_fwd_h16: bad shape");
    for (int ph = 0; ph < 4; ++ph) {
        const int rc = launch_conv_h16("deconv4x4s2_fwd_h16", x, (const unsigned short*)w + (long long)ph * Cout * 4 * Cin, scale, bias, nullptr, y,
                                       deconv_phase_geom(N, H, W, Cin, Cout, ph, relu), N, dtype, (hipStream_t)stream);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int vatl_pack_conv_weight_dgrad_h16(const float* w_oihw, void* w_packed, int Cout, int Cin, int R, int S, int stride, int pad, int dtype, void* stream) {
    if (!w_oihw || !w_packed || Cout < 1 || Cin < 1 || R < 1 || S < 1 || R > 7 || S > 7 || (stride != 1 && stride != 2) || pad < 0 || !h16_dtype_ok(dtype))
        return fail(VATL_EINVAL, "pack_conv_weight_dgrad_h16: bad arguments");
    const int Cin8 = (Cin + 7) & ~7, Cout8 = (Cout + 7) & ~7;
    const auto kernel = dtype == kH16F16 ? pack_dgrad_weight_h16_kernel<F16> : pack_dgrad_weight_h16_kernel<BF16>;
    hipLaunchKernelGGL(kernel, dim3(pack_grid((long long)Cin8 * Cout8 * R * S)), dim3(256), 0, (hipStream_t)stream, w_oihw, (unsigned short*)w_packed, Cout, Cin, Cout8,
                       Cin8, R, S, stride, pad);
    return check_launch("pack_conv_weight_dgrad_h16");
}

extern "C" int vatl_conv2d_dgrad_h16(const void* dz, const void* w_dgrad, const void* residual, void* dx, int N, int H, int W, int Cin8, int Cout8, int R, int S,
                                     int stride, int pad, int dtype, void* stream) {
    const char* what = "conv2d_dgrad_h16";
    // roles on the kernel: dz is the input (Cout8 channels), dx the output (Cin8 channels)
    if (const int rc = conv_h16_contract(what, dz, w_dgrad, residual, dx, Cout8, Cin8, 0, dtype)) return rc;
    if (const int rc = conv_shape_contract(what, nullptr, true, N, H, W, Cin8, Cout8, R, S, stride, pad)) return rc;
    if (N == 0) return 0;
    for (int phase = 0; phase < stride * stride; ++phase) {
        const DgradPhase p = dgrad_phase_geom(N, H, W, Cin8, Cout8, R, S, stride, pad, phase);
        if (p.Hp == 0 || p.Wp == 0) continue;
        if (p.ay.taps == 0 || p.ax.taps == 0) {
            const long long total = (long long)N * p.Hp * p.Wp * (Cin8 >> 3);
            hipLaunchKernelGGL(dgrad_fill_phase_h16_kernel, dim3(pack_grid(total)), dim3(256), 0, (hipStream_t)stream, (const uint4*)residual, (uint4*)dx,
                               (long long)N, H, W, Cin8 >> 3, stride, p.py, p.px, p.Hp, p.Wp);
            if (const int rc = check_launch(what)) return rc;
            continue;
        }
        if (const int rc = launch_conv_h16(what, dz, (const unsigned short*)w_dgrad + p.w_off, nullptr, nullptr, residual, dx, p.g, N, dtype, (hipStream_t)stream))
            return rc;
    }
    return 0;
}
