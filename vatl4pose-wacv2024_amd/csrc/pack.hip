// Weight packs and parameter folding: OIHW parameters -> the layouts the conv kernels read.  Every layout has ONE index formula
// (pack_conv_elem, pack_deconv_elem, pack_dgrad_tile; the Winograd transforms live in winograd_pack.h), called by the per-tensor
// entry points and by the table-driven launch that re-packs every weight of a fine-tune step at once, so both write the same copies.
#include "glue_common.h"
#include "winograd_pack.h"

namespace vatl {

// element i of the forward layout [CoutPad][R][Spad][CinPad] of a (Cout, Cin, R, S) filter; padding is zero.  I: the index type
// (the multi launch keeps to 32-bit arithmetic)
template <class I>
__device__ __forceinline__ float pack_conv_elem(const float* __restrict__ w, I i, int Cout, int Cin, int R, int S, int Spad, int CinPad) {
    const I c = i % (I)CinPad;
    I t = i / (I)CinPad;
    const I s = t % (I)Spad; t /= (I)Spad;
    const I r = t % (I)R;
    const I o = t / (I)R;
    float v = 0.f;
    if ((int)o < Cout && (int)s < S && (int)c < Cin) v = w[(((long long)o * Cin + c) * R + r) * S + s];
    return v;
}

// element i of the ConvTranspose2d(4,2,1) layout [phase][CoutPad][ty][tx][Cin] of a (Cin, Cout, 4, 4) filter
template <class I>
__device__ __forceinline__ float pack_deconv_elem(const float* __restrict__ w, I i, int Cin, int Cout, int CoutPad) {
    const I c = i % (I)Cin;
    I t = i / (I)Cin;
    const int tx = (int)(t & 1); t >>= 1;
    const int ty = (int)(t & 1); t >>= 1;
    const I o = t % (I)CoutPad;
    const int ph = (int)(t / (I)CoutPad);
    const int ky = 3 - (ph >> 1) - 2 * ty, kx = 3 - (ph & 1) - 2 * tx;
    float v = 0.f;
    if ((int)o < Cout) v = w[(((long long)c * Cout + o) * 4 + ky) * 4 + kx];
    return v;
}

// data-gradient layout out[c][t][n] = w[n][c][tap t] ([CinPad][ntaps][CoutK], zero outside Cin x Cout) = a transpose of OIHW: a block
// makes one 32 (input channels) x 32 (output channels) tile of one tap through LDS, so that reads run along the input channels of a filter
// row and writes along the output channels (one element per thread read a different cache line per lane: 305 us of the R50 step).
struct DgradTile { unsigned n_t, tp, c_t; };
__device__ __forceinline__ DgradTile dgrad_tile(unsigned bl, int CoutK, int ntaps) {
    const unsigned tiles_n = (unsigned)(CoutK + 31) >> 5;
    const unsigned t = bl / tiles_n;
    return {bl % tiles_n, t % (unsigned)ntaps, t / (unsigned)ntaps};
}
// tap = r * S + s of tap index T.tp
__device__ __forceinline__ void pack_dgrad_tile(const float* __restrict__ w, float* __restrict__ out, int Cout, int Cin, int RS, int tap, int CinPad, int CoutK,
                                                int ntaps, DgradTile T) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int n = (int)T.n_t * 32 + ty + 8 * k, c = (int)T.c_t * 32 + tx;
        tile[ty + 8 * k][tx] = (c < Cin && n < Cout) ? w[((size_t)n * Cin + c) * RS + tap] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = (int)T.c_t * 32 + ty + 8 * k, n = (int)T.n_t * 32 + tx;
        if (c < CinPad && n < CoutK) out[((size_t)c * ntaps + T.tp) * CoutK + n] = tile[tx][ty + 8 * k];
    }
}

__global__ void pack_conv_weight_kernel(const float* __restrict__ w, float* __restrict__ out, int Cout, int Cin, int R, int S,
                                        int CoutPad, int Spad, int CinPad) {
    const long long total = (long long)CoutPad * R * Spad * CinPad;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        out[i] = pack_conv_elem<long long>(w, i, Cout, Cin, R, S, Spad, CinPad);
}

__global__ void pack_deconv_weight_kernel(const float* __restrict__ w, float* __restrict__ out, int Cin, int Cout, int CoutPad) {
    const long long total = 4LL * CoutPad * 4 * Cin;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        out[i] = pack_deconv_elem<long long>(w, i, Cin, Cout, CoutPad);
}

struct TapList { int r[16]; int s[16]; int n; };
__global__ __launch_bounds__(256) void pack_dgrad_weight_kernel(const float* __restrict__ w, float* __restrict__ out, int Cout, int Cin, int R, int S,
                                                                int CinPad, int CoutK, TapList taps) {
    const DgradTile T = dgrad_tile(blockIdx.x, CoutK, taps.n);
    pack_dgrad_tile(w, out, Cout, Cin, R * S, taps.r[T.tp] * S + taps.s[T.tp], CinPad, CoutK, taps.n, T);
}

// dual-source 1x1: out[o][k] = w1[o][k] * s1[o] (k < C1) | w2[o][k - C1] * s2[o]; rows o >= Cout zero; bias = b1 + b2
__global__ void pack_dual_weight_kernel(const float* __restrict__ w1, const float* __restrict__ s1, const float* __restrict__ b1,
                                        const float* __restrict__ w2, const float* __restrict__ s2, const float* __restrict__ b2,
                                        float* __restrict__ out, float* __restrict__ bias, int Cout, int C1, int C2, int CoutPad) {
    const int K = C1 + C2;
    const long long total = (long long)CoutPad * K;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i % K), o = (int)(i / K);
        float v = 0.f;
        if (o < Cout) v = k < C1 ? w1[(long long)o * C1 + k] * s1[o] : w2[(long long)o * C2 + (k - C1)] * s2[o];
        out[i] = v;
        if (k == 0 && o < Cout) bias[o] = b1[o] + b2[o];
    }
}

__global__ void bn_fold_kernel(const float* gamma, const float* beta, const float* mean, const float* var, const float* cbias,
                               float eps, float* scale, float* bias, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float s = 1.f, b = 0.f;
    if (var) {
        s = (gamma ? gamma[c] : 1.f) / sqrtf(var[c] + eps);
        b = (beta ? beta[c] : 0.f) - mean[c] * s;
    }
    if (cbias) b += cbias[c] * s;
    scale[c] = s;
    bias[c] = b;
}

// F(4x3,2x2) phase filters of ConvTranspose2d(4,2,1) (winograd_pack.h).  Inference only: the plans pack it once per weight version, so it has
// no kind in the table-driven launch below.
__global__ __launch_bounds__(256) void wino43_pack_kernel(const float* __restrict__ w, float* __restrict__ out, int Cout, int Cin) {
    wino43_pack_block(w, out, Cout, Cin, blockIdx.x, threadIdx.x);
}

// F(4x3,2x2) phase filters of the 3x3 / stride 2 conv (winograd_pack.h), inference only like the one above.
__global__ __launch_bounds__(256) void wino_s2_43_pack_kernel(const float* __restrict__ w, float* __restrict__ out, int Cout, int Cin) {
    wino_s2_43_pack_block(w, out, Cout, Cin, blockIdx.x, threadIdx.x);
}

// Every weight re-pack of a fine-tune step in ONE launch (the trainers need ~60 .. 180 packed copies per step — forward
// layouts of the 3x3 / 7x7 / transposed convs, data-gradient layouts of every conv — and each used to be its own 5 us
// launch).  jobs: device array sorted by first_block; a block of 256 threads makes 1024 consecutive elements of one job (kinds 0 / 2),
// one 32 x 32 tile of one tap (kind 1) or 4096 elements of a Winograd filter transform (kinds 3 .. 6).
__global__ __launch_bounds__(256) void pack_multi_kernel(const VatlPackJob* __restrict__ jobs, int njobs) {
    __shared__ int sj;
    if (threadIdx.x == 0) {
        int lo = 0, hi = njobs - 1;
        const long long b = blockIdx.x;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (jobs[mid].first_block <= b) lo = mid; else hi = mid - 1;
        }
        sj = lo;
    }
    __syncthreads();
    const VatlPackJob* J = jobs + sj;
    const float* __restrict__ w = J->src;
    float* __restrict__ out = J->dst;
    const int kind = J->kind, Cout = J->Cout, Cin = J->Cin, R = J->R, S = J->S, pa = J->a, pb = J->b, pc = J->c;
    if (kind >= 7) {                                               // 7 / 8: F(4x4,3x3) filter transform, forward / data gradient; c = inner dimension of src; 256 items per block
        f4_pack_item(w, out, kind - 7, pc, Cout, Cin, ((long long)blockIdx.x - J->first_block) * 256 + threadIdx.x);
        return;
    }
    if (kind >= 3) {                                               // 3 / 4 / 5: Winograd filter transforms (forward, data gradient, transposed conv); b = NH, c = w_i
        wino_pack_block(w, out, kind - 3, pc, Cout, Cin, pb, (long long)blockIdx.x - J->first_block, threadIdx.x);   // 4096 elements per block
        return;
    }
    const unsigned bl = (unsigned)((long long)blockIdx.x - J->first_block);
    if (kind == 1) {                                               // data-gradient layout: (a, b, c) = (CinPad, CoutK, ntaps)
        const DgradTile T = dgrad_tile(bl, pb, pc);
        pack_dgrad_tile(w, out, Cout, Cin, R * S, J->tap_r[T.tp] * S + J->tap_s[T.tp], pa, pb, pc, T);
        return;
    }
    // kinds 0 / 2 (forward layouts of the strided 3x3 / 7x7 convs and of the implicit-GEMM transposed convs): a few layers; 32-bit index arithmetic
    const unsigned base = bl * 1024u;
    const unsigned total = kind == 0 ? (unsigned)pa * R * pb * pc       // (a, b, c) = (CoutPad, Spad, CinPad)
                                     : 16u * pa * Cin;                  // a = CoutPad
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned i = base + e * 256 + threadIdx.x;
        if (i >= total) continue;
        out[i] = kind == 0 ? pack_conv_elem<unsigned>(w, i, Cout, Cin, R, S, pb, pc) : pack_deconv_elem<unsigned>(w, i, Cin, Cout, pa);
    }
}

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_pack_conv_weight(const float* w, float* out, int Cout, int Cin, int R, int S, int CoutPad, int Spad, int CinPad, void* stream) {
    if (!w || !out || CoutPad < Cout || Spad < S || CinPad < Cin) return fail(VATL_EINVAL, "pack_conv_weight: bad arguments");
    hipLaunchKernelGGL(pack_conv_weight_kernel, dim3(ew_grid((long long)CoutPad * R * Spad * CinPad)), dim3(256), 0, (hipStream_t)stream,
                       w, out, Cout, Cin, R, S, CoutPad, Spad, CinPad);
    return check_launch("pack_conv_weight");
}

extern "C" int vatl_pack_conv1x1_dual_weight(const float* w1, const float* scale1, const float* bias1, const float* w2, const float* scale2,
                                             const float* bias2, float* out, float* bias, int Cout, int C1, int C2, int CoutPad, void* stream) {
    if (!w1 || !scale1 || !bias1 || !w2 || !scale2 || !bias2 || !out || !bias || CoutPad < Cout) return fail(VATL_EINVAL, "pack_conv1x1_dual_weight: bad arguments");
    hipLaunchKernelGGL(pack_dual_weight_kernel, dim3(ew_grid((long long)CoutPad * (C1 + C2))), dim3(256), 0, (hipStream_t)stream, w1, scale1, bias1, w2,
                       scale2, bias2, out, bias, Cout, C1, C2, CoutPad);
    return check_launch("pack_conv1x1_dual_weight");
}

extern "C" int vatl_pack_deconv4x4s2_weight(const float* w, float* out, int Cin, int Cout, int CoutPad, void* stream) {
    if (!w || !out || CoutPad < Cout) return fail(VATL_EINVAL, "pack_deconv4x4s2_weight: bad arguments");
    hipLaunchKernelGGL(pack_deconv_weight_kernel, dim3(ew_grid(16LL * CoutPad * Cin)), dim3(256), 0, (hipStream_t)stream, w, out, Cin, Cout, CoutPad);
    return check_launch("pack_deconv4x4s2_weight");
}

// ConvTranspose2d(4, 2, 1) filter (Cin, Cout, 4, 4) -> four phase filters G4 g_phase G3^T of 20 positions each
extern "C" int64_t vatl_winograd_deconv43_weight_floats(int Cout, int Cin) { return 4LL * 20 * Cout * Cin; }

extern "C" int vatl_pack_winograd_deconv43_weight(const float* w, float* u, int Cout, int Cin, void* stream) {
    if (!w || !u || Cout <= 0 || Cin <= 0) return fail(VATL_EINVAL, "pack_winograd_deconv43_weight: null pointer or empty filter");
    if (Cin % 16 != 0 || Cout % 64 != 0) return fail(VATL_EINVAL, "pack_winograd_deconv43_weight: Cin %d must be a multiple of 16 and Cout %d of 64", Cin, Cout);
    const long long blocks = 4LL * (Cout / 32) * (Cin / 8);
    if (blocks > 0x7FFFFFFF) return fail(VATL_EINVAL, "pack_winograd_deconv43_weight: filter too large");
    hipLaunchKernelGGL(wino43_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, u, Cout, Cin);
    return check_launch("wino43_pack");
}

// 3x3 / stride 2 / pad 1 filter (Cout, Cin, 3, 3) -> its four input-phase filters G4 g_phase G3^T: 20 positions for the two by = 0 phases, 16 for the two by = 1
extern "C" int64_t vatl_winograd_s2_43_weight_floats(int Cout, int Cin) { return 72LL * Cout * Cin; }

extern "C" int vatl_pack_winograd_s2_43_weight(const float* w, float* u, int Cout, int Cin, void* stream) {
    if (!w || !u || Cout <= 0 || Cin <= 0) return fail(VATL_EINVAL, "pack_winograd_s2_43_weight: null pointer or empty filter");
    if (Cin % 16 != 0 || Cout % 64 != 0) return fail(VATL_EINVAL, "pack_winograd_s2_43_weight: Cin %d must be a multiple of 16 and Cout %d of 64", Cin, Cout);
    const long long blocks = 4LL * (Cout / 32) * (Cin / 8);
    if (blocks > 0x7FFFFFFF) return fail(VATL_EINVAL, "pack_winograd_s2_43_weight: filter too large");
    hipLaunchKernelGGL(wino_s2_43_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, u, Cout, Cin);
    return check_launch("wino_s2_43_pack");
}

extern "C" int vatl_pack_dgrad_weight(const float* w_oihw, float* out, int Cout, int Cin, int R, int S, int CinPad, int CoutK,
                                      int ntaps, const int* tap_r, const int* tap_s, void* stream) {
    if (!w_oihw || !out || !tap_r || !tap_s || ntaps < 1 || ntaps > 16 || CinPad < Cin || CoutK < Cout) return fail(VATL_EINVAL, "pack_dgrad_weight: bad arguments");
    TapList t{};
    t.n = ntaps;
    for (int i = 0; i < ntaps; ++i) {
        if (tap_r[i] < 0 || tap_r[i] >= R || tap_s[i] < 0 || tap_s[i] >= S) return fail(VATL_EINVAL, "pack_dgrad_weight: tap %d out of range", i);
        t.r[i] = tap_r[i]; t.s[i] = tap_s[i];
    }
    hipLaunchKernelGGL(pack_dgrad_weight_kernel, dim3((unsigned)((long long)cdiv(CinPad, 32) * ntaps * cdiv(CoutK, 32))), dim3(256), 0, (hipStream_t)stream,
                       w_oihw, out, Cout, Cin, R, S, CinPad, CoutK, t);
    return check_launch("pack_dgrad_weight");
}

extern "C" int vatl_pack_weights_multi(const VatlPackJob* jobs_device, int njobs, int64_t total_blocks, void* stream) {
    if (njobs == 0) return 0;
    if (!jobs_device || njobs < 0 || total_blocks <= 0 || total_blocks > 0x7FFFFFFF) return fail(VATL_EINVAL, "pack_weights_multi: bad arguments");
    hipLaunchKernelGGL(pack_multi_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, jobs_device, njobs);
    return check_launch("pack_weights_multi");
}

extern "C" int vatl_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, const float* conv_bias,
                            float eps, float* scale, float* bias, int C, void* stream) {
    if (!scale || !bias || (var && !mean)) return fail(VATL_EINVAL, "bn_fold: bad arguments");
    hipLaunchKernelGGL(bn_fold_kernel, dim3(cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, gamma, beta, mean, var, conv_bias, eps, scale, bias, C);
    return check_launch("bn_fold");
}
