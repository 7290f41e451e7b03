// Deformable 3x3 convolution (DCN v1 / v2; pad 1, dilation 1, groups 1, stride 1 or 2) on NHWC tensors.  Three kernels, all on the
// sampling rules of deform_sample.h:
//   deform_conv_fwd_kernel     the fused forward: gather + bilinear blend straight into the A operand of v_mfma_f32_32x32x2f32, folded
//                              scale / bias (+ReLU) epilogue (inference);
//   deform_columns_kernel      the sampled, mask-weighted matrix [pixels][9*C] that the 1x1 GEMMs then multiply (training forward, and
//                              the second implementation the fused one is checked against);
//   deform_columns_bwd_kernel  its backward: dx by float atomics (vector memory instructions), d_offset / d_mask by a fixed-order
//                              reduction over the deformable group's channels.  The ordered, bit-reproducible dx is
//                              deform_dx_ordered.hip's; it runs this kernel without the atomics for d_offset / d_mask.
// Offsets and masks are read per pixel with a caller-given stride, so that they can stay inside conv2_offset's NHWC output
// ([18*dg offsets | 9*dg mask logits] per pixel); a mask that arrives as logits gets its sigmoid here.
#include "deform_tap.h"

namespace vatl {

// ---- fused forward ------------------------------------------------------------------------------------------------------------
// A block owns 32 output pixels x up to 128 output channels (4 waves x one 32x32 accumulator).  Phase 1: for every (pixel, tap,
// deformable group) of the tile the four corner pixel indices and the four blend weights (mask multiplied in) go to LDS, once.
// Phase 2: lane (pixel = lane % 32, k-half = lane / 32) walks the taps and 8-channel chunks; it fetches its 4 channels of the four
// corners as 16-byte loads (channels are contiguous in NHWC), blends them and feeds them as the A operand of four MFMAs whose B
// operand is the [tap][c][co] filter row of its output channel (k = 0 <-> channel c0 + j, k = 1 <-> channel c0 + 4 + j).
constexpr int kDcPix = 32;

__global__ __launch_bounds__(256) void deform_conv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wt, DeformGeom q,
                                                              const float* __restrict__ scale, const float* __restrict__ bias,
                                                              float* __restrict__ y, int Co, int relu) {
    extern __shared__ __align__(16) unsigned char dc_lds[];
    const int entries = kDcPix * 9 * q.dg;
    int* s_idx = reinterpret_cast<int*>(dc_lds);                       // [tap * dg + g][pixel][4]
    float* s_w = reinterpret_cast<float*>(dc_lds) + entries * 4;
    const long long p0 = (long long)blockIdx.x * kDcPix;
    for (int e = threadIdx.x; e < entries; e += blockDim.x) {
        const int pi = e % kDcPix, tg = e / kDcPix, t = tg / q.dg, g = tg % q.dg;
        int id[4] = {0, 0, 0, 0};
        float ww[4] = {0.f, 0.f, 0.f, 0.f};
        if (p0 + pi < q.P) {
            const DeformTap d = deform_tap(q, p0 + pi, t, g);
#pragma unroll
            for (int k = 0; k < 4; ++k) { id[k] = (int)(d.base + d.s.idx[k]); ww[k] = d.s.w[k] * d.m; }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { s_idx[e * 4 + k] = id[k]; s_w[e * 4 + k] = ww[k]; }
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, pi = lane & 31, kh = lane >> 5;
    const int co = (blockIdx.y * 4 + wave) * 32 + pi;
    if ((blockIdx.y * 4 + wave) * 32 >= Co) return;                    // (no barrier after this point)
    const bool co_ok = co < Co;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int t = 0; t < 9; ++t) {
        int g_have = -1;
        int id[4];
        float ww[4];
        for (int c0 = 0; c0 < q.C; c0 += 8) {
            const int cc = c0 + 4 * kh;
            const int g = cc / q.Cg;
            if (g != g_have) {
                const int e = ((t * q.dg + g) * kDcPix + pi) * 4;
#pragma unroll
                for (int k = 0; k < 4; ++k) { id[k] = s_idx[e + k]; ww[k] = s_w[e + k]; }
                g_have = g;
            }
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(x + (long long)id[k] * q.C + cc);
                a[0] = fmaf(ww[k], v[0], a[0]); a[1] = fmaf(ww[k], v[1], a[1]); a[2] = fmaf(ww[k], v[2], a[2]); a[3] = fmaf(ww[k], v[3], a[3]);
            }
            const float* wr = wt + ((long long)t * q.C + cc) * Co + co;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float b = co_ok ? wr[(long long)j * Co] : 0.f;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b, acc, 0, 0, 0);
            }
        }
    }
    // D layout of the 32x32 MFMA: acc[i] is row (pixel) 8 * (i / 4) + 4 * (lane / 32) + i % 4, column (channel) lane % 32
    if (!co_ok) return;
    const float sc = scale ? scale[co] : 1.f, bi = bias ? bias[co] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const long long p = p0 + 8 * (i >> 2) + 4 * kh + (i & 3);
        if (p < q.P) {
            float v = fmaf(acc[i], sc, bi);
            if (relu) v = fmaxf(v, 0.f);
            y[p * Co + co] = v;
        }
    }
}

// ---- columns ------------------------------------------------------------------------------------------------------------------
// col[p][t * C + c] = m(p, t, g(c)) * S(x[n, :, :, c], py, px); columns 9 * C .. col_stride - 1 (padding up to the GEMM's K step) = 0.
__global__ void deform_columns_kernel(const float* __restrict__ x, DeformGeom q, float* __restrict__ col, int col_stride) {
    const int C4 = q.C >> 2, K4 = col_stride >> 2;
    const long long total = q.P * K4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long p = i / K4;
        const int k4 = (int)(i - p * K4);
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        if (k4 < 9 * C4) {
            const int t = k4 / C4, cc = (k4 - t * C4) * 4;
            const DeformTap d = deform_tap(q, p, t, cc / q.Cg);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float wk = d.s.w[k] * d.m;
                const f32x4 v = *reinterpret_cast<const f32x4*>(x + (d.base + d.s.idx[k]) * q.C + cc);
                a[0] = fmaf(wk, v[0], a[0]); a[1] = fmaf(wk, v[1], a[1]); a[2] = fmaf(wk, v[2], a[2]); a[3] = fmaf(wk, v[3], a[3]);
            }
        }
        *reinterpret_cast<f32x4*>(col + p * col_stride + k4 * 4) = a;
    }
}

// ---- backward of the columns --------------------------------------------------------------------------------------------------
// 16 lanes own one (pixel, tap, deformable group): lane l takes the group's 4-channel runs l, l + 16, ...  Per channel with
// v = dcol: dx[corner k] += v * m * w[k] (float atomics: the order in which pixels meet at a corner is not fixed, so dx is not
// bit-reproducible — kAddDx = false leaves dx alone: the ordered entry sums it through an index); d_mask += v * S, d_py += v * m * sum_k gy[k] x_k, d_px likewise, summed per lane in channel order and then
// across the 16 lanes by a butterfly — a fixed order.  Where the position fails the validity rule all three are 0.
template <bool kAddDx>
__global__ void deform_columns_bwd_kernel(const float* __restrict__ dcol, int col_stride, const float* __restrict__ x, DeformGeom q,
                                          float* __restrict__ dx, float* __restrict__ d_offset, int d_off_stride,
                                          float* __restrict__ d_mask, int d_mask_stride) {
    const long long entries = q.P * 9 * q.dg;
    const long long e = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 4;       // uniform over each group of 16 lanes
    if (e >= entries) return;
    const int l = threadIdx.x & 15;
    const int g = (int)(e % q.dg);
    const int t = (int)((e / q.dg) % 9);
    const long long p = e / (9 * q.dg);
    const DeformTap d = deform_tap(q, p, t, g);
    float sm = 0.f, sy = 0.f, sx = 0.f;
    if (d.s.valid) {
        for (int cc = g * q.Cg + 4 * l; cc < (g + 1) * q.Cg; cc += 64) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(dcol + p * col_stride + t * q.C + cc);
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, ty = {0.f, 0.f, 0.f, 0.f}, tx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (d.s.w[k] == 0.f && d.s.gy[k] == 0.f && d.s.gx[k] == 0.f) continue;     // a corner that does not count
                const long long at = (d.base + d.s.idx[k]) * q.C + cc;
                const f32x4 xv = *reinterpret_cast<const f32x4*>(x + at);
                const float wk = d.s.w[k] * d.m;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    s[c] = fmaf(d.s.w[k], xv[c], s[c]);
                    ty[c] = fmaf(d.s.gy[k], xv[c], ty[c]);
                    tx[c] = fmaf(d.s.gx[k], xv[c], tx[c]);
                    if (kAddDx && wk != 0.f) unsafeAtomicAdd(dx + at + c, v[c] * wk);
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) { sm = fmaf(v[c], s[c], sm); sy = fmaf(v[c], ty[c], sy); sx = fmaf(v[c], tx[c], sx); }
        }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) { sm += __shfl_xor(sm, o, 16); sy += __shfl_xor(sy, o, 16); sx += __shfl_xor(sx, o, 16); }
    if (l == 0) {
        d_offset[p * d_off_stride + 18 * g + 2 * t] = sy * d.m;
        d_offset[p * d_off_stride + 18 * g + 2 * t + 1] = sx * d.m;
        if (d_mask) d_mask[p * d_mask_stride + 9 * g + t] = q.mask_logits ? sm * d.m * (1.f - d.m) : sm;
    }
}

int deform_bwd_check(const char* who, DeformGeom& q, const float* dcol, int col_stride, const float* x, const float* offset, int offset_stride,
                     const float* mask_or_null, int mask_stride, int mask_is_logits, const float* dx, const float* d_offset, int d_offset_stride,
                     const float* d_mask_or_null, int d_mask_stride, int N, int H, int W, int C, int stride, int deform_groups) {
    if (!dcol || !x || !dx || !d_offset) return fail(VATL_EINVAL, "%s: null pointer", who);
    if ((mask_or_null == nullptr) != (d_mask_or_null == nullptr)) return fail(VATL_EINVAL, "%s: mask and d_mask go together", who);
    if (int rc = deform_geom(who, q, offset, offset_stride, mask_or_null, mask_stride, mask_is_logits, N, H, W, C, stride, deform_groups)) return rc;
    if (col_stride < 9 * C || (col_stride & 3) || q.P * col_stride >= (1LL << 30)) return fail(VATL_EINVAL, "%s: column stride %d invalid", who, col_stride);
    if (d_offset_stride < 18 * deform_groups || (d_mask_or_null && d_mask_stride < 9 * deform_groups) || q.P * (long long)d_offset_stride >= (1LL << 30) ||
        q.P * (long long)d_mask_stride >= (1LL << 30))
        return fail(VATL_EINVAL, "%s: gradient stride invalid", who);
    return 0;
}

void deform_bwd_launch(bool add_dx, const float* dcol, int col_stride, const float* x, const DeformGeom& q, float* dx, float* d_offset,
                       int d_offset_stride, float* d_mask_or_null, int d_mask_stride, hipStream_t st) {
    const long long threads = q.P * 9 * q.dg * 16;
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (add_dx)
        hipLaunchKernelGGL(deform_columns_bwd_kernel<true>, grid, dim3(256), 0, st, dcol, col_stride, x, q, dx, d_offset, d_offset_stride, d_mask_or_null,
                           d_mask_stride);
    else
        hipLaunchKernelGGL(deform_columns_bwd_kernel<false>, grid, dim3(256), 0, st, dcol, col_stride, x, q, dx, d_offset, d_offset_stride, d_mask_or_null,
                           d_mask_stride);
}

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_deform_conv2d_supported(int C, int Cout, int stride, int deform_groups) {
    return C > 0 && C % 16 == 0 && Cout > 0 && Cout % 16 == 0 && (stride == 1 || stride == 2) &&
           (deform_groups == 1 || deform_groups == 2 || deform_groups == 4);
}

extern "C" int vatl_deform_conv2d_fwd(const float* x, const float* w_tcc, const float* offset, int offset_stride, const float* mask_or_null,
                                      int mask_stride, int mask_is_logits, const float* scale, const float* bias, float* y, int N, int H, int W,
                                      int C, int Cout, int stride, int deform_groups, int relu, void* stream) {
    if (!x || !w_tcc || !y) return fail(VATL_EINVAL, "deform_conv2d_fwd: null pointer");
    if (!vatl_deform_conv2d_supported(C, Cout, stride, deform_groups))
        return fail(VATL_EINVAL, "deform_conv2d_fwd: C %d / Cout %d (multiples of 16), stride %d (1, 2), %d deformable groups (1, 2, 4) not served", C, Cout,
                    stride, deform_groups);
    DeformGeom q{};
    if (int rc = deform_geom("deform_conv2d_fwd", q, offset, offset_stride, mask_or_null, mask_stride, mask_is_logits, N, H, W, C, stride, deform_groups)) return rc;
    if (q.P * Cout >= (1LL << 30)) return fail(VATL_EINVAL, "deform_conv2d_fwd: a tensor exceeds 2^30 elements; split the batch");
    const dim3 grid((unsigned)cdiv(q.P, kDcPix), (unsigned)cdiv(Cout, 128));
    const size_t lds = (size_t)kDcPix * 9 * deform_groups * 8 * sizeof(float);        // <= 36 KB
    hipLaunchKernelGGL(deform_conv_fwd_kernel, grid, dim3(256), lds, (hipStream_t)stream, x, w_tcc, q, scale, bias, y, Cout, relu);
    return check_launch("deform_conv2d_fwd");
}

extern "C" int vatl_deform_columns(const float* x, const float* offset, int offset_stride, const float* mask_or_null, int mask_stride,
                                   int mask_is_logits, float* col, int col_stride, int N, int H, int W, int C, int stride, int deform_groups,
                                   void* stream) {
    if (!x || !col) return fail(VATL_EINVAL, "deform_columns: null pointer");
    DeformGeom q{};
    if (int rc = deform_geom("deform_columns", q, offset, offset_stride, mask_or_null, mask_stride, mask_is_logits, N, H, W, C, stride, deform_groups)) return rc;
    if (col_stride < 9 * C || (col_stride & 3) || q.P * col_stride >= (1LL << 30)) return fail(VATL_EINVAL, "deform_columns: column stride %d invalid", col_stride);
    long long blocks = (q.P * (col_stride / 4) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(deform_columns_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, q, col, col_stride);
    return check_launch("deform_columns");
}

extern "C" int vatl_deform_columns_bwd(const float* dcol, int col_stride, const float* x, const float* offset, int offset_stride,
                                       const float* mask_or_null, int mask_stride, int mask_is_logits, float* dx, float* d_offset,
                                       int d_offset_stride, float* d_mask_or_null, int d_mask_stride, int N, int H, int W, int C, int stride,
                                       int deform_groups, void* stream) {
    DeformGeom q{};
    if (int rc = deform_bwd_check("deform_columns_bwd", q, dcol, col_stride, x, offset, offset_stride, mask_or_null, mask_stride, mask_is_logits, dx, d_offset,
                                  d_offset_stride, d_mask_or_null, d_mask_stride, N, H, W, C, stride, deform_groups))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(dx, 0, (size_t)N * H * W * C * sizeof(float), st) != hipSuccess) return fail(VATL_ELAUNCH, "deform_columns_bwd: memset failed");
    deform_bwd_launch(true, dcol, col_stride, x, q, dx, d_offset, d_offset_stride, d_mask_or_null, d_mask_stride, st);
    return check_launch("deform_columns_bwd");
}
