// What the deformable-convolution kernels share (deform_conv.hip, deform_dx_ordered.hip): the geometry of a call, its checks, and
// `deform_tap`, the one place where a kernel turns (output pixel, tap, deformable group) into a sample of deform_sample.h.
#pragma once
#include "common.h"
#include "deform_sample.h"

namespace vatl {

struct DeformGeom {
    int N, H, W, C, Ho, Wo, stride, dg, Cg;           // Cg = C / dg channels per deformable group
    long long P;                                       // N * Ho * Wo output pixels
    const float* offset; int off_stride;               // offset[p * off_stride + 18 g + 2 t (+1)]
    const float* mask; int mask_stride, mask_logits;   // mask[p * mask_stride + 9 g + t], NULL = 1
};

struct DeformTap { DeformSample s; float m, raw; long long base; };   // base = n * H * W: pixel index of the image's first pixel

// everything the kernels need to know about (output pixel p, tap t, deformable group g)
__device__ __forceinline__ DeformTap deform_tap(const DeformGeom& q, long long p, int t, int g) {
    const int xo = (int)(p % q.Wo);
    const long long r = p / q.Wo;
    const int yo = (int)(r % q.Ho);
    const long long n = r / q.Ho;
    const float* o = q.offset + p * q.off_stride + 18 * g + 2 * t;
    DeformTap d;
    d.s = deform_sample(deform_pos(yo, q.stride, t / 3, o[0]), deform_pos(xo, q.stride, t % 3, o[1]), q.H, q.W);
    d.raw = q.mask ? q.mask[p * q.mask_stride + 9 * g + t] : 1.f;
    d.m = (q.mask && q.mask_logits) ? deform_sigmoid(d.raw) : d.raw;
    d.base = n * q.H * q.W;
    return d;
}

inline int deform_geom(const char* who, DeformGeom& q, const float* offset, int off_stride, const float* mask, int mask_stride, int mask_logits,
                       int N, int H, int W, int C, int stride, int dg) {
    if (!offset || N <= 0 || H <= 0 || W <= 0) return fail(VATL_EINVAL, "%s: null pointer or empty tensor", who);
    if (stride != 1 && stride != 2) return fail(VATL_EINVAL, "%s: stride %d (1 or 2)", who, stride);
    if (dg != 1 && dg != 2 && dg != 4) return fail(VATL_EINVAL, "%s: %d deformable groups (1, 2 or 4)", who, dg);
    if (C <= 0 || C % 16) return fail(VATL_EINVAL, "%s: C %d must be a multiple of 16", who, C);
    if (off_stride < 18 * dg || (mask && mask_stride < 9 * dg)) return fail(VATL_EINVAL, "%s: offset / mask stride too small", who);
    q.N = N; q.H = H; q.W = W; q.C = C; q.stride = stride; q.dg = dg; q.Cg = C / dg;
    q.Ho = (H + 2 - 3) / stride + 1; q.Wo = (W + 2 - 3) / stride + 1;
    q.P = (long long)N * q.Ho * q.Wo;
    q.offset = offset; q.off_stride = off_stride; q.mask = mask; q.mask_stride = mask_stride; q.mask_logits = mask ? mask_logits : 0;
    const long long lim = 1LL << 30;
    if ((long long)N * H * W * C >= lim || q.P * 9 * C >= lim || q.P * (long long)off_stride >= lim || q.P * (long long)mask_stride >= lim)
        return fail(VATL_EINVAL, "%s: a tensor exceeds 2^30 elements; split the batch", who);
    return 0;
}

// The argument checks of the two backward entries (vatl_deform_columns_bwd, vatl_deform_columns_bwd_ordered), deform_geom included, and
// the launch of deform_columns_bwd_kernel (deform_conv.hip): with `add_dx` dx by float atomics into a zeroed dx, without it d_offset
// and d_mask only — the same code, the same bits.
__attribute__((visibility("hidden"))) int deform_bwd_check(const char* who, DeformGeom& q, const float* dcol, int col_stride, const float* x,
                                                           const float* offset, int offset_stride, const float* mask_or_null, int mask_stride,
                                                           int mask_is_logits, const float* dx, const float* d_offset, int d_offset_stride,
                                                           const float* d_mask_or_null, int d_mask_stride, int N, int H, int W, int C, int stride,
                                                           int deform_groups);
__attribute__((visibility("hidden"))) void deform_bwd_launch(bool add_dx, const float* dcol, int col_stride, const float* x, const DeformGeom& q,
                                                             float* dx, float* d_offset, int d_offset_stride, float* d_mask_or_null,
                                                             int d_mask_stride, hipStream_t st);

}  // namespace vatl
