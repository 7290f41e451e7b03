// The training-mode BatchNorm pieces that the conv write-outs (conv_igemm.h: conv_epilogue, conv_winograd.hip: winograd_body, winograd_f4.hip:
// f4_body) share with one another and with the stand-alone reduction (bn_train.hip): each formula below exists once, so that the fused
// epilogues and col_reduce_kernel give the same per-channel sums up to summation order, and the mask of a data gradient is the very expression
// (glue_common.h: relu_on) that scale_bias_act_kernel's activation came from.  All on one channel quad (f32x4) of one pixel.
#pragma once
#include "glue_common.h"

namespace vatl {

// forward statistics of a stored quad: (sum o, sum o^2)
__device__ __forceinline__ void fold_stats(f32x4& s, f32x4& q, f32x4 o) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { s[e] += o[e]; q[e] += o[e] * o[e]; }
}
// one row of the backward reduction: (sum g, sum g * xhat).  The product goes into the sum as ONE fused multiply-add, spelled out: left to the
// compiler's contraction, a write-out that packs the products of two rows into one multiply adds them unfused, and the partials move in their last bits.
__device__ __forceinline__ void fold_g_xhat(f32x4& s, f32x4& q, f32x4 g, f32x4 zz, f32x4 mu, f32x4 is) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { s[e] += g[e]; q[e] = fmaf(g[e], (zz[e] - mu[e]) * is[e], q[e]); }
}

// Per-channel constants of the backward reduction for channels n .. n + 3 (`valid`: the quad is in range): saved mean and inverse deviation,
// and the (scale, bias) the ReLU mask is recomputed from.  No mask given (mscale == NULL): 0 * z + 1 > 0.
struct BnConsts { f32x4 mu, is, msc, mbi; };
__device__ __forceinline__ BnConsts bn_consts(const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ mscale,
                                              const float* __restrict__ mbias, int n, bool valid) {
    const f32x4 one = {1.f, 1.f, 1.f, 1.f}, nul = {0.f, 0.f, 0.f, 0.f};
    BnConsts k = {nul, nul, nul, one};
    if (valid) {
        k.mu = *reinterpret_cast<const f32x4*>(mean + n); k.is = *reinterpret_cast<const f32x4*>(invstd + n);
        if (mscale) { k.msc = *reinterpret_cast<const f32x4*>(mscale + n); k.mbi = *reinterpret_cast<const f32x4*>(mbias + n); }
    }
    return k;
}

// g = d where the consumer layer's ReLU let the activation through — its saved output y > 0 (`saved`), else recomputed from its conv output z —
// and the quad is stored at all (`stored`: a pixel past the edge contributes exact zeros); folds g into (s, q)
__device__ __forceinline__ f32x4 bn_masked_grad(f32x4 d, f32x4 z, f32x4 y, bool saved, const BnConsts& k, f32x4& s, f32x4& q, bool stored = true) {
    f32x4 g;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool on = saved ? y[e] > 0.f : relu_on(z[e], k.msc[e], k.mbi[e]);
        g[e] = (on && stored) ? d[e] : 0.f;
    }
    fold_g_xhat(s, q, g, z, k.mu, k.is);
    return g;
}

// Block combine of the write-out's fp32 partials: NT threads, thread t holding channel quad t % C4 of its rows -> one double (sum, sum^2) pair per
// (row block rb, channel) in the layout bn_train_finalize_kernel / bn_bwd_finalize_kernel reduce, summed through LDS in a fixed order (no atomics).
// `smem`: 2 * NT float4 that every thread is done with once it arrives here; n0: first channel of the block's C4 quads.  The caller's row block comes
// as its factors, rb = rb_hi * rb_mul + rb_lo, formed behind the combine loop: as one value the two-half and gather Winograd kernels compile to other code.
template <int NT, int C4>
__device__ __forceinline__ void stats_block_store(float* smem, int tid, f32x4 s, f32x4 q, double* stats, long long rb_hi, int rb_mul, int rb_lo, int n0, int Cout) {
    lds_barrier();                                     // (LDS hand-off only: __syncthreads() would wait for the tile's stores)
    f32x4* sh = reinterpret_cast<f32x4*>(smem);
    sh[tid] = s; sh[NT + tid] = q;
    lds_barrier();
    if (tid < C4) {
        double ds[4] = {0, 0, 0, 0}, dq[4] = {0, 0, 0, 0};
#pragma unroll 2                                       // (full unrolling cost the 128x32 implicit-GEMM kernel 256 VGPRs and spills)
        for (int k = 0; k < NT / C4; ++k) {
            const f32x4 a = sh[k * C4 + tid], b = sh[NT + k * C4 + tid];
#pragma unroll
            for (int c = 0; c < 4; ++c) { ds[c] += a[c]; dq[c] += b[c]; }
        }
        const long long rb = rb_hi * rb_mul + rb_lo;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int n = n0 + tid * 4 + c;
            if (n < Cout) {
                stats[(rb * Cout + n) * 2 + 0] = ds[c];
                stats[(rb * Cout + n) * 2 + 1] = dq[c];
            }
        }
    }
}

// The fusion arguments of a *_bnbwd entry point `who`: the consumer layer's conv output, its saved statistics, somewhere to put the partials and
// their count, and the mask's scale WITH its bias or neither.
static inline int bnbwd_args_check(const char* who, const float* bn_z, const float* bn_scale, const float* bn_bias, const float* bn_mean,
                                   const float* bn_invstd, const double* stats, const int64_t* row_blocks_used) {
    if (!bn_z || !stats || !row_blocks_used || !bn_mean || !bn_invstd || (!bn_scale != !bn_bias))
        return fail(VATL_EINVAL, "%s: needs z, mean, invstd and a statistics buffer (and scale WITH bias, or neither)", who);
    return 0;
}

}  // namespace vatl
