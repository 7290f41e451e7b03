// Optimiser steps of the pose-network pre-training loop (alphapose/pretrain.py), pure HBM streams:
//   vatl_adam_step_multi      torch.optim.Adam over a whole parameter group in one launch   posetrack_train.py:155-156
//   vatl_rmsprop_step         torch.optim.RMSprop (defaults: momentum 0, not centered) on one flat span   :157-158
//   vatl_rmsprop_step_multi   the same over a parameter group in one launch
// The table is vatl_adamw_step_multi's: rows of {p, g, m, v, numel, first_block}, all int64 on the device.  A block updates
// kOptBlock (common.h, = vatl_adamw_multi_block_elems()) consecutive elements of ONE tensor, so tensors get blocks in proportion
// to their size; every element is read and written by exactly one thread: no atomics, and the result does not depend on the
// launch shape.
#include "common.h"

namespace vatl {

enum { OPT_ADAM = 0, OPT_RMSPROP = 1 };

struct OptScalars {                                // Adam: wd, 1-b1, b2, 1-b2, sqrt(1-b2^t), eps, lr/(1-b1^t);  RMSprop: wd, -, alpha, 1-alpha, -, eps, lr
    float wd, omb1, b2, omb2, bc2s, eps, step_size;
};

// Every product-sum below is written out — fused where `fma` stands, rounded twice elsewhere — under `fp contract(off)`, so an
// element's bits depend on nothing but its values: not on the path (float4 or scalar), the unroll factor or the launch shape.
//
// Adam must reproduce vatl_adam_step (opt_kernel<0> in train.hip), whose code object contracts `a * b + c` as the compiler saw fit:
// its float4 body — the elements below 4 * (n / 4) — computes m and v with one rounding (fma), its scalar tail of n mod 4 elements
// with two (mul, then add).  BODY says which of the two an element gets; tests/test_gpu_pose_pretrain.py pins the equality.
//   g' = fma(wd, p, g);  m = fma(1-b1, g' - m, m) | m + (1-b1)*(g' - m);  v = fma(b2, v, (g'*g')*(1-b2)) | b2*v + (g'*g')*(1-b2);
//   p = fma(-lr/(1-b1^t), m / (sqrt(v)/sqrt(1-b2^t) + eps), p)
// RMSprop (torch.optim.RMSprop, momentum 0, not centered): g' = fma(wd, p, g);  sq = fma(alpha, sq, ((1-alpha)*g')*g');
//   p = p - (lr*g') / (sqrt(sq) + eps)
template <int KIND, bool BODY>
__device__ __forceinline__ void opt_update(float& P, float G, float& M, float& V, const OptScalars& s) {
#pragma clang fp contract(off)
    G = __builtin_fmaf(s.wd, P, G);
    if (KIND == OPT_ADAM) {
        const float gg = (G * G) * s.omb2;
        if (BODY) {
            M = __builtin_fmaf(s.omb1, G - M, M);
            V = __builtin_fmaf(s.b2, V, gg);
        } else {
            const float dm = s.omb1 * (G - M), bv = s.b2 * V;
            M = M + dm;
            V = bv + gg;
        }
        const float denom = sqrtf(V) / s.bc2s + s.eps;
        P = __builtin_fmaf(-s.step_size, M / denom, P);
    } else {
        V = __builtin_fmaf(s.b2, V, (s.omb2 * G) * G);
        const float denom = sqrtf(V) + s.eps;
        P = P - (s.step_size * G) / denom;
    }
}

// Elements [e0, e1) of one tensor of n elements, e0 a multiple of 4.  16-byte-aligned bases take float4 accesses and a scalar tail of
// < 4 elements; any other base (a view that starts in the middle of a buffer) takes the scalar path throughout.
template <int KIND>
__device__ __forceinline__ void opt_span(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                         long long e0, long long e1, long long n, bool vec, const OptScalars& s) {
    const long long body_end = n & ~3LL;
    long long done = e0;
    if (vec) {
        const long long q1 = e1 >> 2;
        for (long long q = (e0 >> 2) + threadIdx.x; q < q1; q += 256) {
            f32x4 P = *reinterpret_cast<f32x4*>(p + 4 * q);
            const f32x4 G = *reinterpret_cast<const f32x4*>(g + 4 * q);
            f32x4 M = {0.f, 0.f, 0.f, 0.f};
            if (KIND == OPT_ADAM) M = *reinterpret_cast<f32x4*>(m + 4 * q);
            f32x4 V = *reinterpret_cast<f32x4*>(v + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = P[e], me = M[e], ve = V[e];
                opt_update<KIND, true>(pe, G[e], me, ve, s);
                P[e] = pe; M[e] = me; V[e] = ve;
            }
            *reinterpret_cast<f32x4*>(p + 4 * q) = P;
            if (KIND == OPT_ADAM) *reinterpret_cast<f32x4*>(m + 4 * q) = M;
            *reinterpret_cast<f32x4*>(v + 4 * q) = V;
        }
        done = q1 << 2;
    }
    for (long long i = done + threadIdx.x; i < e1; i += 256) {
        float P = p[i], M = (KIND == OPT_ADAM) ? m[i] : 0.f, V = v[i];
        if (i < body_end) opt_update<KIND, true>(P, g[i], M, V, s);
        else opt_update<KIND, false>(P, g[i], M, V, s);
        p[i] = P; v[i] = V;
        if (KIND == OPT_ADAM) m[i] = M;
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void opt_multi_kernel(const long long* __restrict__ table, int n_tensors, OptScalars s) {
    __shared__ int st;
    if (threadIdx.x == 0) {                         // the last row whose first_block <= this block
        int lo = 0, hi = n_tensors - 1;
        const long long b = blockIdx.x;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (table[6 * (long long)mid + 5] <= b) lo = mid; else hi = mid - 1;
        }
        st = lo;
    }
    __syncthreads();
    const long long* row = table + 6 * (long long)st;
    const long long n = row[4];
    const long long e0 = ((long long)blockIdx.x - row[5]) * kOptBlock;
    if (e0 >= n) return;                            // a table whose block counts exceed ceil(numel / kOptBlock): nothing to do
    const long long e1 = e0 + kOptBlock < n ? e0 + kOptBlock : n;
    const long long bases = row[0] | row[1] | row[3] | (KIND == OPT_ADAM ? row[2] : 0);
    opt_span<KIND>(reinterpret_cast<float*>(row[0]), reinterpret_cast<const float*>(row[1]), reinterpret_cast<float*>(row[2]),
                   reinterpret_cast<float*>(row[3]), e0, e1, n, (bases & 15) == 0, s);
}

// One flat span: the same per-block work, the row in the kernel arguments; blocks walk the span grid-stride.
template <int KIND>
__global__ __launch_bounds__(256) void opt_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, long long n, bool vec, OptScalars s) {
    for (long long e0 = (long long)blockIdx.x * kOptBlock; e0 < n; e0 += (long long)gridDim.x * kOptBlock) {
        const long long e1 = e0 + kOptBlock < n ? e0 + kOptBlock : n;
        opt_span<KIND>(p, g, m, v, e0, e1, n, vec, s);
    }
}

static int multi_args(const char* what, const int64_t* table_dev, int64_t total_blocks, int step) {
    if (!table_dev) return fail(VATL_EINVAL, "%s: null table", what);
    if (step < 1) return fail(VATL_EINVAL, "%s: step is 1-based", what);
    if (total_blocks <= 0 || total_blocks > 0x7FFFFFFF) return fail(VATL_EINVAL, "%s: total_blocks %lld out of range", what, (long long)total_blocks);
    return 0;
}

static OptScalars rmsprop_scalars(double lr, double alpha, double eps, double weight_decay) {
    return OptScalars{(float)weight_decay, 0.f, (float)alpha, (float)(1.0 - alpha), 1.f, (float)eps, (float)lr};
}

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_adam_step_multi(const int64_t* table_dev, int n_tensors, int64_t total_blocks, double lr, double beta1, double beta2, double eps,
                                    double weight_decay, int step, void* stream) {
    if (n_tensors <= 0) return 0;
    if (int rc = multi_args("adam_step_multi", table_dev, total_blocks, step)) return rc;
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);       // the scalars of vatl_adam_step
    const OptScalars s{(float)weight_decay, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)sqrt(bc2), (float)eps, (float)(lr / bc1)};
    hipLaunchKernelGGL(opt_multi_kernel<OPT_ADAM>, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(table_dev), n_tensors, s);
    return check_launch("adam_step_multi");
}

extern "C" int vatl_rmsprop_step(float* p, const float* g, float* sq, int64_t n, double lr, double alpha, double eps, double weight_decay,
                                 void* stream) {
    if (!p || !g || !sq) return fail(VATL_EINVAL, "rmsprop_step: null pointer");
    if (n <= 0) return 0;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)sq) & 3) return fail(VATL_EINVAL, "rmsprop_step: spans must be 4-byte aligned");
    long long blocks = (n + kOptBlock - 1) / kOptBlock;
    if (blocks > 256 * 8) blocks = 256 * 8;
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)sq) & 15) == 0;
    hipLaunchKernelGGL(opt_flat_kernel<OPT_RMSPROP>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, (float*)nullptr, sq,
                       (long long)n, vec, rmsprop_scalars(lr, alpha, eps, weight_decay));
    return check_launch("rmsprop_step");
}

extern "C" int vatl_rmsprop_step_multi(const int64_t* table_dev, int n_tensors, int64_t total_blocks, double lr, double alpha, double eps,
                                       double weight_decay, void* stream) {
    if (n_tensors <= 0) return 0;
    if (int rc = multi_args("rmsprop_step_multi", table_dev, total_blocks, 1)) return rc;
    hipLaunchKernelGGL(opt_multi_kernel<OPT_RMSPROP>, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(table_dev), n_tensors, rmsprop_scalars(lr, alpha, eps, weight_decay));
    return check_launch("rmsprop_step_multi");
}
