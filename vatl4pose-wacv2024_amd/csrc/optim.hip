// Element-wise optimiser steps, pure HBM streams: one update function, one span walker, two kernels.
//   vatl_adamw_step / _multi    torch.optim.AdamW (decoupled weight decay)            ActiveLearning.py:224-228, :673
//   vatl_adam_step / _multi     torch.optim.Adam (L2 decay folded into the gradient)  ActiveLearning.py:222-223, posetrack_train.py:155-156
//   vatl_sgd_step / _multi      torch.optim.SGD (momentum, dampening 0, no Nesterov)  ActiveLearning.py:220-221
//   vatl_rmsprop_step / _multi  torch.optim.RMSprop (momentum 0, not centered)        posetrack_train.py:157-158
// A flat call takes one span; a multi call takes a device table with rows of {p, g, m, v, numel, first_block} (all int64), one launch
// per parameter group instead of one per tensor (161 tensors for SimplePose-R50).  Either way a block updates kOptBlock (common.h,
// = vatl_adamw_multi_block_elems()) consecutive elements of ONE tensor, so in a table an 8.4 M-element deconv weight and a 64-element
// BatchNorm bias both get blocks in proportion to their size.  Every element is read and written by exactly one thread: no atomics,
// and the result does not depend on the launch shape.
#include "common.h"

namespace vatl {

enum { OPT_ADAMW, OPT_ADAM, OPT_SGD_FIRST, OPT_SGD, OPT_RMSPROP };       // SGD_FIRST: buf = g;  SGD: buf = mu * buf + g

template <int KIND> constexpr bool kHasM = KIND != OPT_RMSPROP;           // row[2]: exp_avg / momentum_buffer
template <int KIND> constexpr bool kHasV = KIND != OPT_SGD_FIRST && KIND != OPT_SGD;   // row[3]: exp_avg_sq / square_avg

struct OptScalars {                                // AdamW: -, 1-b1, b2, 1-b2, sqrt(1-b2^t), eps, lr/(1-b1^t), 1-lr*wd;  Adam: wd, then the same, -
    float wd, omb1, b2, omb2, bc2s, eps, step_size, decay;                // SGD: wd, -, mu, -, -, -, lr, -;  RMSprop: wd, -, alpha, 1-alpha, -, eps, lr, -
};

// Every product-sum below is written out — fused where `fma` stands, rounded twice elsewhere — under `fp contract(off)`, so an
// element's bits depend on nothing but its values and BODY: not on the path (float4 or scalar), the unroll factor, the launch shape
// or the compiler's taste.  The forms are those of the code objects the per-kind kernels once compiled to, whose float4 body — the
// elements below 4 * (n / 4) — and scalar tail of n mod 4 elements were contracted differently; BODY says which of the two an element
// gets.  tests/golden/optim_bits.npz pins the bits (tests/test_gpu_optim.py).  Do not tidy the arithmetic.
template <int KIND, bool BODY>
__device__ __forceinline__ void opt_update(float& P, float G, float& M, float& V, const OptScalars& s) {
#pragma clang fp contract(off)
    if (KIND == OPT_ADAMW || KIND == OPT_ADAM) {
        // Adam: g' = fma(wd, p, g) in body and tail.  Both: body m = fma(1-b1, g-m, m), v = fma(b2, v, (g*g)*(1-b2)); tail mul, then add.
        if (KIND == OPT_ADAM) G = __builtin_fmaf(s.wd, P, G);
        const float gg = (G * G) * s.omb2;
        if (BODY) {
            M = __builtin_fmaf(s.omb1, G - M, M);
            V = __builtin_fmaf(s.b2, V, gg);
        } else {
            const float dm = s.omb1 * (G - M), bv = s.b2 * V;
            M = M + dm;
            V = bv + gg;
        }
        const float q = M / (sqrtf(V) / s.bc2s + s.eps);
        // AdamW: body p = fma(1-lr*wd, p, -(step*q)), tail (1-lr*wd)*p - step*q.  Adam: p = fma(-step, q, p) in body and tail.
        if (KIND == OPT_ADAM) P = __builtin_fmaf(-s.step_size, q, P);
        else {
            const float t = s.step_size * q;
            if (BODY) P = __builtin_fmaf(s.decay, P, -t);
            else { const float dp = s.decay * P; P = dp - t; }
        }
    } else if (KIND == OPT_SGD_FIRST) {
        // SGD, first step: all fused, body and tail alike.
        G = __builtin_fmaf(s.wd, P, G);
        M = G;
        P = __builtin_fmaf(-s.step_size, M, P);
    } else if (KIND == OPT_SGD) {
        // SGD, later steps: body g' = fma(wd, p, g), buf = fma(mu, buf, g'); tail mul, then add for both.  p = fma(-lr, buf, p) in both.
        if (BODY) {
            G = __builtin_fmaf(s.wd, P, G);
            M = __builtin_fmaf(s.b2, M, G);
        } else {
            const float wp = s.wd * P, mb = s.b2 * M;
            G = wp + G;
            M = mb + G;
        }
        P = __builtin_fmaf(-s.step_size, M, P);
    } else {
        // RMSprop: g' = fma(wd, p, g); sq = fma(alpha, sq, ((1-alpha)*g')*g'); p = p - (lr*g') / (sqrt(sq) + eps); body and tail alike.
        G = __builtin_fmaf(s.wd, P, G);
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
            f32x4 M = {0.f, 0.f, 0.f, 0.f}, V = {0.f, 0.f, 0.f, 0.f};
            if (kHasM<KIND>) M = *reinterpret_cast<f32x4*>(m + 4 * q);
            if (kHasV<KIND>) V = *reinterpret_cast<f32x4*>(v + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = P[e], me = M[e], ve = V[e];
                opt_update<KIND, true>(pe, G[e], me, ve, s);
                P[e] = pe; M[e] = me; V[e] = ve;
            }
            *reinterpret_cast<f32x4*>(p + 4 * q) = P;
            if (kHasM<KIND>) *reinterpret_cast<f32x4*>(m + 4 * q) = M;
            if (kHasV<KIND>) *reinterpret_cast<f32x4*>(v + 4 * q) = V;
        }
        done = q1 << 2;
    }
    for (long long i = done + threadIdx.x; i < e1; i += 256) {
        float P = p[i], M = kHasM<KIND> ? m[i] : 0.f, V = kHasV<KIND> ? v[i] : 0.f;
        if (i < body_end) opt_update<KIND, true>(P, g[i], M, V, s);
        else opt_update<KIND, false>(P, g[i], M, V, s);
        p[i] = P;
        if (kHasM<KIND>) m[i] = M;
        if (kHasV<KIND>) v[i] = V;
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
    const long long bases = row[0] | row[1] | (kHasM<KIND> ? row[2] : 0) | (kHasV<KIND> ? row[3] : 0);
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

// One span per block, like the multi launch, up to 2^29 elements; the loop covers anything larger.  Measured on 34 M elements
// (profiles/optim_unify_notes.md): a cap of 8 blocks per CU, where most blocks walk two spans and a few a third, was 1.5 % slower.
constexpr long long kOptFlatMaxBlocks = 65536;

template <int KIND>
static int launch_flat(const char* what, float* p, const float* g, float* m, float* v, int64_t n, const OptScalars& s, void* stream) {
    long long blocks = (n + kOptBlock - 1) / kOptBlock;
    if (blocks > kOptFlatMaxBlocks) blocks = kOptFlatMaxBlocks;
    const uintptr_t bases = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v;            // an unused buffer is null
    hipLaunchKernelGGL(opt_flat_kernel<KIND>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long long)n,
                       (bases & 15) == 0, s);
    return check_launch(what);
}

template <int KIND>
static int launch_multi(const char* what, const int64_t* table_dev, int n_tensors, int64_t total_blocks, int step, const OptScalars& s,
                        void* stream) {
    if (n_tensors <= 0) return 0;
    if (!table_dev) return fail(VATL_EINVAL, "%s: null table", what);
    if (step < 1) return fail(VATL_EINVAL, "%s: step is 1-based", what);
    if (total_blocks <= 0 || total_blocks > 0x7FFFFFFF) return fail(VATL_EINVAL, "%s: total_blocks %lld out of range", what, (long long)total_blocks);
    hipLaunchKernelGGL(opt_multi_kernel<KIND>, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(table_dev), n_tensors, s);
    return check_launch(what);
}

// Host-side scalars: computed in double, then cast.  A step < 1 (rejected by every caller before a launch) gives scalars nobody uses.
static OptScalars adam_scalars(double lr, double beta1, double beta2, double eps, double weight_decay, int step, bool decoupled) {
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
    return OptScalars{decoupled ? 0.f : (float)weight_decay, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)sqrt(bc2),
                      (float)eps, (float)(lr / bc1), decoupled ? (float)(1.0 - lr * weight_decay) : 1.f};
}

static OptScalars sgd_scalars(double lr, double momentum, double weight_decay) {
    return OptScalars{(float)weight_decay, 0.f, (float)momentum, 0.f, 1.f, 0.f, (float)lr, 1.f};
}

static OptScalars rmsprop_scalars(double lr, double alpha, double eps, double weight_decay) {
    return OptScalars{(float)weight_decay, 0.f, (float)alpha, (float)(1.0 - alpha), 1.f, (float)eps, (float)lr, 1.f};
}

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                               double eps, double weight_decay, int step, void* stream) {
    if (!p || !g || !m || !v) return fail(VATL_EINVAL, "adamw_step: null pointer");
    if (step < 1) return fail(VATL_EINVAL, "adamw_step: step is 1-based");
    if (n <= 0) return 0;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return fail(VATL_EINVAL, "adamw_step: spans must be 16-byte aligned");
    return launch_flat<OPT_ADAMW>("adamw_step", p, g, m, v, n, adam_scalars(lr, beta1, beta2, eps, weight_decay, step, true), stream);
}

extern "C" int vatl_adamw_step_multi(const int64_t* table_dev, int n_tensors, int64_t total_blocks, double lr, double beta1, double beta2, double eps,
                                     double weight_decay, int step, void* stream) {
    return launch_multi<OPT_ADAMW>("adamw_step_multi", table_dev, n_tensors, total_blocks, step,
                                   adam_scalars(lr, beta1, beta2, eps, weight_decay, step, true), stream);
}

extern "C" int64_t vatl_adamw_multi_block_elems(void) { return kOptBlock; }

extern "C" int vatl_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                              double eps, double weight_decay, int step, void* stream) {
    if (!p || !g || !m || !v) return fail(VATL_EINVAL, "adam_step: null pointer");
    if (step < 1) return fail(VATL_EINVAL, "adam_step: step is 1-based");
    if (n <= 0) return 0;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return fail(VATL_EINVAL, "adam_step: spans must be 16-byte aligned");
    return launch_flat<OPT_ADAM>("adam_step", p, g, m, v, n, adam_scalars(lr, beta1, beta2, eps, weight_decay, step, false), stream);
}

extern "C" int vatl_adam_step_multi(const int64_t* table_dev, int n_tensors, int64_t total_blocks, double lr, double beta1, double beta2, double eps,
                                    double weight_decay, int step, void* stream) {
    return launch_multi<OPT_ADAM>("adam_step_multi", table_dev, n_tensors, total_blocks, step,
                                  adam_scalars(lr, beta1, beta2, eps, weight_decay, step, false), stream);
}

extern "C" int vatl_sgd_step(float* p, const float* g, float* buf, int64_t n, double lr, double momentum, double weight_decay, int step,
                             void* stream) {
    if (!p || !g || !buf) return fail(VATL_EINVAL, "sgd_step: null pointer");
    if (step < 1) return fail(VATL_EINVAL, "sgd_step: step is 1-based");
    if (n <= 0) return 0;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) return fail(VATL_EINVAL, "sgd_step: spans must be 16-byte aligned");
    const OptScalars s = sgd_scalars(lr, momentum, weight_decay);
    if (step == 1) return launch_flat<OPT_SGD_FIRST>("sgd_step", p, g, buf, nullptr, n, s, stream);
    return launch_flat<OPT_SGD>("sgd_step", p, g, buf, nullptr, n, s, stream);
}

// Rows of {p, g, buf, 0, numel, first_block}; every tensor of a call is at the same step, so one call is one form.
extern "C" int vatl_sgd_step_multi(const int64_t* table_dev, int n_tensors, int64_t total_blocks, double lr, double momentum, double weight_decay,
                                   int step, void* stream) {
    const OptScalars s = sgd_scalars(lr, momentum, weight_decay);
    if (step == 1) return launch_multi<OPT_SGD_FIRST>("sgd_step_multi", table_dev, n_tensors, total_blocks, step, s, stream);
    return launch_multi<OPT_SGD>("sgd_step_multi", table_dev, n_tensors, total_blocks, step, s, stream);
}

extern "C" int vatl_rmsprop_step(float* p, const float* g, float* sq, int64_t n, double lr, double alpha, double eps, double weight_decay,
                                 void* stream) {
    if (!p || !g || !sq) return fail(VATL_EINVAL, "rmsprop_step: null pointer");
    if (n <= 0) return 0;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)sq) & 3) return fail(VATL_EINVAL, "rmsprop_step: spans must be 4-byte aligned");
    return launch_flat<OPT_RMSPROP>("rmsprop_step", p, g, nullptr, sq, n, rmsprop_scalars(lr, alpha, eps, weight_decay), stream);
}

extern "C" int vatl_rmsprop_step_multi(const int64_t* table_dev, int n_tensors, int64_t total_blocks, double lr, double alpha, double eps,
                                       double weight_decay, void* stream) {
    return launch_multi<OPT_RMSPROP>("rmsprop_step_multi", table_dev, n_tensors, total_blocks, 1, rmsprop_scalars(lr, alpha, eps, weight_decay), stream);
}
