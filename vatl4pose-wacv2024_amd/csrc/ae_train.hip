// WholeBodyAE training at pre-training batch sizes (scripts/wholebodyAE_train.py:110-184: batches of 10 000 / 8 000):
//   vatl_ae_backward           parameter (and input) gradients for given upstream gradients   loss.backward(), script line 151
//   vatl_ae_train_step_large   forward + MSELoss(output, input) + backward + Adam / AdamW      script lines 147-152
// Two launches each, no host synchronisation, no floating-point atomics:
//   1. ae_grad_partial_kernel: block k takes a contiguous range of items, 64 at a time (one item per lane).  It recomputes the forward
//      pass in LDS with ae_forward_kernel's operation order (pose_feature.hip: acc = bias, then fmaf over k ascending), so the ReLU masks are
//      the ones the forward pass produced, forms the deltas layer by layer, and every thread sums ITS parameters over the items in item
//      order.  The block's sums go to partial[k][P], its squared-error sum to the P-th column block.
//   2. ae_grad_finish_kernel: one thread per parameter adds the block partials in block order in double, then writes the gradient
//      or applies the optimiser update in place.
// The block count and the item ranges depend on N alone (ae_blocks), never on the device: the same call gives the same bits everywhere.
// Parameter layout = vatl_pack_ae order (W0,b0,...,W7,b7), W row-major (out, in).
#include "common.h"

namespace vatl {

constexpr int AEL_CHUNK = 64;                         // items per pass = lanes of a wave
constexpr int AEL_MAXW = 64;                          // D, z <= 64 like vatl_ae_forward
constexpr int AEL_MAXBLOCKS = 1024;
// dynamic LDS of the D = z = 64 case: P + 64 * sum(dims | 1) + 2 * 64 * 65 floats
constexpr int AEL_MAXLDS = 4 * (4926 + AEL_CHUNK * (3 * 65 + 2 * 25 + 2 * 13 + 2 * 7) + 2 * AEL_CHUNK * 65);

struct AeBlocks {
    int chunks_per_block, blocks;
};
static AeBlocks ae_blocks(int N) {
    const int chunks = cdiv(N, AEL_CHUNK);
    AeBlocks b;
    b.chunks_per_block = cdiv(chunks, AEL_MAXBLOCKS);
    b.blocks = cdiv(chunks, b.chunks_per_block);
    return b;
}
static int ae_param_count(int D, int z) { return 2 * (D * 24 + 24 * 12 + 12 * 7 + 7 * z) + 2 * (24 + 12 + 7) + D + z; }

// FUSED = 0: delta at the output = dy * y * (1 - y).  FUSED = 1: dy = d MSELoss(y, x) / dy = 2 (y - x) / (N D), and the block's sum of
// (y - x)^2 goes to lossp[block].
template <int FUSED>
__global__ __launch_bounds__(256) void ae_grad_partial_kernel(const float* __restrict__ feat, const float* __restrict__ dy, const float* __restrict__ ae,
                                                              int D, int z, int N, int chunks_per_block, float inv_numel, float* __restrict__ part,
                                                              float* __restrict__ lossp, float* __restrict__ dx) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int dims[9], offw[8], aoff[9], astr[9];
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) {
        const int d[9] = {D, 24, 12, 7, z, 7, 12, 24, D};
        int p = 0, a = 0;
        for (int l = 0; l < 9; ++l) {
            dims[l] = d[l];
            astr[l] = d[l] | 1;                      // odd row stride: the 64 items of a chunk fall on 64 different banks
            aoff[l] = a; a += AEL_CHUNK * astr[l];
            if (l < 8) { offw[l] = p; p += d[l + 1] * d[l] + d[l + 1]; }
        }
    }
    __syncthreads();
    const int P = offw[7] + D * 24 + D;
    const int dstr = (D > z ? (D > 24 ? D : 24) : (z > 24 ? z : 24)) | 1;
    float* W = lds;
    float* act = W + P;
    float* delta = act + aoff[8] + AEL_CHUNK * astr[8];
    for (int i = tid; i < P; i += 256) W[i] = ae[i];
    float* mypart = part + (long long)blockIdx.x * P;
    float ls = 0.f;

    for (int c = 0; c < chunks_per_block; ++c) {
        const long long item0 = ((long long)blockIdx.x * chunks_per_block + c) * AEL_CHUNK;
        if (item0 >= N) break;                       // uniform over the block
        const int cnt = (int)(N - item0 < AEL_CHUNK ? N - item0 : AEL_CHUNK);
        __syncthreads();                             // the previous chunk's readers are done (and W is in place)
        for (int idx = tid; idx < AEL_CHUNK * D; idx += 256) {
            const int b = idx / D, i = idx - b * D;
            act[b * astr[0] + i] = b < cnt ? feat[item0 * D + idx] : 0.f;
            if (!FUSED) delta[b * dstr + i] = b < cnt ? dy[item0 * D + idx] : 0.f;
        }
        __syncthreads();
        // forward: lane = item, the wave walks the neurons wv, wv + 4, ...
        for (int l = 0; l < 8; ++l) {
            const int ni = dims[l], no = dims[l + 1];
            const float* a = act + aoff[l] + lane * astr[l];
            float* y = act + aoff[l + 1] + lane * astr[l + 1];
            const float* w = W + offw[l];
            for (int o = wv; o < no; o += 4) {
                float acc = w[no * ni + o];
                for (int k = 0; k < ni; ++k) acc = fmaf(w[o * ni + k], a[k], acc);
                if (l == 7) acc = 1.f / (1.f + expf(-acc));
                else if (l != 3) acc = fmaxf(acc, 0.f);
                y[o] = acc;
            }
            __syncthreads();
        }
        // output delta through the sigmoid; rows past the end of the batch get 0 and so add nothing below
        {
            const float* x = act + lane * astr[0];
            const float* y = act + aoff[8] + lane * astr[8];
            float* dl = delta + lane * dstr;
            for (int o = wv; o < D; o += 4) {
                const float yo = y[o];
                if (FUSED) {
                    const float d = lane < cnt ? yo - x[o] : 0.f;
                    ls += d * d;
                    dl[o] = 2.f * d * inv_numel * yo * (1.f - yo);
                } else {
                    dl[o] = dl[o] * yo * (1.f - yo);
                }
            }
        }
        __syncthreads();
        // backward
        int cur = 0;
        for (int l = 7; l >= 0; --l) {
            const int ni = dims[l], no = dims[l + 1];
            const float* dcur = delta + cur * AEL_CHUNK * dstr;
            const float* a = act + aoff[l];
            const int as = astr[l];
            for (int idx = tid; idx < no * ni + no; idx += 256) {          // a thread owns its parameters: sums in item order
                const int pi = offw[l] + idx;
                float g = c == 0 ? 0.f : mypart[pi];
                if (idx < no * ni) {
                    const int o = idx / ni, i = idx - o * ni;
                    for (int b = 0; b < cnt; ++b) g = fmaf(dcur[b * dstr + o], a[b * as + i], g);
                } else {
                    const int o = idx - no * ni;
                    for (int b = 0; b < cnt; ++b) g += dcur[b * dstr + o];
                }
                mypart[pi] = g;
            }
            if (l > 0 || dx) {
                float* dn = delta + (cur ^ 1) * AEL_CHUNK * dstr + lane * dstr;
                const float* dl = dcur + lane * dstr;
                const float* w = W + offw[l];
                const float* al = a + lane * as;
                for (int i = wv; i < ni; i += 4) {
                    float d = 0.f;
                    for (int o = 0; o < no; ++o) d = fmaf(w[o * ni + i], dl[o], d);
                    if (l != 4 && l != 0) d = al[i] > 0.f ? d : 0.f;        // act[l] is the ReLU output of layer l-1 (act[4] = code: linear)
                    dn[i] = d;
                }
            }
            __syncthreads();
            cur ^= 1;
        }
        if (dx) {                                    // cur now names the buffer that holds d loss / d input
            const float* d0 = delta + cur * AEL_CHUNK * dstr;
            for (int idx = tid; idx < cnt * D; idx += 256) {
                const int b = idx / D, i = idx - b * D;
                dx[item0 * D + idx] = d0[b * dstr + i];
            }
        }
    }
    if (FUSED) {
        ls = wave_sum(ls);
        if (lane == 0) red[wv] = ls;
        __syncthreads();
        if (tid == 0) lossp[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

// MODE 0: grad[pi] = sum of the block partials.  MODE 1: torch.optim.Adam (l2 = weight_decay, decay = 1) or torch.optim.AdamW
// (l2 = 0, decay = 1 - lr * weight_decay) on ae / am / av with that gradient; per element the formulas of opt_update<OPT_ADAM> /
// <OPT_ADAMW> (optim.hip), in plain C++ here: this kernel's contraction is the compiler's.  Block 0 also reduces the loss.
template <int MODE>
__global__ __launch_bounds__(256) void ae_grad_finish_kernel(const float* __restrict__ part, const float* __restrict__ lossp, int nblk, int P,
                                                             float* __restrict__ grad, float* __restrict__ ae, float* __restrict__ am,
                                                             float* __restrict__ av, float l2, float decay, float omb1, float b2, float omb2,
                                                             float bc2s, float eps, float step_size, double inv_numel, float* __restrict__ loss) {
    const int pi = blockIdx.x * 256 + threadIdx.x;
    if (pi < P) {
        double s = 0.0;
#pragma unroll 8
        for (int k = 0; k < nblk; ++k) s += (double)part[(long long)k * P + pi];
        float g = (float)s;
        if (MODE == 0) grad[pi] = g;
        else {
            float p = ae[pi];
            g = g + l2 * p;
            p = p * decay;
            const float m = am[pi] + (g - am[pi]) * omb1;
            const float v = av[pi] * b2 + g * g * omb2;
            am[pi] = m; av[pi] = v;
            ae[pi] = p - step_size * (m / (sqrtf(v) / bc2s + eps));
        }
    }
    if (MODE == 1 && loss && blockIdx.x == 0) {
        __shared__ double red[4];
        double s = 0.0;
        for (int k = threadIdx.x; k < nblk; k += 256) s += (double)lossp[k];
        s = wave_sum(s);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) *loss = (float)(((red[0] + red[1]) + (red[2] + red[3])) * inv_numel);
    }
}

static int ae_lds_bytes(int D, int z) {
    const int d[9] = {D, 24, 12, 7, z, 7, 12, 24, D};
    int mx = 24, a = 0;
    for (int l = 0; l < 9; ++l) { a += AEL_CHUNK * (d[l] | 1); mx = d[l] > mx ? d[l] : mx; }
    return 4 * (ae_param_count(D, z) + a + 2 * AEL_CHUNK * (mx | 1));
}

static int ae_check(const char* what, int D, int z, int N, const void* workspace) {
    if (D < 1 || D > AEL_MAXW || z < 1 || z > AEL_MAXW) return fail(VATL_EINVAL, "%s: widths must be in 1..64 (D=%d z=%d)", what, D, z);
    if (N < 1) return fail(VATL_EINVAL, "%s: batch %d must be at least 1", what, N);
    if ((long long)N * D > 0x7FFFFFFF) return fail(VATL_EINVAL, "%s: N * D = %lld does not fit 31 bits", what, (long long)N * D);
    if (!workspace || ((uintptr_t)workspace & 3)) return fail(VATL_EINVAL, "%s: workspace (vatl_ae_grad_workspace_floats) missing or misaligned", what);
    return 0;
}

}  // namespace vatl

using namespace vatl;

extern "C" int64_t vatl_ae_grad_workspace_floats(int N, int D, int z) {
    if (N < 1 || D < 1 || D > AEL_MAXW || z < 1 || z > AEL_MAXW) return 0;
    return (int64_t)ae_blocks(N).blocks * (ae_param_count(D, z) + 1);
}

extern "C" int vatl_ae_backward(const float* feat, const float* dy, const float* ae, int D, int z, int N, float* grad, float* dx_or_null,
                                float* workspace, void* stream) {
    if (!feat || !dy || !ae || !grad) return fail(VATL_EINVAL, "ae_backward: null pointer");
    if (int rc = ae_check("ae_backward", D, z, N, workspace)) return rc;
    static std::atomic<unsigned> done{0};
    if (int rc = ensure_dynamic_lds((const void*)ae_grad_partial_kernel<0>, AEL_MAXLDS, done, "ae_grad_partial_kernel<0>")) return rc;
    const AeBlocks b = ae_blocks(N);
    const int P = ae_param_count(D, z);
    hipLaunchKernelGGL(ae_grad_partial_kernel<0>, dim3(b.blocks), dim3(256), ae_lds_bytes(D, z), (hipStream_t)stream, feat, dy, ae, D, z, N,
                       b.chunks_per_block, 0.f, workspace, (float*)nullptr, dx_or_null);
    hipLaunchKernelGGL(ae_grad_finish_kernel<0>, dim3(cdiv(P, 256)), dim3(256), 0, (hipStream_t)stream, workspace, (const float*)nullptr, b.blocks, P,
                       grad, (float*)nullptr, (float*)nullptr, (float*)nullptr, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.0, (float*)nullptr);
    return check_launch("ae_backward");
}

extern "C" int vatl_ae_train_step_large(float* ae, float* m, float* v, const float* feat, int N, int D, int z, double lr, double beta1,
                                        double beta2, double eps, double weight_decay, int step, int decoupled, float* loss_or_null,
                                        float* workspace, void* stream) {
    if (!ae || !m || !v || !feat) return fail(VATL_EINVAL, "ae_train_step_large: null pointer");
    if (int rc = ae_check("ae_train_step_large", D, z, N, workspace)) return rc;
    if (step < 1) return fail(VATL_EINVAL, "ae_train_step_large: step is 1-based");
    if (decoupled != 0 && decoupled != 1) return fail(VATL_EINVAL, "ae_train_step_large: decoupled must be 0 (Adam) or 1 (AdamW)");
    static std::atomic<unsigned> done{0};
    if (int rc = ensure_dynamic_lds((const void*)ae_grad_partial_kernel<1>, AEL_MAXLDS, done, "ae_grad_partial_kernel<1>")) return rc;
    const AeBlocks b = ae_blocks(N);
    const int P = ae_param_count(D, z);
    const double numel = (double)N * D;
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
    float* lossp = workspace + (long long)b.blocks * P;
    hipLaunchKernelGGL(ae_grad_partial_kernel<1>, dim3(b.blocks), dim3(256), ae_lds_bytes(D, z), (hipStream_t)stream, feat, (const float*)nullptr, ae,
                       D, z, N, b.chunks_per_block, (float)(1.0 / numel), workspace, lossp, (float*)nullptr);
    hipLaunchKernelGGL(ae_grad_finish_kernel<1>, dim3(cdiv(P, 256)), dim3(256), 0, (hipStream_t)stream, workspace, lossp, b.blocks, P,
                       (float*)nullptr, ae, m, v, decoupled ? 0.f : (float)weight_decay, decoupled ? (float)(1.0 - lr * weight_decay) : 1.f,
                       (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)sqrt(bc2), (float)eps, (float)(lr / bc1), 1.0 / numel,
                       loss_or_null);
    return check_launch("ae_train_step_large");
}
