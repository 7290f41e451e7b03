// Scorers on decoded poses:
//   wpu           compute_hybrid + AE + MSE           active_learning/Whole_body_AE/*, ActiveLearning.py:364-386
//   ae forward    WholeBodyAE.forward (+ MSE)         Whole_body_AE/AutoEncoder.py:13-39
//   hybrid f64    compute_hybrid on float64 inputs    Whole_body_AE/hybrid_feature.py:14-59
//   oks           compute_OKS                         al_metric.py:42-69
#include "scorer_common.h"

namespace vatl {

// --------------------------------------------------------------------------
// hybrid feature (42 values): (x-gx)/h [17], (y-gy)/h [17], 8 joint-triangle angles; float64 arithmetic on float32 or float64 key-points
// --------------------------------------------------------------------------
// angle t of 8 between the two sides of a joint triangle
template <typename T>
__device__ __forceinline__ double joint_angle(const T* kp, int t) {
    const int tri[8][3] = {{8, 6, 12}, {6, 8, 10}, {5, 7, 9}, {7, 5, 11}, {11, 12, 14}, {12, 11, 13}, {12, 14, 16}, {11, 13, 15}};
    const double x0 = kp[3 * tri[t][0]], y0 = kp[3 * tri[t][0] + 1];
    const double x1 = kp[3 * tri[t][1]], y1 = kp[3 * tri[t][1] + 1];
    const double x2 = kp[3 * tri[t][2]], y2 = kp[3 * tri[t][2] + 1];
    const double eps = 1e-6;
    const double m1 = (y1 - y0) / (x1 - x0 + eps);
    const double m2 = (y2 - y1) / (x2 - x1 + eps);
    return atan(fabs((m1 - m2) / (1.0 + m1 * m2 + eps)));
}

// compute_hybrid on float64 key-points and an (x,y,w,h) box: one thread per item
__global__ void hybrid_f64_kernel(const double* __restrict__ kpts, const double* __restrict__ bbox_xywh, double* __restrict__ feat,
                                  int32_t* __restrict__ status, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double* kp = kpts + (long long)i * 51;
    double* f = feat + (long long)i * 42;
    const double height = bbox_xywh[4 * i + 3];
    double sw = 0.0, sx = 0.0, sy = 0.0;
    for (int j = 0; j < 17; ++j) { const double s = kp[3 * j + 2]; sw += s; sx += kp[3 * j] * s; sy += kp[3 * j + 1] * s; }
    int st = 0;
    if (!(height > 0.0)) st = 1; else if (!(sw > 0.0)) st = 2;
    if (status) status[i] = st;
    if (st) { for (int k = 0; k < 42; ++k) f[k] = __builtin_nan(""); return; }
    const double gx = sx / sw, gy = sy / sw;
    for (int j = 0; j < 17; ++j) { f[j] = (kp[3 * j] - gx) / height; f[17 + j] = (kp[3 * j + 1] - gy) / height; }
    for (int t = 0; t < 8; ++t) f[34 + t] = joint_angle(kp, t);
}

// --------------------------------------------------------------------------
// WholeBodyAE forward: one wave per item, lane l owns feature / neuron l.  csrc/ae_train.hip recomputes this forward pass with
// the same operation order (acc = bias, then fmaf over k ascending), so that its ReLU masks are the ones of this walk.
// --------------------------------------------------------------------------
__device__ __forceinline__ float dense_lane(const float* __restrict__ Wt, const float* __restrict__ bias, int n_out, int n_in,
                                            float h, int lane) {
    // out[lane] = bias[lane] + sum_k W[lane][k] * h_k, h_k broadcast from lane k
    float acc = lane < n_out ? bias[lane] : 0.f;
    for (int k = 0; k < n_in; ++k) {
        const float hk = __shfl(h, k, 64);
        if (lane < n_out) acc = fmaf(Wt[lane * n_in + k], hk, acc);
    }
    return acc;
}

// D -> 24 -> 12 -> 7 -> z -> 7 -> 12 -> 24 -> D on the packed weights (W, b per layer): the reconstruction of x0, lane by lane
__device__ __forceinline__ float ae_forward_lane(const float* ae, int D, int z, float x0, int lane) {
    const int dims[5] = {D, 24, 12, 7, z};
    const float* w = ae;
    float h = x0;
    for (int i = 0; i < 4; ++i) {                               // encoder: ReLU after all but the code layer
        const int ni = dims[i], no = dims[i + 1];
        h = dense_lane(w, w + no * ni, no, ni, h, lane);
        if (i < 3) h = fmaxf(h, 0.f);
        w += no * ni + no;
    }
    for (int i = 4; i > 0; --i) {                               // decoder: ReLU, Sigmoid on the last
        const int ni = dims[i], no = dims[i - 1];
        h = dense_lane(w, w + no * ni, no, ni, h, lane);
        h = i > 1 ? fmaxf(h, 0.f) : 1.f / (1.f + expf(-h));
        w += no * ni + no;
    }
    return h;
}

__global__ __launch_bounds__(256) void ae_forward_kernel(const float* __restrict__ feat, const float* __restrict__ ae, int D, int z,
                                                         float* __restrict__ recon, float* __restrict__ mse, int N) {
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= N) return;
    const float x0 = lane < D ? feat[(long long)item * D + lane] : 0.f;
    const float h = ae_forward_lane(ae, D, z, x0, lane);
    if (recon && lane < D) recon[(long long)item * D + lane] = h;
    const float d = lane < D ? (h - x0) * (h - x0) : 0.f;
    const float s = wave_sum(d);
    if (mse && lane == 0) mse[item] = s / (float)D;
}

// WPU: hybrid feature of a float32 pose and its crop box, auto-encoder, reconstruction MSE
__global__ __launch_bounds__(256) void wpu_kernel(const float* __restrict__ kpts, const float* __restrict__ bbox,
                                                  const float* __restrict__ ae, int D, int z, int only38,
                                                  float* __restrict__ wpu, int32_t* __restrict__ status, int N) {
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= N) return;
    const float* kp = kpts + (long long)item * 51;
    // bbox_xyxy_to_xywh: h = ymax - ymin + 1 (alphapose/utils/bbox.py:96)
    const double height = (double)bbox[item * 4 + 3] - (double)bbox[item * 4 + 1] + 1.0;
    double sw = 0.0, sx = 0.0, sy = 0.0;
    for (int j = 0; j < 17; ++j) {
        const double s = kp[3 * j + 2];
        sw += s; sx += (double)kp[3 * j] * s; sy += (double)kp[3 * j + 1] * s;
    }
    int st = 0;
    if (!(height > 0.0)) st = 1;
    else if (!(sw > 0.0)) st = 2;
    if (st) {
        if (lane == 0) { wpu[item] = __builtin_nanf(""); if (status) status[item] = st; }
        return;
    }
    const double gx = sx / sw, gy = sy / sw;
    double f = 0.0;
    if (lane < 17) f = ((double)kp[3 * lane] - gx) / height;
    else if (lane < 34) f = ((double)kp[3 * (lane - 17) + 1] - gy) / height;
    else if (lane < 42) f = joint_angle(kp, lane - 34);
    // D == 38: the auto-encoder's declared width takes the 38-value subset (drop 3,4,20,21)
    float x0f = (float)f;
    if (D == 38) {
        const int srcl = lane < 3 ? lane : (lane < 18 ? lane + 2 : lane + 4);
        x0f = __shfl(x0f, srcl & 63, 64);
        if (lane >= 38) x0f = 0.f;
    }
    const float h = ae_forward_lane(ae, D, z, x0f, lane);
    float d = 0.f;
    int cnt = D;
    if (lane < D) {
        bool use = true;
        if (only38) use = !(lane == 3 || lane == 4 || lane == 20 || lane == 21);
        d = use ? (h - x0f) * (h - x0f) : 0.f;
    }
    if (only38) cnt = D - 4;
    const float s = wave_sum(d);
    if (lane == 0) { wpu[item] = s / (float)cnt; if (status) status[item] = 0; }
}

// compute_OKS (al_metric.py:42-69): one thread per item, float64 like the numpy original.
__global__ void oks_kernel(const float* __restrict__ pred, const double* __restrict__ gt, const double* __restrict__ bbox_xywh,
                           double* __restrict__ out, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double sig[17] = {.026, .025, .025, .035, .035, .079, .079, .072, .072, .062, .062, .107, .107, .087, .087, .089, .089};
    const double bx = bbox_xywh[4 * i], by = bbox_xywh[4 * i + 1], bw = bbox_xywh[4 * i + 2], bh = bbox_xywh[4 * i + 3];
    const double area = bw * bh + 2.220446049250313e-16;                  // np.spacing(1)
    const float* d = pred + (long long)i * 51;
    const double* g = gt + (long long)i * 51;
    bool any_vis = false;
    for (int k = 0; k < 17; ++k) any_vis |= g[3 * k + 2] > 0.0;
    double acc = 0.0; int cnt = 0;
    for (int k = 0; k < 17; ++k) {
        const double xd = (double)d[3 * k], yd = (double)d[3 * k + 1];
        double dx, dy;
        if (any_vis) {
            if (!(g[3 * k + 2] > 0.0)) continue;
            dx = xd - g[3 * k]; dy = yd - g[3 * k + 1];
        } else {
            dx = fmax(0.0, (bx - bw) - xd) + fmax(0.0, xd - (bx + 2 * bw));
            dy = fmax(0.0, (by - bh) - yd) + fmax(0.0, yd - (by + 2 * bh));
        }
        const double var = (sig[k] * 2) * (sig[k] * 2);
        acc += exp(-((dx * dx + dy * dy) / var / area * 0.5));
        ++cnt;
    }
    out[i] = acc / (double)cnt;
}

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_hybrid_ae_wpu(const float* kpts, const float* bbox, const float* ae, int D, int z, int only38,
                                  float* wpu, int32_t* status, int N, void* stream) {
    if (N <= 0) return 0;
    if (!kpts || !bbox || !ae || !wpu) return fail(VATL_EINVAL, "hybrid_ae_wpu: null pointer");
    if (D != 38 && D != 42) return fail(VATL_EINVAL, "hybrid_ae_wpu: D must be 38 or 42, got %d", D);
    if (z < 1 || z > 64) return fail(VATL_EINVAL, "hybrid_ae_wpu: code width %d out of range", z);
    if (only38 && D != 42) return fail(VATL_EINVAL, "hybrid_ae_wpu: only38 needs D == 42");
    hipLaunchKernelGGL(wpu_kernel, dim3(cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, kpts, bbox, ae, D, z, only38, wpu, status, N);
    return check_launch("hybrid_ae_wpu");
}

extern "C" int vatl_ae_forward(const float* feat, const float* ae, int D, int z, float* recon, float* mse, int N, void* stream) {
    if (N <= 0) return 0;
    if (!feat || !ae || (!recon && !mse)) return fail(VATL_EINVAL, "ae_forward: null pointer");
    if (D < 1 || D > 64 || z < 1 || z > 64) return fail(VATL_EINVAL, "ae_forward: widths must be in 1..64 (D=%d z=%d)", D, z);
    hipLaunchKernelGGL(ae_forward_kernel, dim3(cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, feat, ae, D, z, recon, mse, N);
    return check_launch("ae_forward");
}

extern "C" int vatl_hybrid_feature_f64(const double* kpts, const double* bbox_xywh, double* feat, int32_t* status, int N, void* stream) {
    if (N <= 0) return 0;
    if (!kpts || !bbox_xywh || !feat) return fail(VATL_EINVAL, "hybrid_feature_f64: null pointer");
    hipLaunchKernelGGL(hybrid_f64_kernel, dim3(cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, kpts, bbox_xywh, feat, status, N);
    return check_launch("hybrid_feature_f64");
}

extern "C" int vatl_oks(const float* pred_kpts, const double* gt_kpts, const double* bbox_xywh, double* out, int N, void* stream) {
    if (N <= 0) return 0;
    if (!pred_kpts || !gt_kpts || !bbox_xywh || !out) return fail(VATL_EINVAL, "oks: null pointer");
    hipLaunchKernelGGL(oks_kernel, dim3((unsigned)((N + 127) / 128)), dim3(128), 0, (hipStream_t)stream, pred_kpts, gt_kpts, bbox_xywh, out, N);
    return check_launch("oks");
}
