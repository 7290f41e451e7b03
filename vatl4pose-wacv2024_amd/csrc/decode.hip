// Heat-map decoders: each reads the (N,J,H,W) fp32 heat-maps once (HBM-bound), one 256-thread block or one wave per (item, joint) plane.
//   arg-max       heatmap_to_coord_simple             alphapose/utils/transforms.py:550-583
//   soft-arg-max  heatmap_to_coord_simple_regress     transforms.py:586-702  (L1JointRegression configs)
//   pose scores   HP and the json "score"             active_learning/ActiveLearning.py:304-314, 329-330
#include "scorer_common.h"

namespace vatl {

// --------------------------------------------------------------------------
// inverse crop affine of one item's box: control points rounded to float32 like the reference's np.float32 src/dst arrays, the
// transform itself in float64 (cv2.getAffineTransform).  The decoded key-points are bit-identical to the reference's through this.
// --------------------------------------------------------------------------
struct CropAffine {
    float cx32, cy32;
    double g;
};

__device__ __forceinline__ CropAffine crop_affine(const float* bbox, int item, int W) {
    const double xmin = bbox[item * 4 + 0], ymin = bbox[item * 4 + 1];
    const double xmax = bbox[item * 4 + 2], ymax = bbox[item * 4 + 3];
    const double bw = xmax - xmin, bh = ymax - ymin;
    const double cx = xmin + bw * 0.5, cy = ymin + bh * 0.5;
    CropAffine a;
    a.cx32 = (float)cx; a.cy32 = (float)cy;
    const float top32 = (float)(cy + bw * -0.5);
    const float d32 = a.cy32 - top32;
    a.g = (double)d32 / (W * 0.5);
    return a;
}

// heat-map position (u, v) -> image coordinates, stored at dst[0], dst[1]
__device__ __forceinline__ void store_uv(float* dst, const CropAffine& a, float u, float v, int H, int W) {
    dst[0] = (float)((double)a.cx32 + ((double)u - W * 0.5) * a.g);
    dst[1] = (float)((double)a.cy32 + ((double)v - H * 0.5) * a.g);
}

// --------------------------------------------------------------------------
// arg-max decode
// --------------------------------------------------------------------------
// scan step of np.argmax: the first maximum in ascending index order (strict '>'), the first element always, NaN is the maximum
__device__ __forceinline__ void argmax_take(float v, int idx, float& best, int& bidx) {
    if (v > best || bidx == 0x7fffffff || (v != v && best == best)) { best = v; bidx = idx; }
}

// quarter-pixel shift + inverse crop affine + stores of one plane's result (one thread)
__device__ __forceinline__ void decode_finish(const float* __restrict__ src, const float* __restrict__ bbox, float* __restrict__ coords,
                                              float* __restrict__ maxvals, int32_t* __restrict__ idx_out, long long plane, int item,
                                              float best, int bidx, int H, int W, int cs, int ms, int mo) {
    // cs / ms / mo: element stride of a plane's coordinate pair / score and the score's offset — (2, 1, 0) for separate (N,J,2) + (N,J)
    // arrays, (3, 3, 2) with coords == maxvals for the interleaved (N,J,3) key-point rows of vatl_decode_pose
    int px = bidx % W, py = bidx / W;
    if (!(best > 0.f)) { px = 0; py = 0; }                      // pred_mask: maxval <= 0 zeroes the coords
    float u = (float)px, v = (float)py;
    if (1 < px && px < W - 1 && 1 < py && py < H - 1) {
        const float dx = src[py * W + px + 1] - src[py * W + px - 1];
        const float dy = src[(py + 1) * W + px] - src[(py - 1) * W + px];
        u += (dx > 0.f ? 0.25f : (dx < 0.f ? -0.25f : 0.f));
        v += (dy > 0.f ? 0.25f : (dy < 0.f ? -0.25f : 0.f));
    }
    store_uv(coords + plane * cs, crop_affine(bbox, item, W), u, v, H, W);
    maxvals[plane * ms + mo] = best;
    if (idx_out) idx_out[plane] = bidx;
}

__global__ __launch_bounds__(256) void decode_kernel(const float* __restrict__ hm, const float* __restrict__ bbox,
                                                     float* __restrict__ coords, float* __restrict__ maxvals,
                                                     int32_t* __restrict__ idx_out, int J, int H, int W, int cs, int ms, int mo) {
    const int item = blockIdx.x / J;
    const int HW = H * W;
    const float* src = hm + (long long)blockIdx.x * HW;
    const int tid = threadIdx.x;

    float best = -INFINITY;
    int bidx = 0x7fffffff;
    if ((HW & 3) == 0) {
        const int n4 = HW >> 2;
        for (int q = tid; q < n4; q += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) argmax_take(v[e], 4 * q + e, best, bidx);
        }
    } else {
        for (int q = tid; q < HW; q += 256) argmax_take(src[q], q, best, bidx);
    }
    wave_argmax<true>(best, bidx);
    __shared__ float sv[4];
    __shared__ int si[4];
    block4_put(sv, best); block4_put(si, bidx);
    __syncthreads();
    if (tid != 0) return;
    block4_argmax<true>(sv, si, best, bidx);
    decode_finish(src, bbox, coords, maxvals, idx_out, (long long)blockIdx.x, item, best, bidx, H, W, cs, ms, mo);
}

// one wave per plane (scorer_common.h): same ordering rules, same finish
template <int NV>
__global__ __launch_bounds__(256) void decode_wave_kernel(const float* __restrict__ hm, const float* __restrict__ bbox,
                                                          float* __restrict__ coords, float* __restrict__ maxvals,
                                                          int32_t* __restrict__ idx_out, int planes, int J, int H, int W, int cs, int ms, int mo) {
    const int lane = threadIdx.x & 63;
    const long long plane = wave_plane();
    if (plane >= planes) return;
    const float* src = hm + plane * (64LL * NV * 4);
    f32x4 v[NV];
    load_plane<NV>(src, lane, v);
    float best = -INFINITY;
    int bidx = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) argmax_take(v[k][e], 4 * (k * 64 + lane) + e, best, bidx);
    wave_argmax<true>(best, bidx);
    if (lane == 0) decode_finish(src, bbox, coords, maxvals, idx_out, plane, (int)(plane / J), best, bidx, H, W, cs, ms, mo);
}

// Per-item pose scores from the interleaved key-point rows: HP = -np.sum(scores) (ActiveLearning.py:329-330) and the json "score" =
// np.mean(scores) + 1.25 np.max(scores) (:314), with NumPy's float32 pairwise summation order (8 running sums over the leading multiple
// of 8, combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the tail added in order; halves of a run longer than 128 summed separately) —
// HP is bit-identical to the reference's float32 np.sum, not merely close.  One thread per item.
__device__ float np_pairwise_sum(const float* a, int n, int stride) {
    if (n < 8) {
        float r = 0.f;
        for (int i = 0; i < n; ++i) r += a[i * stride];
        return r;
    }
    if (n <= 128) {
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = a[j * stride];
        int i = 8;
        for (; i < n - (n % 8); i += 8)
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += a[(i + j) * stride];
        float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i * stride];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_sum(a, n2, stride) + np_pairwise_sum(a + (long long)n2 * stride, n - n2, stride);
}

__global__ void pose_scores_kernel(const float* __restrict__ kpts, float* __restrict__ hp, double* __restrict__ pose_score, int N, int J) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float* sc = kpts + (long long)i * J * 3 + 2;
    const float sum = np_pairwise_sum(sc, J, 3);
    float mx = sc[0];
    for (int j = 1; j < J; ++j) {                              // np.max: NaN propagates
        const float v = sc[j * 3];
        if (v > mx || v != v) mx = (mx != mx) ? mx : v;
    }
    if (hp) hp[i] = -sum;
    // float(np.mean(s) + 1.25 * np.max(s)) under the reference's pinned numpy==1.23.5 (pyproject.toml:35): np.mean of float32 scores is a float32
    // scalar (pairwise sum / J, correctly rounded); `1.25 * np.float32` is a python float times a NumPy SCALAR, which numpy 1.x promotes to float64,
    // so the product (exact in float64) and the sum (one rounding, in float64) are doubles and the json "score" is that double.  (NumPy >= 2 keeps the
    // whole expression in float32; round 5 followed that and was up to 1 ulp of float32 away from the reference's file.  alphapose/utils/bbox.py
    // follows the same 1.23 promotion for _center_scale_to_box.)
    if (pose_score) pose_score[i] = (double)(sum / (float)J) + 1.25 * (double)mx;
}

// --------------------------------------------------------------------------
// soft-arg-max decode
// --------------------------------------------------------------------------
template <int NORM>   // 0 softmax, 1 sigmoid, 2 divide_sum
__device__ __forceinline__ float softargmax_prob(float v, float mx) {
    if (NORM == 0) return expf(v - mx);
    if (NORM == 1) return 1.f / (1.f + expf(-v));
    return v;
}

// expectation -> /W - 0.5 -> (c + 0.5) * W, in float32 like the reference's tensors; inverse crop affine; stores (one thread)
template <int NORM>
__device__ __forceinline__ void softargmax_finish(const float* bbox, float* coords, float* scores,
                                                  long long plane, int item, double s, double sx, double sy, float mx, int H, int W) {
    const float ex = (float)(sx / s), ey = (float)(sy / s);
    const float u = ((ex / (float)W - 0.5f) + 0.5f) * (float)W;
    const float v = ((ey / (float)H - 0.5f) + 0.5f) * (float)H;
    store_uv(coords + plane * 2, crop_affine(bbox, item, W), u, v, H, W);
    scores[plane] = NORM == 1 ? 1.f / (1.f + expf(-mx)) : 1.f;
}

template <int NORM>
__global__ __launch_bounds__(256) void softargmax_kernel(const float* __restrict__ hm, const float* __restrict__ bbox,
                                                         float* __restrict__ coords, float* __restrict__ scores, int J, int H, int W) {
    const int item = blockIdx.x / J;
    const int HW = H * W;
    const float* gsrc = hm + (long long)blockIdx.x * HW;
    const int tid = threadIdx.x;
    extern __shared__ __attribute__((aligned(16))) float plane[];   // the plane is read from HBM once
    __shared__ float red[4];
    __shared__ double dred[3][4];
    float mx = -INFINITY;
    const int step = (HW & 3) == 0 ? 4 : 1;            // 16-byte loads when the plane allows it
    if (step == 4) {
        for (int q = tid; q < (HW >> 2); q += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(gsrc + 4 * q);
            *reinterpret_cast<f32x4*>(plane + 4 * q) = v;
            mx = fmaxf(fmaxf(mx, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
        }
    } else {
        for (int q = tid; q < HW; q += 256) { const float v = gsrc[q]; plane[q] = v; mx = fmaxf(mx, v); }
    }
    const float* src = plane;                          // each thread re-reads only what it wrote
    block4_put(red, wave_max(mx));
    __syncthreads();
    mx = block4_max(red);
    double s = 0.0, sx = 0.0, sy = 0.0;
    const float inv_w = 1.0f / (float)W;
    for (int q0 = tid * step; q0 < HW; q0 += 256 * step)
        for (int q = q0; q < q0 + step; ++q) {
            const float p = softargmax_prob<NORM>(src[q], mx);
            const int y = fast_div(q, inv_w), x = q - y * W;
            s += p; sx += (double)p * x; sy += (double)p * y;
        }
    block4_put(dred[0], wave_sum(s)); block4_put(dred[1], wave_sum(sx)); block4_put(dred[2], wave_sum(sy));
    __syncthreads();
    if (tid != 0) return;
    softargmax_finish<NORM>(bbox, coords, scores, (long long)blockIdx.x, item, block4_sum(dred[0]), block4_sum(dred[1]), block4_sum(dred[2]), mx, H, W);
}

// one wave per plane (scorer_common.h): same arithmetic
template <int NORM, int NV>
__global__ __launch_bounds__(256) void softargmax_wave_kernel(const float* __restrict__ hm, const float* __restrict__ bbox,
                                                              float* __restrict__ coords, float* __restrict__ scores, int planes, int J, int H, int W) {
    const int lane = threadIdx.x & 63;
    const long long plane = wave_plane();
    if (plane >= planes) return;
    const int item = (int)(plane / J);
    f32x4 v[NV];
    load_plane<NV>(hm + plane * (64LL * NV * 4), lane, v);
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < NV; ++k) mx = fmaxf(fmaxf(mx, fmaxf(v[k][0], v[k][1])), fmaxf(v[k][2], v[k][3]));
    mx = wave_max(mx);
    double s = 0.0, sx = 0.0, sy = 0.0;
    const float inv_w = 1.0f / (float)W;
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float p = softargmax_prob<NORM>(v[k][c], mx);
            const int q = 4 * (k * 64 + lane) + c;
            const int y = fast_div(q, inv_w), x = q - y * W;
            s += p; sx += (double)p * x; sy += (double)p * y;
        }
    s = wave_sum(s); sx = wave_sum(sx); sy = wave_sum(sy);
    if (lane != 0) return;
    softargmax_finish<NORM>(bbox, coords, scores, plane, item, s, sx, sy, mx, H, W);
}

}  // namespace vatl

using namespace vatl;

static int decode_launch(const float* hm, const float* bbox, float* coords, float* maxvals, int32_t* idx, int N, int J, int H, int W, int cs, int ms,
                         int mo, hipStream_t st) {
    const long long planes = (long long)N * J;
    const int nv = wave_route_nv(hm, planes, H, W);
    if (nv == 12)
        hipLaunchKernelGGL(decode_wave_kernel<12>, dim3(cdiv(planes, 4)), dim3(256), 0, st, hm, bbox, coords, maxvals, idx, (int)planes, J, H, W, cs, ms, mo);
    else if (nv == 27)
        hipLaunchKernelGGL(decode_wave_kernel<27>, dim3(cdiv(planes, 4)), dim3(256), 0, st, hm, bbox, coords, maxvals, idx, (int)planes, J, H, W, cs, ms, mo);
    else
        hipLaunchKernelGGL(decode_kernel, dim3(N * J), dim3(256), 0, st, hm, bbox, coords, maxvals, idx, J, H, W, cs, ms, mo);
    return check_launch("decode_argmax_affine");
}

extern "C" int vatl_decode_argmax_affine(const float* hm, const float* bbox, float* coords, float* maxvals, int32_t* idx,
                                         int N, int J, int H, int W, void* stream) {
    if (N <= 0) return 0;
    if (!hm || !bbox || !coords || !maxvals) return fail(VATL_EINVAL, "decode_argmax_affine: null pointer");
    return decode_launch(hm, bbox, coords, maxvals, idx, N, J, H, W, 2, 1, 0, (hipStream_t)stream);
}

extern "C" int vatl_decode_pose(const float* hm, const float* bbox, float* kpts, int32_t* idx, float* hp, double* pose_score, int N, int J, int H, int W,
                                void* stream) {
    if (N <= 0) return 0;
    if (!hm || !bbox || !kpts) return fail(VATL_EINVAL, "decode_pose: null pointer");
    if (int rc = decode_launch(hm, bbox, kpts, kpts, idx, N, J, H, W, 3, 3, 2, (hipStream_t)stream)) return rc;
    if (hp || pose_score) {
        hipLaunchKernelGGL(pose_scores_kernel, dim3(cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, kpts, hp, pose_score, N, J);
        return check_launch("pose_scores");
    }
    return 0;
}

template <int NORM>
static void softargmax_launch(const float* hm, const float* bbox, float* coords, float* scores, int N, int J, int H, int W, size_t smem, hipStream_t st) {
    const long long planes = (long long)N * J;
    const int nv = wave_route_nv(hm, planes, H, W);
    if (nv == 12) hipLaunchKernelGGL((softargmax_wave_kernel<NORM, 12>), dim3(cdiv(planes, 4)), dim3(256), 0, st, hm, bbox, coords, scores, (int)planes, J, H, W);
    else if (nv == 27) hipLaunchKernelGGL((softargmax_wave_kernel<NORM, 27>), dim3(cdiv(planes, 4)), dim3(256), 0, st, hm, bbox, coords, scores, (int)planes, J, H, W);
    else hipLaunchKernelGGL(softargmax_kernel<NORM>, dim3(N * J), dim3(256), smem, st, hm, bbox, coords, scores, J, H, W);
}

extern "C" int vatl_decode_softargmax(const float* hm, const float* bbox, float* coords, float* scores,
                                      int N, int J, int H, int W, int norm_type, void* stream) {
    if (N <= 0) return 0;
    if (!hm || !bbox || !coords || !scores) return fail(VATL_EINVAL, "decode_softargmax: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t smem = (size_t)H * W * sizeof(float);
    if (smem > 60 * 1024) return fail(VATL_EINVAL, "decode_softargmax: heat-map %dx%d too large for the LDS tile", H, W);
    if (norm_type == 0) softargmax_launch<0>(hm, bbox, coords, scores, N, J, H, W, smem, st);
    else if (norm_type == 1) softargmax_launch<1>(hm, bbox, coords, scores, N, J, H, W, smem, st);
    else if (norm_type == 2) softargmax_launch<2>(hm, bbox, coords, scores, N, J, H, W, smem, st);
    else return fail(VATL_EINVAL, "decode_softargmax: norm_type must be 0 (softmax), 1 (sigmoid) or 2 (divide_sum)");
    return check_launch("decode_softargmax");
}
