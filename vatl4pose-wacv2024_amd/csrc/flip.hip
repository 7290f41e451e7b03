// Flip testing of the evaluation stream (alphapose/models/hip_engine_flip.py): the pose network runs on the crops and on their mirror
// image, and the mirrored heat-maps are flipped back, their left / right joints exchanged, and averaged into the first pass's maps.
//   flip_nchw   y[r][w] = x[r][W-1-w]                                            the mirrored fp32 NCHW crops (a move of 32-bit words)
//   flip_merge  hm[n][j][y][x] = (hm[n][j][y][x] + flip[n][src[j]][y][sx(x)]) / 2   in place, fp32 NCHW heat-maps
// with sx(x) = W-1-x, or with shift: sx(0) = W-1, sx(x) = W-x — the reference's flip_heatmap(shift=True), whose
// out[..., 1:] = out[..., 0:-1] moves the flipped row one pixel right and leaves column 0 in place (transforms.py:486-518), followed
// by the decoder's (hms + hms_flip) / 2 (:550-552).  One rounding (the sum); the halving is exact.
//
// Both are HBM-bound.  Where W % 4 == 0 and the tensors are 16-byte aligned a thread owns four consecutive pixels: a row starts on a
// 16-byte boundary then, and so does the mirrored quad W/4-1-q, whose four words are taken in reverse.  With the shift the four sources
// are the upper three words of that quad and the first word of the next one (W-4q), one 4-byte load that the neighbouring thread's quad
// has brought into the cache; the first quad of a row repeats word W-1 instead.  Every other shape takes a thread per pixel.
#include "glue_common.h"

namespace vatl {

__global__ void flip_rows_kernel(const unsigned* __restrict__ x, unsigned* __restrict__ y, long long total, int W) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int w = (int)(i % W);
        y[i] = x[i - w + (W - 1 - w)];
    }
}

// W4 = W / 4 quads a row
__global__ void flip_rows4_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, long long total, int W4) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(i % W4);
        const uint4 s = x[i - q + (W4 - 1 - q)];
        y[i] = make_uint4(s.w, s.z, s.y, s.x);
    }
}

// first element of the hm_flip row that feeds row `row` (= (n * J + j) * H + y) of hm
__device__ __forceinline__ long long flip_src_row(long long row, const int* __restrict__ src_joint, int J, int H) {
    const int y = (int)(row % H);
    const long long nj = row / H;
    const int j = (int)(nj % J);
    return ((nj - j + src_joint[j]) * H + y);
}

__global__ void flip_merge_kernel(float* __restrict__ hm, const float* __restrict__ fl, const int* __restrict__ src_joint, long long total, int J, int H, int W,
                                  int shift) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        const int sx = shift ? (x == 0 ? W - 1 : W - x) : W - 1 - x;
        hm[i] = (hm[i] + fl[flip_src_row(i / W, src_joint, J, H) * W + sx]) * 0.5f;
    }
}

__global__ void flip_merge4_kernel(f32x4* __restrict__ hm, const float* __restrict__ fl, const int* __restrict__ src_joint, long long total, int J, int H, int W4,
                                   int shift) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(i % W4);
        const float* row = fl + flip_src_row(i / W4, src_joint, J, H) * (4LL * W4);
        const f32x4 s = *(const f32x4*)(row + 4 * (W4 - 1 - q));   // words W-4q-4 .. W-4q-1
        f32x4 f;
        if (shift) {
            f[0] = q ? row[4 * (W4 - q)] : s[3];                   // word W-4q; pixel 0 keeps word W-1
            f[1] = s[3]; f[2] = s[2]; f[3] = s[1];
        } else {
            f[0] = s[3]; f[1] = s[2]; f[2] = s[1]; f[3] = s[0];
        }
        hm[i] = (hm[i] + f) * 0.5f;
    }
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_flip_nchw(const float* x, float* y, int64_t rows, int W, void* stream) {
    if (!x || !y || rows < 0 || W < 1) return fail(VATL_EINVAL, "flip_nchw: bad arguments");
    if (x < y + rows * W && y < x + rows * W) return fail(VATL_EINVAL, "flip_nchw: works out of place only (y overlaps x)");
    if (rows == 0) return 0;
    if (!(W & 3) && aligned16(x) && aligned16(y)) {
        const long long total = (long long)rows * (W >> 2);
        hipLaunchKernelGGL(flip_rows4_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, (const uint4*)x, (uint4*)y, total, W >> 2);
    } else {
        const long long total = (long long)rows * W;
        hipLaunchKernelGGL(flip_rows_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, (const unsigned*)x, (unsigned*)y, total, W);
    }
    return check_launch("flip_nchw");
}

extern "C" int vatl_flip_merge(float* hm, const float* hm_flip, const int* src_joint, int N, int J, int H, int W, int shift, void* stream) {
    if (!hm || !hm_flip || !src_joint || N < 0 || J < 1 || H < 1 || W < 1 || (shift != 0 && shift != 1)) return fail(VATL_EINVAL, "flip_merge: bad arguments");
    const long long total = (long long)N * J * H * W;
    if (hm < hm_flip + total && hm_flip < hm + total) return fail(VATL_EINVAL, "flip_merge: hm_flip overlaps hm");
    if (N == 0) return 0;
    if (!(W & 3) && aligned16(hm) && aligned16(hm_flip))
        hipLaunchKernelGGL(flip_merge4_kernel, dim3(ew_grid(total >> 2)), dim3(256), 0, (hipStream_t)stream, (f32x4*)hm, hm_flip, src_joint, total >> 2, J, H, W >> 2,
                           shift);
    else
        hipLaunchKernelGGL(flip_merge_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, hm, hm_flip, src_joint, total, J, H, W, shift);
    return check_launch("flip_merge");
}
