// Deformable convolution (DCN v1 / v2), the ONE statement of its sampling rules: where a tap lands, when it counts, which four
// corners it blends and with what weights.  Plain C++ for host and device: the kernels of deform_conv.hip, the stand-alone CPU
// check (tools/deform_sample_check.cpp) and the float64 oracle of the tests (tests/dcn_cases.py, which states the same rules in
// torch) all rest on it.
//
//   position   py = y*stride - 1 + i + dy,  px = x*stride - 1 + j + dx          (3x3 taps, pad 1, dilation 1)
//   validity   S = 0 unless py > -1 && px > -1 && py < H && px < W; NaN and +-inf fail these comparisons.  The test comes BEFORE
//              any conversion to an integer: no address outside the image is ever formed.
//   corners    (y0, x0) = (floor py, floor px) and its three neighbours; a corner outside [0, H-1] x [0, W-1] contributes 0
//              (its weight is 0 and its index is replaced by 0, a pixel that exists).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define VATL_HD __host__ __device__ __forceinline__
#else
#define VATL_HD inline
#endif

namespace vatl {

struct DeformSample {
    int idx[4];      // y*W + x of the corners (y0,x0) (y0,x1) (y1,x0) (y1,x1); 0 where the corner does not count
    float w[4];      // bilinear weights; 0 where the corner does not count
    float gy[4];     // d w[k] / d py  (0 where the corner does not count)
    float gx[4];     // d w[k] / d px
    int valid;       // the position passed the validity rule (otherwise every weight is 0)
};

// sampling position of tap `tap` (0..2) of output coordinate `o` with learned displacement d
VATL_HD float deform_pos(int o, int stride, int tap, float d) { return (float)(o * stride - 1 + tap) + d; }

VATL_HD DeformSample deform_sample(float py, float px, int H, int W) {
    DeformSample s;
    for (int k = 0; k < 4; ++k) { s.idx[k] = 0; s.w[k] = 0.f; s.gy[k] = 0.f; s.gx[k] = 0.f; }
    s.valid = (py > -1.f && px > -1.f && py < (float)H && px < (float)W) ? 1 : 0;     // false for NaN
    if (!s.valid) return s;
    const float fy = floorf(py), fx = floorf(px);          // in [-1, H-1] x [-1, W-1]: the conversions below are exact and small
    const int y0 = (int)fy, x0 = (int)fx;
    const float ly = py - fy, lx = px - fx, hy = 1.f - ly, hx = 1.f - lx;
    const int ys[2] = {y0, y0 + 1}, xs[2] = {x0, x0 + 1};
    const float wy[2] = {hy, ly}, wx[2] = {hx, lx}, dy[2] = {-1.f, 1.f};
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            const int k = 2 * a + b;
            if (ys[a] >= 0 && ys[a] <= H - 1 && xs[b] >= 0 && xs[b] <= W - 1) {
                s.idx[k] = ys[a] * W + xs[b];
                s.w[k] = wy[a] * wx[b];
                s.gy[k] = dy[a] * wx[b];
                s.gx[k] = wy[a] * dy[b];
            }
        }
    return s;
}

// sigmoid of a DCN v2 mask logit (the mask arrives as logits when it is read straight from conv2_offset's output)
VATL_HD float deform_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

}  // namespace vatl
