// What the two generic NHWC implicit GEMMs (conv_f64.hip: the float64 reference, conv_h16.hip: the 16-bit route) share around their
// kernels, ONE copy of each: the launch geometry both kernels take by value, its builders, the shape contract of the entry points and
// the index maps of the filter layouts.  The data-gradient phases build on it in dgrad_phase.h.
#pragma once
#include "common.h"

namespace vatl {

// Geometry of one launch.  Output pixel (n, oy, ox) of the Ho x Wo grid reads input (oy*stride - pad_y + r, ox*stride - pad_x + s) and is
// stored at (oy*osy + ooy, ox*osx + oox) of an OH x OW plane (a transposed conv's phase writes every other pixel).
struct ConvGeom {
    long long M;
    int H, W, Cin, Cout, R, S, stride, pad_y, pad_x, Ho, Wo, OH, OW, osy, osx, ooy, oox, relu;
    int out_nchw;                               // write NCHW instead of NHWC; the 16-bit kernel writes fp32 there
};

inline ConvGeom conv_fwd_geom(int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int relu, int out_nchw) {
    const int Ho = (H + 2 * pad - R) / stride + 1, Wo = (W + 2 * pad - S) / stride + 1;
    return ConvGeom{(long long)N * Ho * Wo, H, W, Cin, Cout, R, S, stride, pad, pad, Ho, Wo, Ho, Wo, 1, 1, 0, 0, relu != 0, out_nchw != 0};
}
// phase ph = py*2 + px of ConvTranspose2d(4,2,1): output (2y+py, 2x+px) = 2x2 taps over inputs (y + py - 1 + ty, x + px - 1 + tx)
inline ConvGeom deconv_phase_geom(int N, int H, int W, int Cin, int Cout, int ph, int relu) {
    const int py = ph >> 1, px = ph & 1;
    return ConvGeom{(long long)N * H * W, H, W, Cin, Cout, 2, 2, 1, 1 - py, 1 - px, H, W, 2 * H, 2 * W, 2, 2, py, px, relu != 0, 0};
}

// The shape contract of the forward and data-gradient entry points: R, S <= 7, stride 1 or 2, pad >= 0, the filter fits the padded
// plane.  `arrow` words the channel counts of the message ("->" forward, "<-" data gradient, null: not named); a data-gradient entry
// point (`dgrad`) reports a filter that does not fit with the same words as the rest.
inline int conv_shape_contract(const char* what, const char* arrow, bool dgrad, int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad) {
    const bool fits = H + 2 * pad >= R && W + 2 * pad >= S;
    if (N < 0 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || R < 1 || S < 1 || R > 7 || S > 7 || (stride != 1 && stride != 2) || pad < 0 || (dgrad && !fits)) {
        char channels[48] = "";
        if (arrow) snprintf(channels, sizeof channels, "%d %s %d channels, ", Cin, arrow, Cout);
        return fail(VATL_EINVAL, "%s: N %d, %dx%d, %s%dx%d / %d, pad %d is not served (R, S <= 7, stride 1 or 2)", what, N, H, W, channels, R, S, stride, pad);
    }
    if (!fits) return fail(VATL_EINVAL, "%s: a %dx%d filter does not fit a %dx%d plane with pad %d", what, R, S, H, W, pad);
    return 0;
}

// Filter layouts: element i of the packed buffer -> element of the module's fp32 parameter, or -1 where i is a padded channel (Cinp:
// the channel count as stored; kPadded: the 16-bit types pad it to 8, float64 stores Cinp = Cin).  The pack kernels convert and zero-fill.
// I: the integer type i is divided in (long long; unsigned where the caller knows the buffer has fewer than 2^31 elements: 64-bit division is slow).
// OIHW -> [Cout][R][S][Cinp]
template <bool kPadded, typename I>
__host__ __device__ inline long long conv_weight_src(I i, int Cin, int Cinp, int R, int S) {
    const int c = (int)(i % (I)Cinp);
    I t = i / (I)Cinp;
    const int s = (int)(t % (I)S); t /= (I)S;
    const int r = (int)(t % (I)R);
    const long long co = (long long)(t / (I)R);
    return !kPadded || c < Cin ? ((co * Cin + c) * R + r) * S + s : -1;
}
// ConvTranspose2d(4,2,1) weight (Cin,Cout,4,4) -> [phase = py*2+px][Cout][ty][tx][Cinp], ky = 3-py-2ty, kx = 3-px-2tx
template <bool kPadded, typename I>
__host__ __device__ inline long long deconv_weight_src(I i, int Cin, int Cinp, int Cout) {
    const int c = (int)(i % (I)Cinp);
    I t = i / (I)Cinp;
    const int tx = (int)(t & 1), ty = (int)((t >> 1) & 1); t >>= 2;
    const int co = (int)(t % (I)Cout);
    const int ph = (int)(t / (I)Cout);
    const int ky = 3 - (ph >> 1) - 2 * ty, kx = 3 - (ph & 1) - 2 * tx;
    return !kPadded || c < Cin ? (((long long)c * Cout + co) * 4 + ky) * 4 + kx : -1;
}

static inline int pack_grid(long long n) { long long b = (n + 255) / 256; return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b)); }

}  // namespace vatl
