// Phase geometry of a DATA GRADIENT run as launch logic on a forward conv kernel (conv_h16.hip for the bf16 fine-tune step,
// conv_f64.hip for the float64 reference): dx = conv(dz, filter with the two channel counts exchanged).  One copy, so that the two
// launchers and their packers cannot drift apart.
// Along one axis, input pixel i = stride*j + ph (phase ph) receives dz[j + d] * w[r] for the taps r = i + pad - stride*(j + d): those of
// the parity of ph + pad under stride 2, all of them under stride 1.  Taken in DESCENDING order r_0 > r_1 > ... they read
// dz[j - pad' + t], t = 0 .. taps-1: a plain stride-1 conv of dz with `taps` taps and padding pad' (which may be negative).
#pragma once
#include "conv_generic.h"

namespace vatl {

struct DgradAxis { int taps, r0, pad; };        // number of taps, the largest one (tap t is r0 - stride*t), the phase conv's padding
__host__ __device__ inline DgradAxis dgrad_axis(int R, int stride, int pad, int ph) {
    const int par = (ph + pad) % stride;
    DgradAxis a{0, 0, 0};
    if (par > R - 1) return a;                  // no tap reaches this phase (1x1 / stride 2, odd pixels)
    a.r0 = par + (R - 1 - par) / stride * stride;
    a.taps = (a.r0 - par) / stride + 1;
    a.pad = (a.r0 - ph - pad) / stride;         // exact: r0 = ph + pad (mod stride)
    return a;
}
// Packed data-gradient filters: the stride*stride phases one after the other (phase = py*stride + px), each [Cin][ty][tx][Cout] (the
// channel counts as the kernel stores them: padded to 8 for the 16-bit types) with w[co][ci][ry.r0 - stride*ty][rx.r0 - stride*tx];
// every tap belongs to exactly one phase, so the whole buffer has Cin*R*S*Cout elements.  cc = Cin*Cout.
__host__ __device__ inline long long dgrad_phase_offset(int R, int S, int stride, int pad, int phase, long long cc) {
    long long off = 0;
    for (int q = 0; q < phase; ++q) off += cc * dgrad_axis(R, stride, pad, q / stride).taps * dgrad_axis(S, stride, pad, q % stride).taps;
    return off;
}
// OIHW -> element i of ONE phase of that buffer, or -1 for a padded channel (kPadded and I as in conv_generic.h)
template <bool kPadded, typename I>
__host__ __device__ inline long long dgrad_weight_src(I i, DgradAxis ay, DgradAxis ax, int Cout, int Cin, int Coutp, int R, int S, int stride) {
    const int co = (int)(i % (I)Coutp);
    I t = i / (I)Coutp;
    const int tx = (int)(t % (I)ax.taps); t /= (I)ax.taps;
    const int ty = (int)(t % (I)ay.taps);
    const int ci = (int)(t / (I)ay.taps);
    const int r = ay.r0 - stride * ty, s = ax.r0 - stride * tx;
    return !kPadded || (co < Cout && ci < Cin) ? (((long long)co * Cin + ci) * R + r) * S + s : -1;
}

// Phase py*stride + px of the data gradient of a conv (H x W input of Cin channels, Cout output channels) covers the Hp x Wp input
// pixels (stride*j + py, stride*i + px).  Hp or Wp zero: nothing to do.  ay.taps or ax.taps zero: no tap reaches the phase, it is
// filled with the residual.  Otherwise g is launched with the filter at w_off of the packed buffer; roles on the kernel: dz is the input
// (Cout channels on the Ho x Wo plane), dx the output (Cin channels).
struct DgradPhase { int py, px, Hp, Wp; DgradAxis ay, ax; ConvGeom g; long long w_off; };
inline DgradPhase dgrad_phase_geom(int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int phase) {
    const int Ho = (H + 2 * pad - R) / stride + 1, Wo = (W + 2 * pad - S) / stride + 1;
    const int py = phase / stride, px = phase % stride;
    const int Hp = H > py ? (H - py + stride - 1) / stride : 0, Wp = W > px ? (W - px + stride - 1) / stride : 0;
    const DgradAxis ay = dgrad_axis(R, stride, pad, py), ax = dgrad_axis(S, stride, pad, px);
    return DgradPhase{py, px, Hp, Wp, ay, ax,
                      ConvGeom{(long long)N * Hp * Wp, Ho, Wo, Cout, Cin, ay.taps, ax.taps, 1, ay.pad, ax.pad, Hp, Wp, H, W, stride, stride, py, px, 0, 0},
                      dgrad_phase_offset(R, S, stride, pad, phase, (long long)Cin * Cout)};
}

}  // namespace vatl
