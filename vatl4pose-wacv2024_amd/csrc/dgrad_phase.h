// Phase geometry of a DATA GRADIENT run as launch logic on a forward conv kernel (conv_h16.hip for the bf16 fine-tune step,
// conv_f64.hip for the float64 reference): dx = conv(dz, filter with the two channel counts exchanged).  One copy, so that the two
// launchers and their packers cannot drift apart.
// Along one axis, input pixel i = stride*j + ph (phase ph) receives dz[j + d] * w[r] for the taps r = i + pad - stride*(j + d): those of
// the parity of ph + pad under stride 2, all of them under stride 1.  Taken in DESCENDING order r_0 > r_1 > ... they read
// dz[j - pad' + t], t = 0 .. taps-1: a plain stride-1 conv of dz with `taps` taps and padding pad' (which may be negative).
#pragma once
#include "common.h"

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

}  // namespace vatl
