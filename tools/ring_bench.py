#!/usr/bin/env python3
"""Per-layer timing of the long-K 1x1 launches of the SimplePose-R50 headline step: the plain layers through vatl_conv2d_fwd and the
dual-source conv3 + projection launches through vatl_conv1x1_dual_fwd (the route that serves them: gemm1x1_ring_kernel, or the tiled
implicit GEMM with an older library through VATL_HIP_LIB, or with --ring 0 in the profiling library: build.py --ablation,
VATL_HIP_LIB=.../libvatl_hip_ablation.so).

    python tools/ring_bench.py [--batch 1024] [--iters 10] [--reps 3]

Prints one line per layer: us per launch (median of --reps timed loops of --iters back-to-back launches), TFLOP/s and the fraction of
the 157.3 TFLOP/s fp32 MFMA peak; then, where the library has it, the same launch on the bf16x6 route (u_x6=, csrc/gemm1x1_bf16x6.hip) timed in the
same run, the timed loops of the two alternating: us, speed-up over the fp32 kernel, and the fraction of the route's own MFMA floor, 6/16 of the
fp32 one.  --hrnet adds the trunk shapes at the 384x288 input of the FastPose configs.

Then the short-K, wide-N conv3 layers (128 -> 512 and 256 -> 1024, with the skip and in the SE form without): the row-streaming kernel
(vh.conv1x1_rows_fwd) against the short-K form of the bf16x6 kernel (the same call with u_x6=), alternating loops, with the spread (max - min) of
the row-streaming kernel's loop timings, which a family has to beat at every shape to stay in the shape rule.  --short times these rows alone.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vatl4pose-wacv2024_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402
import vatl_hip as vh  # noqa: E402

PEAK = 157.3e12
# name: (H, W, K, N, residual)
PLAIN = {"l2.n.c1": (32, 24, 512, 128, False), "l3.0.c1": (32, 24, 512, 256, False), "l3.n.c1": (16, 12, 1024, 256, False),
         "l4.0.c1": (16, 12, 1024, 512, False), "l4.n.c1": (8, 6, 2048, 512, False), "l4.n.c3": (8, 6, 512, 2048, True)}
# further plain shapes the bf16x6 shape rule admits (--hrnet): the same (K, N) pairs of a ResNet trunk at the 384x288 input of the FastPose configs (grids 48x36 / 24x18 / 12x9)
OTHER = {"fp.l2.n.c1": (48, 36, 512, 128, False), "fp.l3.0.c1": (48, 36, 512, 256, False), "fp.l3.n.c1": (24, 18, 1024, 256, False),
         "fp.l4.0.c1": (24, 18, 1024, 512, False), "fp.l4.n.c1": (12, 9, 2048, 512, False), "fp.l4.n.c3": (12, 9, 512, 2048, True)}
# name: (H, W, K, N, residual, batch cap): the layers of vatl_gemm1x1_bf16x6_short_supported; --hrnet adds ResNet-152 at 384x288 (256 crops, profiles/r06_rows_bench.txt)
SHORT = {"l2.n.c3": (32, 24, 128, 512, True, 1024), "se.l2.c3": (32, 24, 128, 512, False, 1024),
         "l3.n.c3": (16, 12, 256, 1024, True, 1024), "se.l3.c3": (16, 12, 256, 1024, False, 1024)}
SHORT_OTHER = {"fp.l2.n.c3": (48, 36, 128, 512, True, 256), "fp.l3.n.c3": (24, 18, 256, 1024, True, 256)}
# name: (Ho, Wo, C1, H2, W2, C2, N)  (projection stride 2)
DUAL = {"l2.0.c3+p": (32, 24, 128, 64, 48, 256, 512), "l3.0.c3+p": (16, 12, 256, 32, 24, 512, 1024), "l4.0.c3+p": (8, 6, 512, 16, 12, 1024, 2048)}


def timed(fns, iters, reps, spread=False):
    """Median us per launch of each of `fns`, their timed loops alternating (spread: also max - min of each one's loop timings)."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record(); b.synchronize()
            t.append(a.elapsed_time(b) * 1e3 / iters)
    med = [sorted(t)[len(t) // 2] for t in ts]
    return (med, [max(t) - min(t) for t in ts]) if spread else med


def report(name, shape, fl, us):
    line = f"{name:10s} {shape}  {us[0]:9.1f} us  {fl / us[0] / 1e6:6.1f} TFLOP/s  {fl / us[0] / 1e-6 / PEAK:5.3f} of peak"
    if len(us) > 1:
        line += f"   bf16x6 {us[1]:9.1f} us  {us[0] / us[1]:5.2f}x  {fl / us[1] / 1e-6 / PEAK:5.3f} of the fp32 floor, {fl * 6 / 16 / us[1] / 1e-6 / PEAK:5.3f} of the 6/16 floor"
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hrnet", action="store_true", help="also the trunk shapes at the 384x288 input of the FastPose configs (pass a smaller --batch: 1024 crops of 48x36x512 exceed the 2^30-element guard)")
    ap.add_argument("--short", action="store_true", help="only the short-K conv3 rows (row-streaming kernel against the short-K bf16x6 form)")
    ap.add_argument("--ring", type=int, default=-1, help="vatl_tune_set(27, v) before timing (profiling library only; -1: leave the library default)")
    a = ap.parse_args()
    vh.lib()
    if a.ring >= 0:
        vh.tune_set(27, a.ring)
    n = a.batch
    g = torch.Generator(device="cuda"); g.manual_seed(0)
    total = total6 = 0.0
    x6 = hasattr(vh, "gemm1x1_bf16x6_supported")        # (an older library through VATL_HIP_LIB: the fp32 column alone)
    plain = {} if a.short else dict(PLAIN, **(OTHER if a.hrnet else {}))
    for name, (h, w, k, cout, res) in plain.items():
        x = torch.randn((n, h, w, k), device="cuda", generator=g)
        wp = vh.pack_conv_weight(torch.randn((cout, k, 1, 1), device="cuda", generator=g) / k ** 0.5)
        sc, bi = torch.rand(cout, device="cuda", generator=g) + 0.5, torch.randn(cout, device="cuda", generator=g)
        rs = torch.randn((n, h, w, cout), device="cuda", generator=g) if res else None
        y = torch.empty((n, h, w, cout), device="cuda")
        fns = [lambda: vh.conv2d_fwd(x, wp, sc, bi, cout, 1, 1, 1, 0, True, residual=rs, out=y)]
        if x6 and vh.gemm1x1_bf16x6_supported(n * h * w, k, 0, cout):
            ux6 = vh.pack_gemm1x1_bf16x6_weight(wp)
            fns.append(lambda: vh.conv2d_fwd(x, wp, sc, bi, cout, 1, 1, 1, 0, True, residual=rs, out=y, u_x6=ux6))
        us = timed(fns, a.iters, a.reps)
        total += us[0]; total6 += us[-1]
        report(name, f"{n}x{h}x{w} {k:5d}->{cout:5d}", 2.0 * n * h * w * k * cout, us)
        del x, rs, y
    for name, (ho, wo, c1, h2, w2, c2, cout) in ({} if a.short else DUAL).items():
        x1 = torch.randn((n, ho, wo, c1), device="cuda", generator=g)
        x2 = torch.randn((n, h2, w2, c2), device="cuda", generator=g)
        ones, zeros = torch.ones(cout, device="cuda"), torch.zeros(cout, device="cuda")
        wp, bias = vh.pack_conv1x1_dual_weight(torch.randn((cout, c1, 1, 1), device="cuda", generator=g) / c1 ** 0.5, ones, zeros,
                                               torch.randn((cout, c2, 1, 1), device="cuda", generator=g) / c2 ** 0.5, ones, zeros)
        y = torch.empty((n, ho, wo, cout), device="cuda")
        fns = [lambda: vh.conv1x1_dual_fwd(x1, x2, wp, bias, cout, 2, True, out=y)]
        if x6 and vh.gemm1x1_bf16x6_supported(n * ho * wo, c1 + c2, c1, cout):
            ux6 = vh.pack_gemm1x1_bf16x6_weight(wp)
            fns.append(lambda: vh.conv1x1_dual_fwd(x1, x2, wp, bias, cout, 2, True, out=y, u_x6=ux6))
        us = timed(fns, a.iters, a.reps)
        total += us[0]; total6 += us[-1]
        report(name, f"{n}x{ho}x{wo} {c1}+{c2}->{cout}", 2.0 * n * ho * wo * (c1 + c2) * cout, us)
        del x1, x2, y
    if not a.short:
        print(f"sum of one launch per shape: {total:.1f} us" + (f"   with bf16x6 where admitted: {total6:.1f} us" if x6 else ""), flush=True)
    if not hasattr(vh, "gemm1x1_bf16x6_short_supported"):
        return
    for name, (h, w, k, cout, res, cap) in dict(SHORT, **(SHORT_OTHER if a.hrnet else {})).items():
        nb = min(n, cap)
        x = torch.randn((nb, h, w, k), device="cuda", generator=g)
        wp = vh.pack_conv_weight(torch.randn((cout, k, 1, 1), device="cuda", generator=g) / k ** 0.5)
        sc, bi = torch.rand(cout, device="cuda", generator=g) + 0.5, torch.randn(cout, device="cuda", generator=g)
        rs = torch.randn((nb, h, w, cout), device="cuda", generator=g) if res else None
        y = torch.empty((nb, h, w, cout), device="cuda")
        relu = res                                      # (the SE form has no ReLU in the launch)
        fns = [lambda: vh.conv1x1_rows_fwd(x, wp, sc, bi, cout, relu, residual=rs, out=y)]
        if vh.gemm1x1_bf16x6_short_supported(nb * h * w, k, cout):
            ux6 = vh.pack_gemm1x1_bf16x6_weight(wp)
            fns.append(lambda: vh.conv1x1_rows_fwd(x, wp, sc, bi, cout, relu, residual=rs, out=y, u_x6=ux6))
        us, sp = timed(fns, a.iters, a.reps, spread=True)
        fl = 2.0 * nb * h * w * k * cout
        line = f"{name:10s} {nb}x{h}x{w} {k:5d}->{cout:5d}{' + skip' if res else '       '}  rows {us[0]:9.1f} us (spread {sp[0]:5.1f})"
        if len(us) > 1:
            line += (f"   bf16x6 short {us[1]:9.1f} us (spread {sp[1]:5.1f})  {us[0] / us[1]:5.2f}x  {fl / us[1] / 1e-6 / PEAK:5.3f} of the fp32 floor, "
                     f"{fl * 6 / 16 / us[1] / 1e-6 / PEAK:5.3f} of the 6/16 floor")
        print(line, flush=True)
        del x, rs, y


if __name__ == "__main__":
    main()
