#!/usr/bin/env python3
"""Winograd F(2x2,3x3) route against the implicit GEMM on the 3x3 / stride-1 layer shapes: error against float64 and time.

    python tools/wino_bench.py [--batch 1024] [--iters 5] [--layers l1.c2,...] [--check 8]
    python tools/wino_bench.py --deconv43 --iters 10        # the transposed convs: F(3x3,2x2) against F(4x3,2x2)
    python tools/wino_bench.py --s2 --iters 10              # the stride-2 3x3 convs: implicit GEMM against F(4x3,2x2) over the four input phases
    python tools/wino_bench.py --stem --iters 10            # the fused ResNet stem: direct sum against the 1-D Winograd F(2,4) + F(2,3) along the rows

For every shape: max |error| of both routes against a float64 convolution (on `--check` crops), then `iters` launches of
each route between HIP events (TFLOP/s are algorithmic = direct-convolution FLOPs for both).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vatl4pose-wacv2024_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402
import vatl_hip as vh  # noqa: E402

SHAPES = {  # name: (H, W, Cin, Cout, residual)
    "l1.c2": (64, 48, 64, 64, False), "l2.c2": (32, 24, 128, 128, False), "l3.c2": (16, 12, 256, 256, False), "l4.c2": (8, 6, 512, 512, False),
    "hr.b32": (64, 48, 32, 32, True), "hr.b64": (32, 24, 64, 64, True), "hr.b128": (16, 12, 128, 128, True), "hr.b256": (8, 6, 256, 256, True),
    "r152.l2.c2": (48, 36, 128, 128, False), "r152.l3.c2": (24, 18, 256, 256, False), "r152.l4.c2": (12, 9, 512, 512, False),
}
# 3x3 / stride 2 / pad 1 layers (H, W = input grid, Cin, Cout): layer2/3/4.0.conv2 of the 256x192 ResNets (SimplePose, FastPose), and the HRNet-W32 layers the shape
# rule of csrc/winograd_s2_43.hip admits (stem conv2, the transitions, the fuse layers' down-sampling convs with >= 64 output channels)
S2 = {"l2.0.c2": (64, 48, 128, 128), "l3.0.c2": (32, 24, 256, 256), "l4.0.c2": (16, 12, 512, 512)}
S2_HR = {"hr.stem2": (128, 96, 64, 64), "hr.t1": (64, 48, 256, 64), "hr.t2": (32, 24, 64, 128), "hr.t3": (16, 12, 128, 256), "hr.f32-64": (64, 48, 32, 64),
         "hr.f32-128": (32, 24, 32, 128), "hr.f32-256": (16, 12, 32, 256), "hr.f64-64": (32, 24, 64, 64), "hr.f64-256": (16, 12, 64, 256)}
DECONVS = {"deconv1": (8, 6, 2048, 256), "deconv2": (16, 12, 256, 256), "deconv3": (32, 24, 256, 256)}


def timed(fn, iters):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--layers", default="")
    ap.add_argument("--check", type=int, default=8)
    ap.add_argument("--group-kb", type=int, default=-1, help="vatl_tune_set(18, v): KB of filter slices per group of the Winograd tile order")
    ap.add_argument("--halves", type=int, default=0, help="vatl_tune_set(21, v): 32-channel filter halves per Winograd block (1, or 2 where the layer allows)")
    ap.add_argument("--persist", type=int, default=-1, help="vatl_tune_set(22, v): layers with at most v 16-channel stages take the persistent Winograd route (0 = never)")
    ap.add_argument("--deconv43", action="store_true", help="deconv layers only: F(3x3,2x2) against F(4x3,2x2) (csrc/winograd_deconv43.hip), median of 3 alternating loops of --iters launches")
    ap.add_argument("--s2", action="store_true", help="stride-2 3x3 layers only: implicit GEMM against F(4x3,2x2) over the four input phases (csrc/winograd_s2_43.hip), "
                    "median of 3 alternating loops of --iters launches; --layers picks from the flagship's three and the hr.* shapes (default: the flagship's)")
    ap.add_argument("--stem", action="store_true", help="the fused ResNet stem on 256x192 crops only: csrc/stem_pool.hip against csrc/stem_pool_w1d.hip, median of 3 alternating "
                    "loops of --iters launches, each over its own executed-FLOP floor")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.persist >= 0:
        vh.tune_set(22, a.persist)
    if a.group_kb >= 0:
        vh.tune_set(18, a.group_kb)
    if a.halves:
        vh.tune_set(21, a.halves)
    warm = torch.randn((4096, 4096), device=dev)
    for _ in range(100):
        warm @ warm
    torch.cuda.synchronize()
    g = torch.Generator(device="cpu").manual_seed(5)
    if a.stem:
        b, h, w = a.batch, 256, 192
        x = (torch.rand((b, 3, h, w), generator=g) - 0.45).to(dev)
        wt = (torch.randn((64, 3, 7, 7), generator=g) * (2.0 / 147) ** 0.5).to(dev)
        sc = (torch.rand(64, generator=g) + 0.5).to(dev)
        bi = (torch.randn(64, generator=g) * 0.5).to(dev)
        pw, u1d = vh.pack_stem_pool_weight(wt), vh.pack_stem_pool_w1d_weight(wt)
        out = torch.empty((b, h // 4, w // 4, 64), device=dev)
        yd = vh.stem_pool_fwd(x, pw, sc, bi)
        yw = vh.stem_pool_fwd(x, pw, sc, bi, out=out, u1d=u1d)
        k = min(a.check, b)
        ref = torch.nn.functional.conv2d(x[:k].double(), wt.double(), None, 2, 3) * sc.double().view(1, -1, 1, 1) + bi.double().view(1, -1, 1, 1)
        ref = torch.nn.functional.max_pool2d(ref.clamp_min(0), 3, 2, 1).permute(0, 2, 3, 1)
        ed, ew = (yd[:k].double() - ref).abs().max().item(), (yw[:k].double() - ref).abs().max().item()
        full = (yd - yw).abs().max().item()
        del yd
        td, tw = [], []
        for _ in range(3):
            td.append(timed(lambda: vh.stem_pool_fwd(x, pw, sc, bi, out=out), a.iters))
            tw.append(timed(lambda: vh.stem_pool_fwd(x, pw, sc, bi, out=out, u1d=u1d), a.iters))
        md, mw = sorted(td)[1], sorted(tw)[1]
        px = b * (h // 2) * (w // 2)                                                             # stem outputs (bands recompute a few rows more below 512 crops)
        fd = 2.0 * px * 168 * 64 / 157.3e12 * 1e6                                              # executed-FLOP floors at the fp32 MFMA peak, us
        fw = 2.0 * (px // 2) * 9 * 24 * 64 / 157.3e12 * 1e6
        print(f"stem 7x7/2 + pool B={b:5d} direct {md:8.1f} us (floor {fd:7.1f}, {fd / md:.3f}) err {ed:.2e} | 1-D F(2,4)+F(2,3) {mw:8.1f} us (floor {fw:7.1f}, {fw / mw:.3f}) err {ew:.2e} | "
              f"max |difference| {full:.2e}  ref max {ref.abs().max().item():.2f}  speed-up {md / mw:.3f}x of {168 / 108:.3f}  loops {' '.join(f'{v:.1f}' for v in td)} / {' '.join(f'{v:.1f}' for v in tw)}", flush=True)
        return
    names = a.layers.split(",") if a.layers else ([] if a.deconv43 else list(SHAPES)) + list(DECONVS)
    if a.s2:
        names = (list(S2) + list(S2_HR) if a.layers == "all" else a.layers.split(",")) if a.layers else list(S2)
    for name in names:
        if a.s2:
            h, w, cin, cout = {**S2, **S2_HR}[name]
            b = a.batch
            if not vh.conv3x3s2_winograd43_supported(b, h, w, cin, cout):
                print(f"{name:11s} B={b:5d} not a shape of the stride-2 F(4x3,2x2) route", flush=True)
                continue
            x = torch.randn((b, h, w, cin), generator=g).to(dev)
            wt = (torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev)
            sc = (torch.rand(cout, generator=g) + 0.5).to(dev)
            bi = torch.randn(cout, generator=g).to(dev)
            wp, us2 = vh.pack_conv_weight(wt), vh.pack_winograd_s2_43_weight(wt)
            out = torch.empty((b, h // 2, w // 2, cout), device=dev)
            yd = vh.conv2d_fwd(x, wp, sc, bi, cout, 3, 3, 2, 1, True)
            yw = vh.conv2d_fwd(x, wp, sc, bi, cout, 3, 3, 2, 1, True, out=out, u_s2=us2)
            k = min(a.check, b)
            ref = torch.nn.functional.conv2d(x[:k].permute(0, 3, 1, 2).double(), wt.double(), None, 2, 1) * sc.double().view(1, -1, 1, 1) + bi.double().view(1, -1, 1, 1)
            ref = ref.clamp_min(0).permute(0, 2, 3, 1)
            ed, ew = (yd[:k].double() - ref).abs().max().item(), (yw[:k].double() - ref).abs().max().item()
            full = (yd - yw).abs().max().item()
            del yd
            td, tw = [], []
            for _ in range(3):
                td.append(timed(lambda: vh.conv2d_fwd(x, wp, sc, bi, cout, 3, 3, 2, 1, True, out=out), a.iters))
                tw.append(timed(lambda: vh.conv2d_fwd(x, wp, sc, bi, cout, 3, 3, 2, 1, True, out=out, u_s2=us2), a.iters))
            md, mw = sorted(td)[1], sorted(tw)[1]
            m = b * (h // 2) * (w // 2)
            fd = 2.0 * m * 9 * cin * cout / 157.3e12 * 1e6                                      # executed-FLOP floors at the fp32 MFMA peak, us
            fw = 2.0 * ((m // 12 + 31) // 32 * 32) * 72 * cin * cout / 157.3e12 * 1e6
            print(f"{name:11s} B={b:5d} igemm {md:8.1f} us (floor {fd:7.1f}, {fd / md:.3f}) err {ed:.2e} | s2 F(4x3,2x2) {mw:8.1f} us (floor {fw:7.1f}, {fw / mw:.3f}) err {ew:.2e} | "
                  f"max |difference| {full:.2e}  ref max {ref.abs().max().item():.2f}  speed-up {md / mw:.3f}x of 1.5  loops {' '.join(f'{v:.1f}' for v in td)} / {' '.join(f'{v:.1f}' for v in tw)}", flush=True)
            continue
        if name in DECONVS and a.deconv43:
            h, w, cin, cout = DECONVS[name]
            b = a.batch
            x = torch.randn((b, h, w, cin), generator=g).to(dev)
            wt = (torch.randn((cin, cout, 4, 4), generator=g) * (2.0 / (4 * cin)) ** 0.5).to(dev)
            sc = (torch.rand(cout, generator=g) + 0.5).to(dev)
            bi = torch.randn(cout, generator=g).to(dev)
            up, u43 = vh.pack_winograd_deconv_weight(wt), vh.pack_winograd_deconv43_weight(wt)
            if not vh.deconv4x4s2_winograd43_supported(b, h, w, cin, cout):
                print(f"{name:11s} B={b:5d} not a shape of the F(4x3,2x2) route", flush=True)
                continue
            out = torch.empty((b, 2 * h, 2 * w, cout), device=dev)
            y33 = vh.deconv4x4s2_winograd_fwd(x, up, sc, bi, cout, True)
            y43 = vh.deconv4x4s2_winograd_fwd(x, up, sc, bi, cout, True, out=out, u43=u43)
            k = min(a.check, b)
            ref = torch.nn.functional.conv_transpose2d(x[:k].permute(0, 3, 1, 2).double(), wt.double(), None, 2, 1) * sc.double().view(1, -1, 1, 1) + bi.double().view(1, -1, 1, 1)
            ref = ref.clamp_min(0).permute(0, 2, 3, 1)
            e33, e43 = (y33[:k].double() - ref).abs().max().item(), (y43[:k].double() - ref).abs().max().item()
            full = (y33 - y43).abs().max().item()
            del y33
            t33, t43 = [], []
            for _ in range(3):
                t33.append(timed(lambda: vh.deconv4x4s2_winograd_fwd(x, up, sc, bi, cout, True, out=out), a.iters))
                t43.append(timed(lambda: vh.deconv4x4s2_winograd_fwd(x, up, sc, bi, cout, True, out=out, u43=u43), a.iters))
            m33, m43 = sorted(t33)[1], sorted(t43)[1]
            print(f"{name:11s} B={b:5d} F(3x3,2x2) {m33:8.1f} us err {e33:.2e} | F(4x3,2x2) {m43:8.1f} us err {e43:.2e} | max |difference| {full:.2e}  ref max {ref.abs().max().item():.2f}  "
                  f"speed-up {m33 / m43:.3f}x  loops {' '.join(f'{v:.1f}' for v in t33)} / {' '.join(f'{v:.1f}' for v in t43)}", flush=True)
            continue
        if name in DECONVS:
            h, w, cin, cout = DECONVS[name]
            b = a.batch
            x = torch.randn((b, h, w, cin), generator=g).to(dev)
            wt = (torch.randn((cin, cout, 4, 4), generator=g) * (2.0 / (4 * cin)) ** 0.5).to(dev)
            sc = (torch.rand(cout, generator=g) + 0.5).to(dev)
            bi = torch.randn(cout, generator=g).to(dev)
            wp, up = vh.pack_deconv_weight(wt), vh.pack_winograd_deconv_weight(wt)
            yd = vh.deconv4x4s2_fwd(x, wp, sc, bi, cout, True)
            yw = vh.deconv4x4s2_winograd_fwd(x, up, sc, bi, cout, True)
            k = min(a.check, b)
            ref = torch.nn.functional.conv_transpose2d(x[:k].permute(0, 3, 1, 2).double(), wt.double(), None, 2, 1) * sc.double().view(1, -1, 1, 1) + bi.double().view(1, -1, 1, 1)
            ref = ref.clamp_min(0).permute(0, 2, 3, 1)
            ed, ew = (yd[:k].double() - ref).abs().max().item(), (yw[:k].double() - ref).abs().max().item()
            td = timed(lambda: vh.deconv4x4s2_fwd(x, wp, sc, bi, cout, True), a.iters)
            tw = timed(lambda: vh.deconv4x4s2_winograd_fwd(x, up, sc, bi, cout, True), a.iters)
            fl = 2.0 * b * h * w * 4 * cout * cin * 4
            print(f"{name:11s} B={b:5d} direct {td:8.1f} us {fl / td / 1e6:6.1f} TF/s err {ed:.2e} | winograd {tw:8.1f} us {fl / tw / 1e6:6.1f} TF/s err {ew:.2e} "
                  f"| ref max {ref.abs().max().item():.2f}  speed-up {td / tw:.2f}x", flush=True)
            continue
        h, w, cin, cout, res = SHAPES[name]
        b = a.batch
        x = torch.randn((b, h, w, cin), generator=g).to(dev)
        wt = (torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev)
        sc = (torch.rand(cout, generator=g) + 0.5).to(dev)
        bi = torch.randn(cout, generator=g).to(dev)
        r = torch.randn((b, h, w, cout), generator=g).to(dev) if res else None
        wp = vh.pack_conv_weight(wt)
        up = vh.pack_winograd_weight(wt)
        yd = vh.conv2d_fwd(x, wp, sc, bi, cout, 3, 3, 1, 1, True, residual=r)
        yw = vh.conv3x3_winograd_fwd(x, up, sc, bi, cout, True, residual=r)
        k = min(a.check, b)
        ref = torch.nn.functional.conv2d(x[:k].permute(0, 3, 1, 2).double(), wt.double(), padding=1) * sc.double().view(1, -1, 1, 1) + bi.double().view(1, -1, 1, 1)
        if res:
            ref = ref + r[:k].permute(0, 3, 1, 2).double()
        ref = ref.clamp_min(0).permute(0, 2, 3, 1)
        ed = (yd[:k].double() - ref).abs().max().item()
        ew = (yw[:k].double() - ref).abs().max().item()
        full = (yd - yw).abs().max().item()
        td = timed(lambda: vh.conv2d_fwd(x, wp, sc, bi, cout, 3, 3, 1, 1, True, residual=r), a.iters)
        tw = timed(lambda: vh.conv3x3_winograd_fwd(x, up, sc, bi, cout, True, residual=r), a.iters)
        fl = 2.0 * b * h * w * cout * cin * 9
        print(f"{name:11s} B={b:5d} direct {td:8.1f} us {fl / td / 1e6:6.1f} TF/s err {ed:.2e} | winograd {tw:8.1f} us {fl / tw / 1e6:6.1f} TF/s err {ew:.2e} "
              f"| max |direct - winograd| {full:.2e}  ref max {ref.abs().max().item():.2f}  speed-up {td / tw:.2f}x", flush=True)


if __name__ == "__main__":
    main()
