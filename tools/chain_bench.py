#!/usr/bin/env python3
"""conv3 (+ skip + ReLU) of one bottleneck chained with conv1 of the next (vatl_bottleneck_chain_fwd, csrc/bottleneck_chain.hip) against the two tiled launches,
and the forms P (projection block + next conv1, vatl_chain_proj_fwd) and S (last block of the stage + first conv1 of the next, vatl_chain_step_fwd) against the two
launches each replaces: three alternating loops of 10 launches per side, median and spread, beside the MFMA floor (157.3 TFLOP/s) and the compulsory-traffic floor.
usage: chain_bench.py [crops of 64x48 pixels, default 1024] [forms]       ("forms": only P and S)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vatl4pose-wacv2024_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import vatl_hip as vh  # noqa: E402


def timed(fn, it=10):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(it):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / it * 1e3


MFMA_TFLOPS = 157.3       # fp32 matrix rate the layer reports use (profiles/r06_layer_report.txt)
COPY_GBS = float(os.environ.get("VATL_COPY_GBS", "4400"))       # measured copy rate of the box (tools/bw_probe.py), read + write bytes per second


def forms(dev, n, h, w):
    g = torch.Generator(device=dev); g.manual_seed(4)
    rnd = lambda *s: torch.randn(s, device=dev, generator=g)
    m = n * h * w
    a, x, res = rnd(n, h, w, 64), rnd(n, h, w, 64), rnd(n, h, w, 256)
    w3, wpj = rnd(256, 64, 1, 1) / 8, rnd(256, 64, 1, 1) / 8
    s3, b3, sp, bp = torch.rand(256, device=dev, generator=g) + 0.5, rnd(256), torch.rand(256, device=dev, generator=g) + 0.5, rnd(256)
    dual, dbias = vh.pack_conv1x1_dual_weight(w3, s3, b3, wpj, sp, bp)
    w3p = vh.pack_conv_weight(w3)
    t = torch.empty((n, h, w, 256), device=dev)
    for name, n2 in (("P", 64), ("S", 128)):
        w1p = vh.pack_conv_weight(rnd(n2, 256, 1, 1) / 16)
        s1, b1 = torch.rand(n2, device=dev, generator=g) + 0.5, rnd(n2)
        y = torch.empty((n, h, w, n2), device=dev)
        if name == "P":
            first = lambda: vh.conv1x1_rows_fwd(a, dual, None, dbias, 256, True, x2=x, out=t)
            second = lambda: vh.conv2d_fwd(t, w1p, s1, b1, 64, 1, 1, 1, 0, True, out=y)
            fused = lambda: vh.conv1x1_rows_fwd(a, dual, None, dbias, 256, True, x2=x, out=t, next_conv1=(w1p, s1, b1), y1_out=y)
            flops, nbytes = 2.0 * m * 256 * (128 + 64), 4.0 * m * (64 + 64 + 256 + 64)
        else:
            first = lambda: vh.bottleneck_chain_fwd(a, w3p, s3, b3, res, out=t)
            second = lambda: vh.conv1x1_rows_fwd(t, w1p, s1, b1, 128, True, out=y)
            fused = lambda: vh.bottleneck_chain_fwd(a, w3p, s3, b3, res, out=t, y1_out=y, next_stage_conv1=(w1p, s1, b1))
            flops, nbytes = 2.0 * m * 256 * (64 + 128), 4.0 * m * (64 + 256 + 256 + 128)
        first(); second(); torch.cuda.synchronize()
        t_ref, y_ref = t.clone(), y.clone()
        t.zero_(); y.zero_(); fused(); torch.cuda.synchronize()
        print(f"form {name}: T bit-identical: {bool(torch.equal(t, t_ref))}, Y bit-identical: {bool(torch.equal(y, y_ref))}, "
              f"Y rel err {float((y - y_ref).abs().max() / y_ref.abs().max()):.2e}")
        base, new, parts = [], [], []
        for rep in range(3):                                        # alternating loops of 10 launches
            t1, t2 = timed(first), timed(second)
            base.append(timed(lambda: (first(), second()))); new.append(timed(fused)); parts.append((t1, t2))
        med = lambda v: sorted(v)[1]
        print(f"form {name} B={n} {h}x{w}: replaced launches {med([p[0] for p in parts]):7.1f} + {med([p[1] for p in parts]):7.1f} us, back to back {med(base):7.1f} us "
              f"(loops {min(base):.1f} .. {max(base):.1f}) | fused {med(new):7.1f} us (loops {min(new):.1f} .. {max(new):.1f}) | gain {med(base) - med(new):6.1f} us "
              f"({med(base) / med(new):.3f}x) | floors: MFMA {flops / MFMA_TFLOPS / 1e6:6.1f} us, traffic {nbytes / COPY_GBS / 1e3:6.1f} us at {COPY_GBS:.0f} GB/s", flush=True)


def main():
    dev = torch.device("cuda:0")
    warm = torch.randn((4096, 4096), device=dev)
    for _ in range(100):
        warm @ warm
    n, h, w = (int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1024), 64, 48
    if "forms" in sys.argv[1:]:
        return forms(dev, n, h, w)
    g = torch.Generator(device=dev); g.manual_seed(3)
    a = torch.randn((n, h, w, 64), device=dev, generator=g)
    res = torch.randn((n, h, w, 256), device=dev, generator=g)
    w3 = torch.randn((256, 64, 1, 1), device=dev, generator=g) / 8
    w1 = torch.randn((64, 256, 1, 1), device=dev, generator=g) / 16
    s3 = torch.rand(256, device=dev, generator=g) + 0.5; b3 = torch.randn(256, device=dev, generator=g)
    s1 = torch.rand(64, device=dev, generator=g) + 0.5; b1 = torch.randn(64, device=dev, generator=g)
    w3p, w1p = vh.pack_conv_weight(w3), vh.pack_conv_weight(w1)
    t_ref = vh.conv2d_fwd(a, w3p, s3, b3, 256, 1, 1, 1, 0, True, residual=res)
    o_ref = vh.conv2d_fwd(t_ref, w1p, s1, b1, 64, 1, 1, 1, 0, True)
    t = torch.empty_like(t_ref); o = torch.empty_like(o_ref)

    def fused(second=True):
        if second:
            vh.bottleneck_chain_fwd(a, w3p, s3, b3, res, w1p, s1, b1, out=t, y1_out=o)
        else:
            vh.bottleneck_chain_fwd(a, w3p, s3, b3, res, out=t)
    fused(); torch.cuda.synchronize()
    print("T bit-identical:", bool(torch.equal(t, t_ref)), " out2 rel err:", float((o - o_ref).abs().max() / o_ref.abs().max()))
    t.zero_(); fused(False); torch.cuda.synchronize()
    print("first GEMM only, T bit-identical:", bool(torch.equal(t, t_ref)))

    def two():
        vh.conv2d_fwd(a, w3p, s3, b3, 256, 1, 1, 1, 0, True, residual=res, out=t)
        vh.conv2d_fwd(t, w1p, s1, b1, 64, 1, 1, 1, 0, True, out=o)
    for rep in range(2):
        t2 = timed(two); tc3 = timed(lambda: vh.conv2d_fwd(a, w3p, s3, b3, 256, 1, 1, 1, 0, True, residual=res, out=t))
        tf = timed(fused); tf1 = timed(lambda: fused(False))
        print(f"B={n}: tiled conv3 {tc3:7.1f} us, conv3 + conv1 {t2:7.1f} us | fused first GEMM only {tf1:7.1f} us, fused pair {tf:7.1f} us  ({t2 / tf:.2f}x)", flush=True)
    del t_ref, o_ref, t, o
    forms(dev, n, h, w)


if __name__ == "__main__":
    main()
