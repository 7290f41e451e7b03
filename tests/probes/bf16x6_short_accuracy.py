"""Accuracy gate of the short-K form of the bf16x6 GEMM route (csrc/gemm1x1_bf16x6.hip, gemm1x1_bf16x6_short_kernel: conv3 of ResNet stages 2 and 3), CPU, minutes:
the probe of the long-K route (tests/probes/bf16x6_accuracy.py, whose emulation this script imports unchanged — the short form has the same k order, products and
accumulator assignment) with the conv3 layers the short rule admits added to its scope: on SimplePose-R50 the 14 + 8 plain 1x1 convs and the 3 conv3 + projection
launches, against the float64 network and against plain fp32.  A checker script, not a collected test.

    python tests/probes/bf16x6_short_accuracy.py

Go when the route's normwise distance to float64 is at most 1.05x plain fp32's in the same run."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16x6_accuracy as long_k  # noqa: E402


def in_scope_short(k, n):
    """The shape rule of vatl_gemm1x1_bf16x6_short_supported, restated."""
    return k % 64 == 0 and 128 <= k < 512 and n % 256 == 0 and n >= 512


def route_short(model):
    """The identity-shortcut conv3 layers the short rule admits (the BatchNorm, the skip and the ReLU stay in the module, as in the long-K probe)."""
    count = 0
    for name in ("layer1", "layer2", "layer3", "layer4"):
        for blk in getattr(model.preact, name):
            c = blk.conv3
            if blk.downsample is None and not isinstance(c, long_k.Conv1x1X6) and in_scope_short(c.in_channels, c.out_channels):
                blk.conv3 = long_k.Conv1x1X6(c); count += 1
    return count


if __name__ == "__main__":
    from oracle import nets, synth
    long_k.selfcheck()
    print("emulation on integer data and on a permutation filter: exact")

    def build(dtype):
        m = nets.SimplePoseRef(50); m.load_state_dict(synth.state_dict_for(m)); return m.to(dtype).eval()
    x = torch.from_numpy(synth.crops(4))
    with torch.no_grad():
        ref64 = build(torch.float64)(x.double())
        y32 = build(torch.float32)(x)
        ms = build(torch.float32)
        plain, dual = long_k.route(ms)
        short = route_short(ms)
        print("replaced: %d long-K + %d short-K plain 1x1 convs, %d conv3 + projection launches (two accumulator sets)" % (plain, short, dual))
        assert (plain, short, dual) == (14, 8, 3)
        ys = ms(x)
    nrm = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    err = lambda a: float((a.double() - ref64).abs().max() / ref64.abs().max())
    am = lambda a: bool(torch.equal(a.flatten(2).argmax(-1), ref64.flatten(2).argmax(-1)))
    print("max-norm vs f64: torch fp32 %.3e  route %.3e" % (err(y32), err(ys)))
    print("normwise vs f64: torch fp32 %.3e  route %.3e   route vs torch fp32 %.3e" % (nrm(y32, ref64), nrm(ys, ref64), nrm(ys, y32)))
    r = nrm(ys, ref64) / nrm(y32, ref64)
    print("arg-max equal to f64: torch fp32", am(y32), " route", am(ys))
    print("route / plain normwise = %.3f -> %s (bar 1.05)" % (r, "go" if r <= 1.05 else "NO GO"))
