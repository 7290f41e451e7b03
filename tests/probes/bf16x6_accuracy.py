"""Accuracy gate of the bf16x6 GEMM route (csrc/gemm1x1_bf16x6.hip: every fp32 product of the long-K 1x1 layers as six bf16 MFMAs on exact three-way splits), CPU,
minutes: the ORACLE network of SimplePose-R50 on 4 crops with the 14 in-scope 1x1 convs and the 3 conv3 + projection launches replaced by an emulation of the
kernel, against the float64 network and against plain fp32.  A checker script like stem_w1d_accuracy.py, not a collected test.

    python tests/probes/bf16x6_accuracy.py [--one]        (--one: all six products into ONE accumulator set, the form that was rejected)

The emulation follows the kernel's k order and accumulator assignment: a and w are cut by truncation into hi / mid / lo (csrc/split16.h); K is walked in stages of
16; per stage one instruction adds the 16 products a0 w0 to the first accumulator, then five instructions add a0 w1, a1 w0, a1 w1, a0 w2, a2 w0, in this order, to the
second; the two are added once at the end.  An instruction is modelled as exact products, summed exactly, ONE fp32 rounding of accumulator + sum (float64 carries
the 16 products of 16-bit pieces and the accumulator without error that matters).  The dual launch runs as the kernel does: folded BatchNorm scales multiplied
into the filter rows in fp32, one pair of accumulators over K = C1 + C2, bias1 + bias2 added in the epilogue.  With exact integer data the emulation returns the
integer result (checked first).  Go when the route's normwise distance to float64 is at most 1.05x plain fp32's in the same run."""
import os, sys, torch, torch.nn as nn, torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "vatl4pose-wacv2024_amd"))
torch.set_num_threads(8)
ONE = "--one" in sys.argv


def trunc16(a):
    return (a.contiguous().view(torch.int32) & -65536).view(torch.float32)


def split3(a):
    hi = trunc16(a); r1 = a - hi; mid = trunc16(r1)
    return hi, mid, r1 - mid


def gemm_x6(a, w, one=ONE):
    """a [M][K], w [N][K] fp32 -> [M][N] fp32 as the kernel sums it."""
    m, k = a.shape
    assert k % 16 == 0 and a.dtype == torch.float32 and w.dtype == torch.float32
    ap = [p.double().reshape(m, k // 16, 16) for p in split3(a)]
    wp = [p.double().reshape(-1, k // 16, 16) for p in split3(w)]
    big = torch.zeros((m, w.shape[0]), dtype=torch.float32)
    sml = big if one else torch.zeros_like(big)
    for s in range(k // 16):
        mma = lambda c, i, j: (c.double() + ap[i][:, s] @ wp[j][:, s].T).float()
        big = mma(big, 0, 0)
        if one:
            sml = big
        for i, j in ((0, 1), (1, 0), (1, 1), (0, 2), (2, 0)):
            sml = mma(sml, i, j)
        if one:
            big = sml
    return big if one else big + sml


class Conv1x1X6(nn.Module):
    def __init__(self, conv):
        super().__init__()
        assert conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.bias is None
        self.w = conv.weight.detach()[:, :, 0, 0].contiguous()

    def forward(self, x):
        n, c, h, w = x.shape
        y = gemm_x6(x.permute(0, 2, 3, 1).reshape(-1, c).contiguous(), self.w)
        return y.reshape(n, h, w, -1).permute(0, 3, 1, 2).contiguous()


def fold(bn):
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    return s, bn.bias - bn.running_mean * s


def dual_forward(blk, x):
    """relu(bn3(conv3(y)) + bn_p(conv_p(x))) as ONE GEMM over K = C1 + C2 (the conv3 + projection launch); conv1 through its own replacement when in scope."""
    y = F.relu(blk.bn1(blk.conv1(x)))
    y = F.relu(blk.bn2(blk.conv2(y)))
    s3, b3 = fold(blk.bn3); sp, bp = fold(blk.downsample[1])
    st = blk.downsample[0].stride[0]
    wd = torch.cat([blk.conv3.weight[:, :, 0, 0] * s3[:, None], blk.downsample[0].weight[:, :, 0, 0] * sp[:, None]], 1).contiguous()
    n, c1, h, w = y.shape
    a = torch.cat([y.permute(0, 2, 3, 1).reshape(-1, c1), x[:, :, ::st, ::st].permute(0, 2, 3, 1).reshape(-1, x.shape[1])], 1).contiguous()
    out = gemm_x6(a, wd) + (b3 + bp)
    return F.relu(out.reshape(n, h, w, -1).permute(0, 3, 1, 2).contiguous())


def in_scope(k, k1, n):
    """The shape rule of vatl_gemm1x1_bf16x6_supported, restated."""
    return n % 128 == 0 and k % 64 == 0 and (k >= 512 if k1 == 0 else (k1 >= 64 and k1 % 64 == 0 and k - k1 >= 64 and k >= 384))


def route(model):
    plain = dual = 0
    for name in ("layer1", "layer2", "layer3", "layer4"):
        for blk in getattr(model.preact, name):
            fused = blk.downsample is not None and in_scope(blk.conv3.in_channels + blk.downsample[0].in_channels, blk.conv3.in_channels, blk.conv3.out_channels)
            for cn in ("conv1",) + (() if blk.downsample is not None else ("conv3",)):
                c = getattr(blk, cn)
                if in_scope(c.in_channels, 0, c.out_channels):
                    setattr(blk, cn, Conv1x1X6(c)); plain += 1
            if fused:
                blk.forward = (lambda b: lambda x: dual_forward(b, x))(blk); dual += 1
    return plain, dual


def selfcheck():
    g = torch.Generator().manual_seed(2)
    a = torch.randint(-8, 9, (37, 64), generator=g).float(); w = torch.randint(-4, 5, (24, 64), generator=g).float()
    assert torch.equal(gemm_x6(a, w), a @ w.T)
    a = torch.randn((33, 512), generator=g); w = torch.eye(512)[torch.randperm(512, generator=g)]
    assert torch.equal(gemm_x6(a, w), a @ w.T)                                       # a permutation filter returns the input bits: the split loses nothing


if __name__ == "__main__":
    from oracle import nets, synth
    selfcheck()
    print("emulation on integer data and on a permutation filter: exact")

    def build(dtype):
        m = nets.SimplePoseRef(50); m.load_state_dict(synth.state_dict_for(m)); return m.to(dtype).eval()
    x = torch.from_numpy(synth.crops(4))
    with torch.no_grad():
        ref64 = build(torch.float64)(x.double())
        y32 = build(torch.float32)(x)
        ms = build(torch.float32)
        print("replaced: %d plain 1x1 convs, %d conv3 + projection launches (%s)" % (*route(ms), "ONE accumulator set" if ONE else "two accumulator sets"))
        ys = ms(x)
    nrm = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    err = lambda a: float((a.double() - ref64).abs().max() / ref64.abs().max())
    am = lambda a: bool(torch.equal(a.flatten(2).argmax(-1), ref64.flatten(2).argmax(-1)))
    print("max-norm vs f64: torch fp32 %.3e  route %.3e" % (err(y32), err(ys)))
    print("normwise vs f64: torch fp32 %.3e  route %.3e   route vs torch fp32 %.3e" % (nrm(y32, ref64), nrm(ys, ref64), nrm(ys, y32)))
    r = nrm(ys, ref64) / nrm(y32, ref64)
    print("arg-max equal to f64: torch fp32", am(y32), " route", am(ys))
    print("route / plain normwise = %.3f -> %s (bar 1.05)" % (r, "go" if r <= 1.05 else "NO GO"))
