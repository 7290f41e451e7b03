"""Accuracy gate of the 1-D Winograd stem (F(2,4) on the odd pixels + F(2,3) on the even pixels of every input row, csrc/stem_pool_w1d.hip), checked before the
kernel existed (CPU, minutes): the ORACLE network of SimplePose-R50 with conv1 replaced by an fp32 emulation of the route, against the float64 network and against
plain fp32.  A checker script like s2_43_accuracy.py, not a collected test (it lives under tests/ because only tests may run the oracle).

    python tests/probes/stem_w1d_accuracy.py

The emulation: a row x of the zero-padded image splits into E[q] = x[2q], O[q] = x[2q + 1]; for a fixed (channel, filter row) the stem output is
y[ox] = sum_i w[2i] O[ox + i - 2] + sum_i w[2i + 1] E[ox + i - 1].  Tiles of two outputs (ox = 2t, 2t + 1): V = B4^T O[2t - 2 .. 2t + 2] (5 positions) and
B3^T E[2t - 1 .. 2t + 2] (4 positions) in fp32 with the integer stencils of the kernel, U = G4 w[0::2] and G3 w[1::2] in float64 rounded once, the products and the
(channel, filter row) reduction in fp32, one output transform per tile.  In float64 the same code reproduces conv2d(stride 2, pad 3) to 1e-14 (checked first).
Go when the route's normwise distance to float64 is at most 1.05x plain fp32's in the same run."""
import os, sys, torch, torch.nn as nn, torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "vatl4pose-wacv2024_amd"))
torch.set_num_threads(8)
T = lambda rows: torch.tensor(rows, dtype=torch.float64)
# F(2,4), points 0, 1, -1, 2, inf; rows 0 - 3 of B^T scaled by 2, 2, 6, 6 (integer stencils), the same rows of G divided by them
B4T = T([[2, -1, -2, 1, 0], [0, 2, 1, -1, 0], [0, -2, 3, -1, 0], [0, -1, 0, 1, 0], [0, 2, -1, -2, 1]])
G4 = T([[0.5, 0, 0, 0], [0.5, 0.5, 0.5, 0.5], [1 / 6, -1 / 6, 1 / 6, -1 / 6], [1 / 6, 1 / 3, 2 / 3, 4 / 3], [0, 0, 0, 1]])
A4T = T([[1, 1, 1, 1, 0], [0, 1, -1, 2, 1]])
# F(2,3), points 0, 1, -1, inf; rows 1, 2 of B^T scaled by 2
B3T = T([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, -1, 0, 1]])
G3 = T([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]])
A3T = T([[1, 1, 1, 0], [0, 1, -1, 1]])


class StemW1d(nn.Module):
    def __init__(self, conv, dtype=torch.float32):
        super().__init__()
        assert conv.kernel_size == (7, 7) and conv.stride == (2, 2) and conv.padding == (3, 3) and conv.bias is None
        w = conv.weight.detach().double()                                   # (o, c, ky, kx)
        self.dtype = dtype
        self.U4 = torch.einsum("pi,ocki->pock", G4, w[..., 0::2]).to(dtype)   # odd-pixel taps kx = 0, 2, 4, 6
        self.U3 = torch.einsum("pi,ocki->pock", G3, w[..., 1::2]).to(dtype)   # even-pixel taps kx = 1, 3, 5

    def forward(self, x):
        n, c, h, w = x.shape
        assert h % 2 == 0 and w % 4 == 0
        xp = F.pad(x.to(self.dtype), (3, 5, 3, 3))                          # padded pixel j = image pixel j - 3; even padded = ODD image pixels
        b4, b3, a4, a3 = (m.to(self.dtype) for m in (B4T, B3T, A4T, A3T))
        rows = xp.unfold(2, 7, 2)                                           # n, c, ho, wp, ky: input rows 2 oy + ky - 3
        # odd image pixels O[q] = x[2q + 1] = xp[2q + 4]; tile t needs O[2t - 2 .. 2t + 2] = xp[4t + 0, 2, .., 8]
        od = rows[:, :, :, 0::2].unfold(3, 5, 2)                            # n, c, ho, t, ky, 5
        ev = rows[:, :, :, 1::2].unfold(3, 4, 2)[:, :, :, :w // 4]          # E[2t - 1 .. 2t + 2] = xp[4t + 1, 3, 5, 7]
        V4 = torch.einsum("pj,nchtkj->nchtkp", b4, od)
        V3 = torch.einsum("pj,nchtkj->nchtkp", b3, ev)
        M4 = torch.einsum("nchtkp,pock->nohtp", V4, self.U4)
        M3 = torch.einsum("nchtkp,pock->nohtp", V3, self.U3)
        Y = torch.einsum("ap,nohtp->nohta", a4, M4) + torch.einsum("ap,nohtp->nohta", a3, M3)
        return Y.reshape(n, -1, h // 2, w // 2)


def selfcheck():
    g = torch.Generator().manual_seed(1)
    conv = nn.Conv2d(3, 8, 7, 2, 3, bias=False).double()
    x = torch.randn((2, 3, 16, 24), generator=g, dtype=torch.float64)
    with torch.no_grad():
        e = float((StemW1d(conv, torch.float64)(x) - conv(x)).abs().max())
    assert e < 1e-13, e
    return e


if __name__ == "__main__":
    from oracle import nets, synth
    print("float64 emulation vs conv2d: max |difference|", selfcheck())

    def build(dtype):
        m = nets.SimplePoseRef(50); m.load_state_dict(synth.state_dict_for(m)); return m.to(dtype).eval()
    x = torch.from_numpy(synth.crops(4))
    with torch.no_grad():
        ref64 = build(torch.float64)(x.double())
        y32 = build(torch.float32)(x)
        ms = build(torch.float32)
        ms.preact.conv1 = StemW1d(ms.preact.conv1)
        ys = ms(x)
    nrm = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    err = lambda a: float((a.double() - ref64).abs().max() / ref64.abs().max())
    am = lambda a: bool(torch.equal(a.flatten(2).argmax(-1), ref64.flatten(2).argmax(-1)))
    print("replaced conv1 (7x7 / stride 2 / pad 3)")
    print("max-norm vs f64: torch fp32 %.3e  route %.3e" % (err(y32), err(ys)))
    print("normwise vs f64: torch fp32 %.3e  route %.3e   route vs torch fp32 %.3e" % (nrm(y32, ref64), nrm(ys, ref64), nrm(ys, y32)))
    r = nrm(ys, ref64) / nrm(y32, ref64)
    print("arg-max equal to f64: torch fp32", am(y32), " route", am(ys))
    print("route / plain normwise = %.3f -> %s (bar 1.05)" % (r, "go" if r <= 1.05 else "NO GO"))
