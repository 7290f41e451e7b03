"""Accuracy gate of the stride-2 3x3 route (F(4x3,2x2) summed over the four input phases, csrc/winograd_s2_43.hip), checked before the kernel existed (CPU, minutes):
the ORACLE network of SimplePose-R50 with layer2/3/4.0.conv2 replaced by an fp32 emulation of the route, against the float64 network and against plain fp32.
A checker script like f4_accuracy.py, not a collected test (it lives under tests/ because only tests may run the oracle).

    python tests/probes/s2_43_accuracy.py

The emulation: pad the 3x3 filter to 4x4 with zeros, r = 2a + b; phase image P[i][j] = x[2i + by - 1][2j + bx - 1], phase filter g[a][b] = w[2a + by][2b + bx];
V = B4^T d B3 in fp32 per phase, U = G4 g G3^T in float64 rounded once, products and the (phase, channel) reduction in fp32, one output transform A4^T M A3.
In float64 the same code reproduces conv2d(stride 2, pad 1) to 1e-14 (checked first; the zero positions of the single-tap phases are asserted)."""
import os, sys, torch, torch.nn as nn, torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "vatl4pose-wacv2024_amd"))
torch.set_num_threads(8)
T = lambda rows: torch.tensor(rows, dtype=torch.float64)
B4T = T([[2, -1, -2, 1, 0], [0, -2, -1, 1, 0], [0, 2, -3, 1, 0], [0, -1, 0, 1, 0], [0, 2, -1, -2, 1]])
B3T = T([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]])
G4 = T([[0.5, 0], [-0.5, -0.5], [-1 / 6, 1 / 6], [1 / 6, 1 / 3], [0, 1]])
G3 = T([[1, 0], [0.5, 0.5], [0.5, -0.5], [0, -1]])
A4T = T([[1, 1, 1, 1, 0], [0, 1, -1, 2, 0], [0, 1, 1, 4, 0], [0, 1, -1, 8, 1]])
A3T = T([[1, 1, 1, 0], [0, 1, -1, 0], [0, 1, 1, 1]])


class S2Conv(nn.Module):
    def __init__(self, conv, dtype=torch.float32):
        super().__init__()
        assert conv.kernel_size == (3, 3) and conv.stride == (2, 2) and conv.padding == (1, 1) and conv.bias is None
        w4 = F.pad(conv.weight.detach().double(), (0, 1, 0, 1))
        self.dtype, self.U = dtype, []
        for by in range(2):
            for bx in range(2):
                u = torch.einsum("xa,ocab,yb->xyoc", G4, w4[:, :, by::2, bx::2], G3)
                if by:
                    assert float(u[4].abs().max()) == 0.0            # the row position "inf" of the single-tap phases
                if bx:
                    assert float(u[:, 3].abs().max()) == 0.0
                self.U.append(u.to(dtype))

    def forward(self, x):
        n, c, h, w = x.shape
        assert h % 8 == 0 and w % 6 == 0
        xp = F.pad(x.to(self.dtype), (1, 1, 1, 1))
        b4, b3, a4, a3 = (m.to(self.dtype) for m in (B4T, B3T, A4T, A3T))
        M = 0
        for ph in range(4):
            by, bx = ph >> 1, ph & 1
            t = xp[:, :, by::2, bx::2].unfold(2, 5, 4).unfold(3, 4, 3)        # n, c, th, tw, 5, 4
            V = torch.einsum("yj,nchwxj->nchwxy", b3, torch.einsum("xi,nchwij->nchwxj", b4, t))
            M = M + torch.einsum("nchwxy,xyoc->nohwxy", V, self.U[ph])
        Y = torch.einsum("by,nohway->nohwab", a3, torch.einsum("ax,nohwxy->nohway", a4, M))
        return Y.permute(0, 1, 2, 4, 3, 5).reshape(n, -1, h // 2, w // 2)


def selfcheck():
    g = torch.Generator().manual_seed(1)
    conv = nn.Conv2d(16, 8, 3, 2, 1, bias=False).double()
    x = torch.randn((2, 16, 16, 12), generator=g, dtype=torch.float64)
    with torch.no_grad():
        e = float((S2Conv(conv, torch.float64)(x) - conv(x)).abs().max())
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
        cnt = 0
        for name in ("layer2", "layer3", "layer4"):
            b = getattr(ms.preact, name)[0]
            b.conv2 = S2Conv(b.conv2); cnt += 1
        ys = ms(x)
    nrm = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    err = lambda a: float((a.double() - ref64).abs().max() / ref64.abs().max())
    am = lambda a: bool(torch.equal(a.flatten(2).argmax(-1), ref64.flatten(2).argmax(-1)))
    print("replaced", cnt, "stride-2 3x3 layers")
    print("max-norm vs f64: torch fp32 %.3e  route %.3e" % (err(y32), err(ys)))
    print("normwise vs f64: torch fp32 %.3e  route %.3e   route vs torch fp32 %.3e" % (nrm(y32, ref64), nrm(ys, ref64), nrm(ys, y32)))
    print("arg-max equal to f64: torch fp32", am(y32), " route", am(ys))
