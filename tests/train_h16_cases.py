"""What the tests of the opt-in bf16 fine-tune step share (tests/test_train_h16_cpu.py, tests/test_gpu_wgrad_h16.py,
tests/test_gpu_dgrad_h16.py, tests/test_gpu_train_glue_h16.py, tests/test_gpu_train_h16.py): the single-launch case tables, float64
references written from the sums' definitions (tests/test_train_h16_cpu.py pins them to autograd), and the TRAINING ROUNDING SIMULATION.

The simulation is a float64 run of the oracle graph (oracle.nets.SimplePoseRef) in train mode on the host that rounds to the 16-bit type
T exactly where the trainer stores T — the input, the weights, every conv / deconv output z, every BatchNorm (+ residual) (+ ReLU)
output y, the pooled stem output — and, in the backward pass, the gradient with respect to each of those tensors (an autograd function
that rounds both ways).  Everything else is (almost) exact, so what it measures against the plain float64 run is the error a correct
bf16 step cannot avoid.
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.h16_cases import round_to

# ------------------------------------------------------------------------------------------------------ single-launch cases
# name -> (N, Cin, Cout, H, W, R, stride, pad, via_converter)
WGRAD_CASES = {
    "3x3_16to24_5x3_n3": (3, 16, 24, 5, 3, 3, 1, 1, False),        # 45 pixels: less than one k-tile; partial channel tiles both ways
    "3x3s2_8to24_6x4": (2, 8, 24, 6, 4, 3, 2, 1, False),
    "3x3s2_8to24_7x5": (2, 8, 24, 7, 5, 3, 2, 1, False),
    "1x1s2_8to32_5x5": (2, 8, 32, 5, 5, 1, 2, 0, False),
    "1x1_8to8_1x1_n1": (1, 8, 8, 1, 1, 1, 1, 0, False),
    "stem7x7s2_3to64_9x7": (2, 3, 64, 9, 7, 7, 2, 3, True),        # 3 -> 8 channels by the converter, 3 real in dW
    "3x3_512to16_2x2": (2, 512, 16, 2, 2, 3, 1, 1, False),
    "head1x1_16to17_6x5": (2, 16, 17, 6, 5, 1, 1, 0, False),       # dz 17 -> 24 channels by the converter
}
WGRAD_DECONV_CASES = {"deconv_8to8_3x2": (2, 8, 8, 3, 2), "deconv_8to8_1x1": (2, 8, 8, 1, 1)}      # (N, Cin, Cout, H, W)
# the split case: 1x1 8 -> 8 on 66 images of 7x9 = 63 pixels, M = 4158 = 2 * 2048 + 62 pixels (62 is no multiple of 32); image 32 covers
# pixels 2016 .. 2078 and image 65 pixels 4095 .. 4157: an image straddles each chunk boundary (2048, 4096)
WGRAD_SPLIT_CASE = (66, 8, 8, 7, 9, 1, 1, 0, False)
WGRAD_CHUNK = 2048

# name -> (N, Cin, Cout, H, W, R, stride, pad): the data gradient of that conv
DGRAD_CASES = {
    "3x3_16to24_5x3_n3": (3, 16, 24, 5, 3, 3, 1, 1),
    "3x3s2_8to24_6x4": (2, 8, 24, 6, 4, 3, 2, 1),
    "3x3s2_8to24_7x5": (2, 8, 24, 7, 5, 3, 2, 1),                  # odd extents: the four phases have different grids
    "1x1s2_8to32_5x5": (2, 8, 32, 5, 5, 1, 2, 0),
    "head1x1_16to17_6x5": (2, 16, 17, 6, 5, 1, 1, 0),
}
DGRAD_DECONV_CASE = (2, 8, 8, 3, 2)                                # (N, Cin, Cout, H, W) of the ConvTranspose2d(4,2,1)


def out_size(h, r, stride, pad):
    return (h + 2 * pad - r) // stride + 1


# ------------------------------------------------------------------------------------------------------ float64 references
def wgrad_ref(x, dz, r, s, stride, pad):
    """dW[co][ci][a][b] = sum over (n, oy, ox) of dz[n][co][oy][ox] * x[n][ci][oy*stride - pad + a][ox*stride - pad + b], from the
    definition (x, dz NCHW float64).  With |x|, |dz| it is the sum of the terms' absolute values."""
    n, cin, h, w = x.shape
    _, cout, ho, wo = dz.shape
    xp = F.pad(x, (pad, pad, pad, pad))
    dw = torch.zeros(cout, cin, r, s, dtype=x.dtype)
    for a in range(r):
        for b in range(s):
            win = xp[:, :, a:a + stride * (ho - 1) + 1:stride, b:b + stride * (wo - 1) + 1:stride]
            dw[:, :, a, b] = torch.einsum("nchw,ndhw->dc", win, dz)
    return dw


def deconv_wgrad_ref(x, dy):
    """Weight gradient (Cin,Cout,4,4) of ConvTranspose2d(4,2,1) from its input x (N,Cin,H,W) and output gradient dy (N,Cout,2H,2W): the
    conv weight gradient with the roles exchanged (dy is the 4x4 / stride 2 / pad 1 conv's input, x its output gradient)."""
    return wgrad_ref(dy, x, 4, 4, 2, 1)


def _axis_phase(r, stride, pad, ph):
    """Taps of input-pixel phase ph along one axis in DESCENDING order, and the padding of the phase's stride-1 conv of dz."""
    taps = [t for t in range(r - 1, -1, -1) if (t - ph - pad) % stride == 0]
    return taps, ((taps[0] - ph - pad) // stride if taps else 0)


def dgrad_ref_phases(dz, wt, h, w, stride, pad):
    """dx (N,Cin,H,W) of a conv with weight wt (Cout,Cin,R,S) from dz, by the phase decomposition the device launches: input pixels
    (stride*j + py, stride*i + px) are a stride-1 conv of dz with the taps of their parity, in descending order."""
    n, cout = dz.shape[:2]
    cin, r, s = wt.shape[1], wt.shape[2], wt.shape[3]
    dx = torch.zeros(n, cin, h, w, dtype=dz.dtype)
    for py in range(stride):
        ty, pady = _axis_phase(r, stride, pad, py)
        for px in range(stride):
            tx, padx = _axis_phase(s, stride, pad, px)
            hp, wp = len(range(py, h, stride)), len(range(px, w, stride))
            if not ty or not tx or hp == 0 or wp == 0:
                continue
            f = wt[:, :, ty][:, :, :, tx].permute(1, 0, 2, 3)                  # (Cin, Cout, taps_y, taps_x)
            # padding may be negative: pad generously with zeros and crop
            big = max(len(ty), len(tx)) + hp + wp
            dzp = F.pad(dz, (big, big, big, big))
            full = F.conv2d(dzp, f)
            y0, x0 = big - pady, big - padx
            dx[:, :, py::stride, px::stride] = full[:, :, y0:y0 + hp, x0:x0 + wp]
    return dx


# ------------------------------------------------------------------------------------------------------ training rounding simulation
class _RoundBoth(torch.autograd.Function):
    """Identity that rounds the value to T going forward and the gradient to T going back: a tensor the trainer stores as T."""

    @staticmethod
    def forward(ctx, t, dtype):
        ctx.dtype = dtype
        return round_to(t, dtype)

    @staticmethod
    def backward(ctx, g):
        return round_to(g, ctx.dtype), None


class _RoundValue(torch.autograd.Function):
    """Rounds the value and passes the gradient through: the bf16 filter of an fp32 master weight (the weight gradient is fp32)."""

    @staticmethod
    def forward(ctx, t, dtype):
        return round_to(t, dtype)

    @staticmethod
    def backward(ctx, g):
        return g, None


class _RoundGrad(torch.autograd.Function):
    """Passes the value through and rounds the gradient: the fp32 heat-maps, whose gradient the trainer converts to T."""

    @staticmethod
    def forward(ctx, t, dtype):
        ctx.dtype = dtype
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        return round_to(g, ctx.dtype), None


def _rounders(dtype):
    if dtype is None:
        ident = lambda t: t
        return ident, ident, ident
    return (lambda t: _RoundBoth.apply(t, dtype)), (lambda t: _RoundValue.apply(t, dtype)), (lambda t: _RoundGrad.apply(t, dtype))


def simulate_trunk(ref: nn.Module, x, dtype, blocks=None):
    """The trunk of the oracle graph (stem, max-pool, the first ``blocks`` bottlenecks; None = all) walked layer by layer with the
    roundings of the bf16 trainer -> the last block's output (NCHW).  See simulate_train_forward."""
    q, wq, _ = _rounders(dtype)

    def conv(c, t):
        return q(F.conv2d(t, wq(c.weight), None, c.stride, c.padding))

    tr = ref.preact
    y = q(F.relu(tr.bn1(conv(tr.conv1, q(x)))))
    y = q(F.max_pool2d(y, 3, 2, 1))
    for b in [b for stage in (tr.layer1, tr.layer2, tr.layer3, tr.layer4) for b in stage][:blocks]:
        a = q(F.relu(b.bn1(conv(b.conv1, y))))
        a = q(F.relu(b.bn2(conv(b.conv2, a))))
        s = y if b.downsample is None else q(b.downsample[1](conv(b.downsample[0], y)))
        y = q(F.relu(b.bn3(conv(b.conv3, a)) + s))
    return y


def simulate_train_forward(ref: nn.Module, x, dtype):
    """Heat-maps of the oracle graph ``ref`` (oracle.nets.SimplePoseRef in float64, train mode: its BatchNorm modules use batch statistics
    and update their running buffers) walked layer by layer with the roundings of the bf16 trainer; ``dtype`` None = the plain float64
    step (no rounding at all).  Differentiable: ``backward`` of a loss of the result leaves the gradients in ``ref``'s parameters."""
    q, wq, gq = _rounders(dtype)
    y = simulate_trunk(ref, x, dtype)
    d = ref.deconv_layers
    for k in (0, 3, 6):
        z = q(F.conv_transpose2d(y, wq(d[k].weight), None, 2, 1))
        y = q(F.relu(d[k + 1](z)))
    h = ref.final_layer
    return gq(F.conv2d(y, wq(h.weight), h.bias))


def masked_mse(out, target, mask):
    """0.5 * MSE(out * m, target * m) with mean reduction (the fine-tune criterion), m (N,J) broadcast over the plane."""
    m = mask.reshape(mask.shape[0], -1, 1, 1)
    return 0.5 * ((out * m - target * m) ** 2).mean()


