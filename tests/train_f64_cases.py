"""What the tests of the float64 reference gradients share (tests/test_train_f64_cpu.py, tests/test_gpu_wgrad_f64.py,
tests/test_gpu_dgrad_f64.py, tests/test_gpu_train_glue_f64.py, tests/test_gpu_train_f64.py): host statements of the two pieces of host
logic the feature adds — the packed layout of a data-gradient filter with its phase launches, and the split count of the weight
gradient — written from their definitions.  tests/test_train_f64_cpu.py holds them to float64 autograd; the GPU tests then hold the
device to them.  The case tables and sum references are those of tests/train_h16_cases.py.
"""
import torch
import torch.nn.functional as F

from tests import train_h16_cases as TC

U = 2.0 ** -53                       # unit roundoff of float64
WGRAD_CHUNK = 2048                   # VATL_WGRAD_F64_CHUNK: tests/train_h16_cases.WGRAD_SPLIT_CASE straddles its boundaries as well
K_TILE = 16                          # pixels per staged image of csrc/wgrad_f64.hip


def wgrad_splits(m):
    """Number of partial slabs of the weight gradient: a function of the pixel count M only."""
    return 0 if m <= 0 else -(-m // WGRAD_CHUNK)


def dgrad_phases(r, s, stride, pad):
    """[(py, px, taps_y, taps_x, pad_y, pad_x)] in launch order: the taps of each input-pixel phase in DESCENDING order (possibly none)
    and the padding of the phase's stride-1 conv of dz."""
    out = []
    for py in range(stride):
        ty, pady = TC._axis_phase(r, stride, pad, py)
        for px in range(stride):
            tx, padx = TC._axis_phase(s, stride, pad, px)
            out.append((py, px, ty, tx, pady, padx))
    return out


def pack_dgrad_filter(wt, stride, pad):
    """(Cout,Cin,R,S) -> the flat data-gradient filter: the phases one after the other, each [Cin][ty][tx][Cout] with
    w[co][ci][taps_y[ty]][taps_x[tx]]; every tap lands in exactly one phase, so Cin*R*S*Cout elements in all."""
    parts = []
    for _, _, ty, tx, _, _ in dgrad_phases(wt.shape[2], wt.shape[3], stride, pad):
        if ty and tx:
            parts.append(wt[:, :, ty][:, :, :, tx].permute(1, 2, 3, 0).reshape(-1))
    return torch.cat(parts)


def dgrad_from_packed(dz, packed, cin, h, w, r, s, stride, pad, residual=None):
    """dx (N,Cin,H,W) as the device launches it: per phase a stride-1 conv of dz with that phase's slice of the packed filter, written at
    every ``stride``-th pixel; phases no tap reaches are filled with the residual (or zero); the residual is added elsewhere."""
    n, cout = dz.shape[:2]
    dx = torch.zeros(n, cin, h, w, dtype=dz.dtype)
    off = 0
    for py, px, ty, tx, pady, padx in dgrad_phases(r, s, stride, pad):
        hp, wp = len(range(py, h, stride)), len(range(px, w, stride))
        if not ty or not tx:
            continue
        cnt = cin * len(ty) * len(tx) * cout
        f = packed[off:off + cnt].reshape(cin, len(ty), len(tx), cout).permute(0, 3, 1, 2)      # (Cin, Cout, ty, tx): an OIHW filter
        off += cnt
        if hp == 0 or wp == 0:
            continue
        big = max(len(ty), len(tx)) + hp + wp                                                    # padding may be negative: pad and crop
        full = F.conv2d(F.pad(dz, (big, big, big, big)), f)
        y0, x0 = big - pady, big - padx
        dx[:, :, py::stride, px::stride] = full[:, :, y0:y0 + hp, x0:x0 + wp]
    assert off == packed.numel()
    return dx if residual is None else dx + residual


def nhwc(t):
    """Host NCHW -> host NHWC, contiguous (no channel padding: the float64 kernels take any channel count)."""
    return t.permute(0, 2, 3, 1).contiguous()
