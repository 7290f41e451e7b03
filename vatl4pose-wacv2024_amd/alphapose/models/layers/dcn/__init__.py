"""Deformable convolution v1 / v2 modules (reference: alphapose/models/layers/dcn/deform_conv.py:190-337) on the gfx950 kernels of
csrc/deform_conv.hip.  Same constructor signatures, attribute names, asserts and parameter keys; 3x3 / pad 1 / dilation 1 /
groups 1 only (what the Bottleneck uses).  Deformable RoI pooling is not provided.

The modules work on their own with NCHW tensors and autograd: one ``torch.autograd.Function`` over the column route —
``deform_columns`` writes the sampled, mask-weighted matrix, the 1x1 GEMMs multiply it; backward = weight gradient and data
gradient of that GEMM, then ``deform_columns_bwd``.  By default its dx is accumulated with float atomics, so a gradient through a
deformable layer is reproducible in value, not in bits.  The ordered path sums the same terms through an inverted index in one fixed
order: with it every gradient of a deformable layer, and so a DCN network's fine-tune step, is bit-reproducible.  It is switched on
by ``set_deterministic(True)``, inside ``with deterministic():``, or — the switch's default, None — whenever
``torch.are_deterministic_algorithms_enabled()`` or ``torch.backends.cudnn.deterministic`` is true (what the driver's ``--seedfix``
sets); ``set_deterministic(False)`` keeps the atomics whatever torch says.  The switch is read when a backward runs.

Inside a pose network the inference plan (hip_engine) and the trainer (hip_train) call the same kernels on NHWC tensors directly,
conv2_offset included.  The two ``...Pack`` classes own their offset conv as an ordinary ``nn.Conv2d`` and evaluate it with torch
before the deformable kernels run; no network of this package uses them.
"""
import contextlib
import math

import torch
import torch.nn as nn
from torch.nn.modules.utils import _pair

import vatl_hip as vh

__all__ = ["DeformConv", "DeformConvPack", "ModulatedDeformConv", "ModulatedDeformConvPack", "deform_conv", "modulated_deform_conv",
           "set_deterministic", "is_deterministic", "deterministic"]


def set_deterministic(mode):
    """The process switch of the deformable backward's dx: True = the ordered, bit-reproducible path, False = float atomics, None (the
    default) = follow torch (``torch.are_deterministic_algorithms_enabled()`` or ``torch.backends.cudnn.deterministic``)."""
    vh.set_deform_deterministic(mode)


def is_deterministic() -> bool:
    """Whether a deformable backward that ran now would take the ordered path."""
    return vh.deform_deterministic()


@contextlib.contextmanager
def deterministic(mode=True):
    """``with deterministic():`` the ordered path (or ``mode``) for the backwards that run inside; the previous setting returns."""
    before = vh.deform_deterministic_mode()
    vh.set_deform_deterministic(mode)
    try:
        yield
    finally:
        vh.set_deform_deterministic(before)


def _pad32(c: int) -> int:
    return (c + 31) // 32 * 32


def check_geometry(weight, stride, padding, dilation, groups):
    """The one geometry the kernels serve; everything else is refused loudly."""
    if tuple(weight.shape[2:]) != (3, 3) or _pair(padding) != (1, 1) or _pair(dilation) != (1, 1) or groups != 1 \
            or _pair(stride) not in ((1, 1), (2, 2)):
        raise NotImplementedError("deformable convolution: only 3x3, padding 1, dilation 1, groups 1, stride 1 or 2 is implemented")
    return _pair(stride)[0]


def columns_forward(xh, oh, mask, weight, stride: int, dg: int):
    """NHWC column route: -> (col, wg): the column matrix and the filter as the (Cout,K,1,1) 1x1 conv that multiplies it."""
    return vh.deform_columns(xh, oh, mask, stride, dg), vh.deform_gemm_weight(weight)


def columns_backward(dzh, col, wg, xh, oh, mask, weight, stride: int, dg: int, grad_channels=None, dw_out=None, deterministic=None):
    """dzh (N,Ho,Wo,pad32(Cout)) NHWC, zero behind Cout -> (dx NHWC, d_offset, d_mask, dw (Cout,C,3,3)).  ``deterministic``: the
    dx path (None = the process switch, resolved here)."""
    co, c = weight.shape[:2]
    k = wg.shape[1]
    n, ho, wo, _ = col.shape
    dwk = vh.conv2d_wgrad(col, dzh, co, k, 1, 1, 1, 0)                                   # (Cout,K,1,1), column t * C + c
    dw = dwk.view(co, k)[:, :9 * c].reshape(co, 3, 3, c).permute(0, 3, 1, 2)
    if dw_out is not None:
        dw_out.view(co, c, 3, 3).copy_(dw)
        dw = dw_out
    else:
        dw = dw.contiguous()
    wd = vh.pack_dgrad_weight(wg, [(0, 0)], cout_k=dzh.shape[3], planned=False)
    dcol = vh.conv2d_fwd_ex(dzh, wd, k, 1, 1, 1, 0, 0, ho, wo, ho, wo, 1, 1, 0, 0)
    dx, d_off, d_mask = vh.deform_columns_bwd(dcol, xh, oh, mask, stride, dg, grad_channels=grad_channels,
                                              deterministic=is_deterministic() if deterministic is None else bool(deterministic))
    return dx, d_off, d_mask, dw


class _DeformConvFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, offset, mask, weight, bias, stride, dg):
        if not x.is_cuda:
            raise vh.VatlError("deformable convolution runs on MI355X only (there is deliberately no CPU fallback)")
        co, c = weight.shape[:2]
        if not vh.deform_conv2d_supported(c, co, stride, dg):
            raise NotImplementedError(f"deformable convolution: {c} -> {co} channels (multiples of 16), {dg} deformable groups (1, 2, 4) not served")
        with torch.no_grad():
            xh = vh.nchw_to_nhwc(x.detach().float().contiguous())
            oh = vh.nchw_to_nhwc(offset.detach().float().contiguous())
            mh = None if mask is None else vh.nchw_to_nhwc(mask.detach().float().contiguous())
            col, wg = columns_forward(xh, oh, mh, weight.detach().float(), stride, dg)
            b = None if bias is None else vh.bn_fold(None, None, None, None, 0.0, bias.detach(), channels=co)[1]
            yh = vh.conv2d_fwd(col, vh.pack_conv_weight(wg, planned=False), None, b, co, 1, 1, 1, 0, False)
            y = vh.nhwc_to_nchw(yh)
        ctx.save_for_backward(xh, oh, mh, col, weight)
        ctx.geom = (stride, dg, offset.shape[1], bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        xh, oh, mh, col, weight = ctx.saved_tensors
        stride, dg, off_ch, has_bias = ctx.geom
        co = weight.shape[0]
        with torch.no_grad():
            dzh = vh.nchw_to_nhwc(dy.detach().float().contiguous(), _pad32(co))
            wg = vh.deform_gemm_weight(weight.detach().float())
            dxh, d_off, d_mask, dw = columns_backward(dzh, col, wg, xh, oh, mh, weight, stride, dg, deterministic=is_deterministic())
            dx = vh.nhwc_to_nchw(dxh)
            doff = vh.nhwc_to_nchw(d_off)[:, :off_ch]
            dmask = None if d_mask is None else vh.nhwc_to_nchw(d_mask)
            db = vh.col_sum(dzh)[:co].contiguous() if has_bias else None
        return dx, doff, dmask, dw, db, None, None


def deform_conv(input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, im2col_step=64):
    """DCN v1 (reference: DeformConvFunction.apply; ``im2col_step`` is accepted and has no meaning here)."""
    s = check_geometry(weight, stride, padding, dilation, groups)
    return _DeformConvFunction.apply(input, offset, None, weight, None, s, deformable_groups)


def modulated_deform_conv(input, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1):
    """DCN v2 (reference: ModulatedDeformConvFunction.apply); ``mask`` holds the modulation itself (already through its sigmoid)."""
    s = check_geometry(weight, stride, padding, dilation, groups)
    return _DeformConvFunction.apply(input, offset, mask, weight, bias, s, deformable_groups)


def _uniform_init(weight, in_channels, kernel_size):
    n = in_channels
    for k in kernel_size:
        n *= k
    stdv = 1. / math.sqrt(n)
    weight.data.uniform_(-stdv, stdv)


class DeformConv(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, bias=False):
        super().__init__()
        assert not bias
        assert in_channels % groups == 0, f"in_channels {in_channels} cannot be divisible by groups {groups}"
        assert out_channels % groups == 0, f"out_channels {out_channels} cannot be divisible by groups {groups}"
        assert groups == 1, "grouped deformable convolutions are not implemented"
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride = _pair(stride)
        self.padding = _pair(padding)
        self.dilation = _pair(dilation)
        self.groups = groups
        self.deformable_groups = deformable_groups
        self.weight = nn.Parameter(torch.Tensor(out_channels, in_channels // self.groups, *self.kernel_size))
        self.reset_parameters()

    def reset_parameters(self):
        _uniform_init(self.weight, self.in_channels, self.kernel_size)

    def forward(self, x, offset):
        return deform_conv(x, offset, self.weight, self.stride, self.padding, self.dilation, self.groups, self.deformable_groups)


class DeformConvPack(DeformConv):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.conv_offset = nn.Conv2d(self.in_channels, self.deformable_groups * 2 * self.kernel_size[0] * self.kernel_size[1],
                                     kernel_size=self.kernel_size, stride=_pair(self.stride), padding=_pair(self.padding), bias=True)
        self.init_offset()

    def init_offset(self):
        self.conv_offset.weight.data.zero_()
        self.conv_offset.bias.data.zero_()

    def forward(self, x):
        offset = self.conv_offset(x)
        return deform_conv(x, offset, self.weight, self.stride, self.padding, self.dilation, self.groups, self.deformable_groups)


class ModulatedDeformConv(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, bias=True):
        super().__init__()
        assert groups == 1, "grouped deformable convolutions are not implemented"
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride = stride
        self.padding = padding
        self.dilation = dilation
        self.groups = groups
        self.deformable_groups = deformable_groups
        self.with_bias = bias
        self.weight = nn.Parameter(torch.Tensor(out_channels, in_channels // groups, *self.kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        _uniform_init(self.weight, self.in_channels, self.kernel_size)
        if self.bias is not None:
            self.bias.data.zero_()

    def forward(self, x, offset, mask):
        return modulated_deform_conv(x, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups,
                                     self.deformable_groups)


class ModulatedDeformConvPack(ModulatedDeformConv):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.conv_offset_mask = nn.Conv2d(self.in_channels, self.deformable_groups * 3 * self.kernel_size[0] * self.kernel_size[1],
                                          kernel_size=self.kernel_size, stride=_pair(self.stride), padding=_pair(self.padding), bias=True)
        self.init_offset()

    def init_offset(self):
        self.conv_offset_mask.weight.data.zero_()
        self.conv_offset_mask.bias.data.zero_()

    def forward(self, x):
        out = self.conv_offset_mask(x)
        o1, o2, mask = torch.chunk(out, 3, dim=1)
        offset = torch.cat((o1, o2), dim=1)
        mask = torch.sigmoid(mask)
        return modulated_deform_conv(x, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups,
                                     self.deformable_groups)
