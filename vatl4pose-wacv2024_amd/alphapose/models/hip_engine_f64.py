"""Float64 REFERENCE forward of the pose networks on the device.

Every parity statement about the fp32 routes rests on a float64 run of the network; this module runs it on the card instead of with
torch on the host: the plans of ``hip_engine_walk`` walk the same ``nn.Module`` trees as ``hip_engine`` does, but every conv — the 3-channel stems, the
17-joint heads and the SE gates' Linear layers included — goes to ONE generic implicit GEMM on the fp64 matrix pipe
(csrc/conv_f64.hip: one fixed K order, no split-K, no atomics), transposed convs to the same kernel as four 2x2 phases, and the glue
between them to small float64 kernels (csrc/glue_f64.hip).  No Winograd, no chains, no fused stem, no torch convolution / linear /
matmul anywhere.  Results are bit-reproducible and do not depend on how a crop is batched.

It stands BESIDE the product path: nothing here is called by ``model(x)``, ``forward_into``, the trainers or ``bench.py``, nothing
feeds the FLOP meter, and there is no knob.  Inference only (eval-mode BatchNorm folded in float64: scale = gamma / sqrt(var + eps),
bias = beta - mean * scale (+ conv_bias * scale), computed from the fp32 parameters converted to float64).

Nothing is cached across calls: the float64 filters are packed at the start of every call from the parameters' current values and
dropped at its end, so there is no stale-plan question to answer (``hip_engine.invalidate`` has nothing to drop here).
"""
from __future__ import annotations

import torch
import torch.nn as nn

import vatl_hip as vh

from . import hip_engine_walk as walk

# The batch is cut by BYTES: float64 NHWC activations are twice the fp32 ones (the stride-2 stem output, the largest tensor of all three
# networks, is 6.3 MB per crop at 256x192) and a handful of them are alive at a time.  One chunk's largest tensor stays below this.
CHUNK_BYTES = 1 << 30


class _Ops:
    """What the float64 reference puts into the shared walker: float64 NHWC activations of any channel count, filters and the BatchNorm
    fold in float64 (a bias without BatchNorm gets a scale of ones), the SE gate a (B, C) float64 matrix all the way."""
    route, plan = "float64 reference", "float64 plan"
    in_dtypes, in_words = (torch.float32, torch.float64), "fp32 or float64 crops"
    esize, fold_dtype, unit_scale = 8, torch.float64, True

    def chunk_bytes(self):
        return CHUNK_BYTES

    def in_channels(self, c):
        return c

    def pack_conv(self, w):
        return vh.pack_conv_weight_f64(w)

    def pack_deconv(self, w):
        return vh.pack_deconv_weight_f64(w)

    def conv(self, x, w, scale, bias, stride, pad, relu, residual=None, final=False, out=None):
        return vh.conv2d_fwd_f64(x, w, scale, bias, stride, pad, relu, residual=residual, out_nchw=final, out=out)

    def deconv(self, x, w, scale, bias, relu):
        return vh.deconv4x4s2_fwd_f64(x, w, scale, bias, relu)

    def se_gate(self, pooled, fc0, fc1):
        b, c = pooled.shape
        hidden = fc0(pooled.reshape(b, 1, 1, c), relu=True)
        return fc1(hidden, relu=False).reshape(b, -1)

    def to_nhwc(self, x):
        return vh.nchw_to_nhwc_f64(x)

    def to_nchw(self, x):
        return vh.nhwc_to_nchw_f64(x)

    def maxpool(self, x):
        return vh.maxpool3x3s2_fwd_f64(x)

    def gap(self, x):
        return vh.gap_fwd_f64(x)

    def pixelshuffle(self, x):
        return vh.pixelshuffle2_fwd_f64(x)

    def se_scale_add_relu(self, x, gate, residual):
        return vh.se_scale_add_relu_f64(x, gate, residual)

    def fuse_upsample_add(self, base, ups, relu):
        return vh.fuse_upsample_add_f64(base, ups, relu=relu)


_OPS = _Ops()


def _net_plan(m):
    return walk._net_plan(_OPS, m)


def forward_f64(m: nn.Module, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Heat-maps (N, J, H/4, W/4) of SimplePose / FastPose / PoseHighResolutionNet in float64 on the device.  ``x``: fp32 (converted exactly)
    or float64 NCHW crops on the model's device; ``out``: a contiguous float64 device tensor to write into, or None."""
    return walk.forward(_OPS, m, x, out, None, "forward_f64")


def embedding_f64(m: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """trunk -> global average pool -> (N, 2048) float64 of SimplePose / FastPose (simplepose.py:88-91, fastpose.py:70-73)."""
    return walk.embedding(_OPS, m, x, "embedding_f64")


def features_f64(module: nn.Module, x):
    """A bare sub-module in float64, NCHW in and out: a ``ResNet`` / ``SEResnet`` trunk, one ``Bottleneck`` / ``BasicBlock`` (with or
    without SE gate and projection), a ``DUC``, or a ``HighResolutionModule`` (``x`` = one tensor per branch; returns a list)."""
    return walk.features(_OPS, module, x, "features_f64")
