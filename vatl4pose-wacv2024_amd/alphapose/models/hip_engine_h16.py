"""Opt-in 16-bit (float16 / bfloat16) inference forward of the pose networks on the device.

The fp32 routes of ``hip_engine`` multiply on the fp32 matrix pipe; this module trades bits for the 16-bit pipe where a caller can
afford it — the evaluation pass of an active-learning round ranks frames and does not need fp32 heat-maps to do so
(``cfg.VAL.PRECISION``).  The plans of ``hip_engine_walk`` walk the same ``nn.Module`` trees as for ``hip_engine_f64``: every conv — the 3-channel stems
(padded to 8 channels by the input converter), the 17-joint heads and the SE gates' Linear layers included — goes to ONE generic
implicit GEMM on ``v_mfma_f32_16x16x32_{f16,bf16}`` (csrc/conv_h16.hip: operands and stored activations 16-bit, products accumulated
in fp32, the folded-BatchNorm write-out computed in fp32 and rounded once; one fixed K order, no split-K, no atomics), transposed convs
to the same kernel as four 2x2 phases, and the glue between them to small kernels (csrc/glue_h16.hip).  No Winograd, no chains, no
torch convolution / linear / matmul anywhere.  Heat-maps, embeddings and SE gates leave the kernels as fp32.  Results are
bit-reproducible and do not depend on how a crop is batched, so sharded evaluation equals single-process evaluation.

It stands BESIDE the product path: nothing here is called by ``model(x)``, ``forward_into``, the trainers or ``bench.py``, nothing
feeds the FLOP meter, and there is no knob.  Inference only (eval-mode BatchNorm folded in fp32 on the device: scale = gamma /
sqrt(var + eps), bias = beta - mean * scale (+ conv_bias * scale)).

Nothing is cached across calls: the 16-bit filters are packed at the start of every call from the parameters' current fp32 values and
dropped at its end, so a fine-tune step between two evaluations can never leave a stale 16-bit copy (``hip_engine.invalidate`` has
nothing to drop here).
"""
from __future__ import annotations

import torch
import torch.nn as nn

import vatl_hip as vh

from . import hip_engine_walk as walk

# The batch is cut by BYTES, as in the float64 engine: one chunk's largest tensor (the stride-2 stem output, H/2 x W/2 x 64 values of
# 2 bytes) stays below this.  Results do not depend on the cut.
CHUNK_BYTES = 1 << 28

DTYPES = (torch.float16, torch.bfloat16)


class _Ops:
    """What the 16-bit route puts into the shared walker for one storage type ``dt``: 16-bit NHWC activations with channels in multiples
    of 8, filters in ``dt``, the BatchNorm fold in fp32 (a bias without BatchNorm has no scale), the pooled vector and the SE gate fp32."""
    route, plan = "16-bit route", "16-bit plan"
    in_dtypes, in_words = (torch.float32,), "fp32 crops (they are rounded to the 16-bit type on the device)"
    esize, fold_dtype, unit_scale = 2, torch.float32, False

    def __init__(self, dt):
        self.dt = dt

    def chunk_bytes(self):
        return CHUNK_BYTES

    def in_channels(self, c):
        return 8                                                                            # the input converter pads the 3 channels to 8

    def pack_conv(self, w):
        return vh.pack_conv_weight_h16(w, self.dt)

    def pack_deconv(self, w):
        return vh.pack_deconv_weight_h16(w, self.dt)

    def conv(self, x, w, scale, bias, stride, pad, relu, residual=None, final=False, out=None):
        return vh.conv2d_fwd_h16(x, w, scale, bias, stride, pad, relu, residual=residual, out_f32_nchw=final, out=out)

    def deconv(self, x, w, scale, bias, relu):
        return vh.deconv4x4s2_fwd_h16(x, w, scale, bias, relu)

    def se_gate(self, pooled, fc0, fc1):
        """fp32 (B, C) -> 16-bit (B,1,1,C), the hidden layer 16-bit, the gate out as fp32 (B, C)."""
        hidden = fc0(vh.nchw_to_nhwc_h16(pooled.reshape(*pooled.shape, 1, 1), self.dt), relu=True)
        gate = fc1(hidden, relu=False, final=True)
        return gate.reshape(gate.shape[0], -1)

    def to_nhwc(self, x):
        return vh.nchw_to_nhwc_h16(x, self.dt)

    def to_nchw(self, x):
        return vh.nhwc_to_nchw_h16(x)

    def maxpool(self, x):
        return vh.maxpool3x3s2_fwd_h16(x)

    def gap(self, x, out=None):
        return vh.gap_fwd_h16(x, out=out)

    def pixelshuffle(self, x):
        return vh.pixelshuffle2_fwd_h16(x)

    def se_scale_add_relu(self, x, gate, residual):
        return vh.se_scale_add_relu_h16(x, gate, residual)

    def fuse_upsample_add(self, base, ups, relu):
        return vh.fuse_upsample_add_h16(base, ups, relu=relu)


def _check_dtype(dtype, who: str) -> None:
    if dtype not in DTYPES:
        raise vh.VatlError(f"{who}: dtype must be torch.float16 or torch.bfloat16, got {dtype}")


def _check_out(t, shape, device, who: str, what: str) -> None:
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or t.device != device or not t.is_contiguous():
        raise vh.VatlError(f"{who}: {what} must be a contiguous fp32 tensor of shape {tuple(shape)} on {device}")


def _net_plan(m, dt):
    return walk._net_plan(_Ops(dt), m)


def forward_h16(m: nn.Module, x: torch.Tensor, out: torch.Tensor | None = None, dtype=torch.float16) -> torch.Tensor:
    """fp32 heat-maps (N, J, H/4, W/4) of SimplePose / FastPose / PoseHighResolutionNet computed in ``dtype`` (float16 or bfloat16) on the
    device — the shape and dtype ``hip_engine.forward_into`` fills, so every scorer takes them unchanged.  ``x``: fp32 NCHW crops on the
    model's device; ``out``: a contiguous fp32 device tensor to write into (it is returned), or None."""
    if out is not None:
        if not (isinstance(out, torch.Tensor) and out.dim() == 4 and out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()
                and isinstance(x, torch.Tensor) and out.shape[0] == x.shape[0]):
            raise vh.VatlError("forward_h16: out must be a contiguous fp32 device tensor with one row per crop")
    _check_dtype(dtype, "forward_h16")
    return walk.forward(_Ops(dtype), m, x, out, None, "forward_h16")


def forward_with_embedding_h16(m: nn.Module, x: torch.Tensor, out: torch.Tensor, emb: torch.Tensor, dtype=torch.float16) -> None:
    """Heat-maps into ``out`` and the get_embedding vectors (N, 2048, fp32: the pixels are summed in fp32) into ``emb`` from ONE trunk pass.
    The heat-maps are bit-identical to forward_h16's: same launches, the pooled trunk output is simply kept."""
    if not (isinstance(x, torch.Tensor) and isinstance(out, torch.Tensor) and isinstance(emb, torch.Tensor)):
        raise vh.VatlError("forward_with_embedding_h16: x, out and emb must be tensors")
    if not x.is_cuda:
        raise vh.VatlError("forward_with_embedding_h16 runs on MI355X only (there is deliberately no CPU fallback)")
    if out.dim() != 4 or out.shape[0] != x.shape[0]:
        raise vh.VatlError("forward_with_embedding_h16: out must be (N,J,H/4,W/4)")
    _check_out(out, out.shape, x.device, "forward_with_embedding_h16", "out")
    if emb.dim() != 2 or emb.shape[0] != x.shape[0]:
        raise vh.VatlError("forward_with_embedding_h16: emb must be (N, channels of the trunk)")
    _check_out(emb, emb.shape, x.device, "forward_with_embedding_h16", "emb")
    _check_dtype(dtype, "forward_with_embedding_h16")
    walk.forward(_Ops(dtype), m, x, out, emb, "forward_with_embedding_h16")


def embedding_h16(m: nn.Module, x: torch.Tensor, dtype=torch.float16) -> torch.Tensor:
    """trunk -> global average pool -> (N, 2048) fp32 of SimplePose / FastPose (simplepose.py:88-91, fastpose.py:70-73), the trunk in ``dtype``."""
    _check_dtype(dtype, "embedding_h16")
    return walk.embedding(_Ops(dtype), m, x, "embedding_h16")


def features_h16(module: nn.Module, x, dtype=torch.float16):
    """A bare sub-module in ``dtype``, fp32 NCHW in and out (the input is rounded to ``dtype``, the output converted exactly): a ``ResNet``
    / ``SEResnet`` trunk, one ``Bottleneck`` / ``BasicBlock`` (with or without SE gate and projection), a ``DUC``, or a
    ``HighResolutionModule`` (``x`` = one tensor per branch; returns a list).  Input channels must be a multiple of 8 except for a trunk."""
    _check_dtype(dtype, "features_h16")
    return walk.features(_Ops(dtype), module, x, "features_h16")
