"""Float64 REFERENCE of the SimplePose training-mode forward and backward on the device: per-tensor gradients in float64.

``hip_engine_f64`` is the yardstick of the inference routes; this module is the same for the fine-tune step.  It walks the graph the
two trainers walk (``hip_train``: fp32, ``hip_train_h16``: bf16) as a small tape, with every tensor float64 NHWC and every sum in one
fixed order:

  forward   z = conv(x) (csrc/conv_f64.hip, no write-out affine) ; batch statistics of z -> (scale, bias) and the running statistics a
            step WOULD write (csrc/train_glue_f64.hip) ; y = relu(z*scale + bias (+ skip))
  backward  g = dy*[y > 0] from the stored y ; (dgamma, dbeta) ; dz = gamma*invstd*(g - dbeta/M - xhat*dgamma/M) ;
            dW = wgrad(x, dz) (csrc/wgrad_f64.hip: fixed-chunk split over pixels, slabs added in split order) ;
            dx = conv(dz, re-packed filter) on the forward kernel — a stride-2 conv as one launch per input-pixel phase, the skip
            gradient added in the write-out.

It stands BESIDE the product path: nothing here is called by ``model(x)``, the trainers, ``ActiveLearning`` or ``bench.py``; nothing
feeds the FLOP meter; there is no knob, no plan cache and no torch convolution / linear / matmul.  The MODEL IS NOT TOUCHED: running
statistics and ``num_batches_tracked`` are not written (``batch_statistics()`` returns what a step would write), ``.grad`` is not
written (``backward`` returns a dict), nothing is stored on the module.  Float64 filters are packed from the parameters' current
values at every ``forward`` and dropped by ``backward``.  There is deliberately no autograd bridge: a reference that fills fp32
``.grad`` would round away what it is for.  The loss is the caller's business: the cotangent comes in, as with the other trainers.

SimplePose on the bottleneck ResNets only: FastPose, HRNet, deformable bottlenecks and BasicBlock ResNets are refused by name.
"""
from __future__ import annotations

import torch
import torch.nn as nn

import vatl_hip as vh

from . import hip_train_tape as tape

_NAMES = {"PoseHighResolutionNet": "HRNet"}
_NO_CPU = "the float64 reference step runs on MI355X only (there is deliberately no CPU fallback)"


def _not_simplepose(cls):
    name = _NAMES.get(cls, cls)
    return f"the float64 reference step serves SimplePose only, not {name}" + (f" ({cls})" if name != cls else "")


def _d64(t):
    return t.detach().double().contiguous()


def _w32(mod):
    return mod.weight.detach().float()


class _Ops:
    """What the float64 step decides on the shared tape: float64 library calls on the calling stream, filters packed from the parameters'
    current values inside each forward (the data-gradient layout rides in the layer's saved tensors and is dropped by its backward),
    BatchNorm from float64 copies into the trainer's ``stats`` (the module is only read), gradients as fresh tensors in a plain dict."""

    NAME, HEAD_NEEDS_BIAS = "float64", True
    REFUSALS = (_not_simplepose, "the float64 reference step does not serve deformable bottlenecks (DCN)",
                "the float64 reference step serves the bottleneck ResNets (50 / 101 / 152) only, not BasicBlock ResNets (18 / 34)")

    def __init__(self, m, stats: dict):
        self.m, self.stats = m, stats

    def check_bn(self, bn):
        if not isinstance(bn, nn.BatchNorm2d) or bn.weight is None or not bn.track_running_stats or bn.momentum is None:
            raise NotImplementedError(f"no float64 training path for {bn}")

    def conv_filters(self, layer):
        return None, None

    deconv_filters = head_filters = conv_filters

    def input(self, x_nchw):
        self.stats.clear()
        if not isinstance(x_nchw, torch.Tensor) or x_nchw.dim() != 4:
            raise vh.VatlError("the float64 reference step expects an (N,C,H,W) tensor")
        if not x_nchw.is_cuda:
            raise vh.VatlError(_NO_CPU)
        if x_nchw.dtype not in (torch.float32, torch.float64):
            raise vh.VatlError(f"the float64 reference step expects fp32 or float64 crops, got {x_nchw.dtype}")
        for t in list(self.m.parameters()) + list(self.m.buffers()):
            if t.device != x_nchw.device:
                raise vh.VatlError(f"model on {t.device}, input on {x_nchw.device}")
        return vh.nchw_to_nhwc_f64(x_nchw.detach().contiguous())

    def conv(self, l, x):
        return vh.conv2d_fwd_f64(x, vh.pack_conv_weight_f64(_w32(l.conv)), None, None, l.stride, l.pad, False)

    def conv_wd(self, l):
        return vh.pack_conv_weight_dgrad_f64(_w32(l.conv), l.stride, l.pad) if l.need_dx else None

    def deconv(self, l, x):
        return vh.deconv4x4s2_fwd_f64(x, vh.pack_deconv_weight_f64(_w32(l.dc)), None, None, False)

    def deconv_wd(self, l):
        return vh.pack_conv_weight_f64(_w32(l.dc))

    def head(self, l, x):
        w = _w32(l.conv)
        wd = vh.pack_conv_weight_dgrad_f64(w, 1, 0)
        return vh.conv2d_fwd_f64(x, vh.pack_conv_weight_f64(w), None, _d64(l.conv.bias), 1, 0, False, out_nchw=True), wd

    def bn_fwd(self, bn, z, skip, relu):
        gamma = _d64(bn.weight)
        st = vh.bn_train_fwd_stats_f64(z, gamma, _d64(bn.bias), _d64(bn.running_mean), _d64(bn.running_var), bn.momentum, bn.eps)
        self.stats[bn] = {"mean": st[0], "var": st[1], "running_mean": st[5], "running_var": st[6]}
        return vh.bn_apply_f64(z, st[3], st[4], skip, relu), (gamma, st[0], st[2])

    def bn_bwd(self, bn, st, dy, y, z, grads, want_g):
        dz, g, grads[bn.weight], grads[bn.bias] = vh.bn_train_bwd_f64(dy, y, z, *st, want_g=want_g)
        return dz, g

    def wgrad(self, p, grads, x, dz, cout, cin, r, s, stride, pad, transposed=False, side=True):
        return vh.conv2d_wgrad_f64(x, dz, cout, cin, r, s, stride, pad, transposed=transposed)

    def dgrad(self, l, wd, dz, xshape, residual=None):
        return vh.conv2d_dgrad_f64(dz, wd, xshape, l.r, l.s, l.stride, l.pad, residual=residual)

    def deconv_dgrad(self, l, wd, dz):
        return vh.conv2d_fwd_f64(dz, wd, None, None, 2, 1, False)

    def head_cotangent(self, l, x, dout_nchw, grads):
        if tuple(dout_nchw.shape) != (x.shape[0], l.cout, x.shape[1], x.shape[2]):
            raise vh.VatlError(f"backward: the cotangent has shape {tuple(dout_nchw.shape)}, the heat-maps {(x.shape[0], l.cout, x.shape[1], x.shape[2])}")
        dy = vh.nchw_to_nhwc_f64(dout_nchw.contiguous())
        grads[l.conv.bias] = vh.col_sum_f64(dy)
        return dy

    def maxpool_fwd(self, x):
        return vh.maxpool3x3s2_fwd_f64(x)

    def maxpool_bwd(self, dpool, x):
        return vh.maxpool3x3s2_bwd_f64(dpool, x)

    def flush(self, grads=None):
        pass

    join = flush


class SimplePoseTrainerF64(tape.SimplePoseTape):
    """Tape-based float64 forward / backward of SimplePose in training mode.  Reads the model, never writes it."""

    def __init__(self, m):
        self.m, self.stats = m, {}
        super().__init__(_Ops(m, self.stats), m)

    # the tape's passes, recorded by no autograd graph
    trunk_forward = torch.no_grad()(tape.SimplePoseTape.trunk_forward)
    trunk_backward = torch.no_grad()(tape.SimplePoseTape.trunk_backward)
    forward = torch.no_grad()(tape.SimplePoseTape.forward)

    def backward(self, dout_nchw):
        """dout (B,J,H,W) float64 NCHW -> {parameter: float64 gradient in the parameter's own shape} for every parameter of the model."""
        if not dout_nchw.is_cuda:
            raise vh.VatlError(_NO_CPU)
        if dout_nchw.dtype != torch.float64:
            raise vh.VatlError(f"backward: the cotangent must be float64, got {dout_nchw.dtype}")
        with torch.no_grad():
            return super().backward(dout_nchw.detach(), {})

    def batch_statistics(self):
        """Per BatchNorm module of the last forward: {"mean", "var" (biased), "running_mean", "running_var"} in float64 — the batch
        statistics and the running statistics a training step WOULD write (momentum, unbiased variance); the module keeps its own."""
        return {bn: dict(s) for bn, s in self.stats.items()}


def trainer_for_f64(m: nn.Module) -> SimplePoseTrainerF64:
    """A float64 tape trainer of a SimplePose network (a new one per call: nothing is cached on the module); any other network is
    refused by name."""
    return SimplePoseTrainerF64(m)

