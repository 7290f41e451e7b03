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

_NAMES = {"PoseHighResolutionNet": "HRNet"}


def _check_model(m):
    """The networks this reference serves; everything else is refused by name, before anything touches the device."""
    from .simplepose import SimplePose
    if not isinstance(m, SimplePose):
        cls = type(m).__name__
        name = _NAMES.get(cls, cls)
        raise NotImplementedError(f"the float64 reference step serves SimplePose only, not {name}" + (f" ({cls})" if name != cls else ""))
    for blk in (b for stage in m.preact.stages() for b in stage):
        if getattr(blk, "with_dcn", False):
            raise NotImplementedError("the float64 reference step does not serve deformable bottlenecks (DCN)")
        if not hasattr(blk, "conv3"):
            raise NotImplementedError("the float64 reference step serves the bottleneck ResNets (50 / 101 / 152) only, not BasicBlock ResNets (18 / 34)")


def _d64(t):
    return t.detach().double().contiguous()


class _BN:
    """BatchNorm2d(train) in float64 on the stored z; the statistics stay here, the module is only read."""

    def __init__(self, bn: nn.BatchNorm2d, stats: dict):
        if not isinstance(bn, nn.BatchNorm2d) or bn.weight is None or not bn.track_running_stats or bn.momentum is None:
            raise NotImplementedError(f"no float64 training path for {bn}")
        self.bn, self.stats = bn, stats

    def forward(self, z, skip, relu):
        bn = self.bn
        self.gamma = _d64(bn.weight)
        st = vh.bn_train_fwd_stats_f64(z, self.gamma, _d64(bn.bias), _d64(bn.running_mean), _d64(bn.running_var), bn.momentum, bn.eps)
        self.mean, self.invstd = st[0], st[2]
        self.stats[bn] = {"mean": st[0], "var": st[1], "running_mean": st[5], "running_var": st[6]}
        return vh.bn_apply_f64(z, st[3], st[4], skip, relu)

    def backward(self, dy, y, z, grads, want_g):
        dz, g, dgamma, dbeta = vh.bn_train_bwd_f64(dy, y, z, self.gamma, self.mean, self.invstd, want_g=want_g)
        grads[self.bn.weight] = dgamma
        grads[self.bn.bias] = dbeta
        self.gamma = self.mean = self.invstd = None
        return dz, g


class _ConvBN:
    """Conv2d (bias-free) + BatchNorm2d(train) (+ residual) (+ ReLU)."""

    def __init__(self, conv: nn.Conv2d, bn: nn.BatchNorm2d, relu: bool, stats: dict, need_dx: bool = True):
        if conv.bias is not None or conv.groups != 1 or conv.dilation != (1, 1) or conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1]:
            raise NotImplementedError(f"no float64 training path for {conv}")
        self.conv, self.bn, self.relu, self.need_dx = conv, _BN(bn, stats), relu, need_dx
        self.cout, self.cin, self.r, self.s = conv.weight.shape
        self.stride, self.pad = conv.stride[0], conv.padding[0]

    def forward(self, x, skip=None):
        w = self.conv.weight.detach().float()
        z = vh.conv2d_fwd_f64(x, vh.pack_conv_weight_f64(w), None, None, self.stride, self.pad, False)
        y = self.bn.forward(z, skip, self.relu)
        wd = vh.pack_conv_weight_dgrad_f64(w, self.stride, self.pad) if self.need_dx else None
        self.saved = (x, z, y if self.relu else None, skip is not None, wd)
        return y

    def backward(self, dy, grads, dx_residual=None):
        """dy: gradient of the layer output -> (dx, gradient of the skip input or None); parameter gradients go to ``grads``."""
        x, z, y, had_skip, wd = self.saved
        self.saved = None
        dz, g = self.bn.backward(dy, y, z, grads, want_g=had_skip and y is not None)
        if had_skip and y is None:
            g = dy
        grads[self.conv.weight] = vh.conv2d_wgrad_f64(x, dz, self.cout, self.cin, self.r, self.s, self.stride, self.pad)
        dx = vh.conv2d_dgrad_f64(dz, wd, x.shape, self.r, self.s, self.stride, self.pad, residual=dx_residual) if self.need_dx else None
        return dx, g


class _DeconvBN:
    """ConvTranspose2d(4,2,1, bias-free) + BatchNorm2d(train) + ReLU."""

    def __init__(self, dc: nn.ConvTranspose2d, bn: nn.BatchNorm2d, stats: dict):
        if dc.kernel_size != (4, 4) or dc.stride != (2, 2) or dc.padding != (1, 1) or dc.output_padding != (0, 0) or dc.groups != 1 or dc.bias is not None:
            raise NotImplementedError(f"no float64 training path for {dc}")
        self.dc, self.bn = dc, _BN(bn, stats)
        self.cin, self.cout = dc.weight.shape[:2]

    def forward(self, x):
        w = self.dc.weight.detach().float()
        z = vh.deconv4x4s2_fwd_f64(x, vh.pack_deconv_weight_f64(w), None, None, False)
        y = self.bn.forward(z, None, True)
        # the data gradient is a plain 4x4 / stride 2 / pad 1 conv of dz whose "OIHW" weight is the (Cin,Cout,4,4) parameter itself
        self.saved = (x, z, y, vh.pack_conv_weight_f64(w))
        return y

    def backward(self, dy, grads):
        x, z, y, wd = self.saved
        self.saved = None
        dz, _ = self.bn.backward(dy, y, z, grads, want_g=False)
        grads[self.dc.weight] = vh.conv2d_wgrad_f64(x, dz, self.cout, self.cin, 4, 4, 2, 1, transposed=True)
        return vh.conv2d_fwd_f64(dz, wd, None, None, 2, 1, False)


class _BottleneckT:
    def __init__(self, blk, stats: dict):
        self.c1 = _ConvBN(blk.conv1, blk.bn1, True, stats)
        self.c2 = _ConvBN(blk.conv2, blk.bn2, True, stats)
        self.c3 = _ConvBN(blk.conv3, blk.bn3, True, stats)
        self.proj = _ConvBN(blk.downsample[0], blk.downsample[1], False, stats) if blk.downsample is not None else None

    def forward(self, x):
        skip = x if self.proj is None else self.proj.forward(x)
        return self.c3.forward(self.c2.forward(self.c1.forward(x)), skip=skip)

    def backward(self, dy, grads):
        db, g = self.c3.backward(dy, grads)                # g = dy*[y > 0]: the gradient of the skip input
        da, _ = self.c2.backward(db, grads)
        dskip = g if self.proj is None else self.proj.backward(g, grads)[0]
        return self.c1.backward(da, grads, dx_residual=dskip)[0]    # dx = dgrad(c1) + dskip in one write-out


class _HeadT:
    """Conv2d(1x1) with bias and no BatchNorm, heat-maps out as float64 NCHW."""

    def __init__(self, conv: nn.Conv2d):
        if conv.kernel_size != (1, 1) or conv.stride != (1, 1) or conv.padding != (0, 0) or conv.bias is None:
            raise NotImplementedError(f"no float64 training path for the head {conv}")
        self.conv = conv
        self.cout, self.cin = conv.weight.shape[:2]

    def forward(self, x):
        w = self.conv.weight.detach().float()
        self.saved = (x, vh.pack_conv_weight_dgrad_f64(w, 1, 0))
        return vh.conv2d_fwd_f64(x, vh.pack_conv_weight_f64(w), None, _d64(self.conv.bias), 1, 0, False, out_nchw=True)

    def backward(self, dout_nchw, grads):
        x, wd = self.saved
        self.saved = None
        if tuple(dout_nchw.shape) != (x.shape[0], self.cout, x.shape[1], x.shape[2]):
            raise vh.VatlError(f"backward: the cotangent has shape {tuple(dout_nchw.shape)}, the heat-maps {(x.shape[0], self.cout, x.shape[1], x.shape[2])}")
        dy = vh.nchw_to_nhwc_f64(dout_nchw.contiguous())
        grads[self.conv.bias] = vh.col_sum_f64(dy)
        grads[self.conv.weight] = vh.conv2d_wgrad_f64(x, dy, self.cout, self.cin, 1, 1, 1, 0)
        return vh.conv2d_dgrad_f64(dy, wd, x.shape, 1, 1, 1, 0)


class SimplePoseTrainerF64:
    """Tape-based float64 forward / backward of SimplePose in training mode.  Reads the model, never writes it."""

    def __init__(self, m):
        _check_model(m)
        self.m = m
        self.stats = {}
        t = m.preact
        self.stem = _ConvBN(t.conv1, t.bn1, True, self.stats, need_dx=False)   # the input gradient is never read
        self.blocks = [_BottleneckT(b, self.stats) for stage in t.stages() for b in stage]
        d = m.deconv_layers
        self.deconvs = [_DeconvBN(d[0], d[1], self.stats), _DeconvBN(d[3], d[4], self.stats), _DeconvBN(d[6], d[7], self.stats)]
        self.head = _HeadT(m.final_layer)

    def _input(self, x_nchw):
        if not isinstance(x_nchw, torch.Tensor) or x_nchw.dim() != 4:
            raise vh.VatlError("the float64 reference step expects an (N,C,H,W) tensor")
        if not x_nchw.is_cuda:
            raise vh.VatlError("the float64 reference step runs on MI355X only (there is deliberately no CPU fallback)")
        if x_nchw.dtype not in (torch.float32, torch.float64):
            raise vh.VatlError(f"the float64 reference step expects fp32 or float64 crops, got {x_nchw.dtype}")
        for t in list(self.m.parameters()) + list(self.m.buffers()):
            if t.device != x_nchw.device:
                raise vh.VatlError(f"model on {t.device}, input on {x_nchw.device}")
        return vh.nchw_to_nhwc_f64(x_nchw.detach().contiguous())

    def trunk_forward(self, x_nchw, blocks=None):
        """Stem, max-pool and the first ``blocks`` bottlenecks (None: all) -> the last block's output, float64 NHWC."""
        with torch.no_grad():
            self.stats.clear()
            x = self._input(x_nchw)
            self.stem_y = self.stem.forward(x)
            x = vh.maxpool3x3s2_fwd_f64(self.stem_y)
            self.ran = self.blocks[:blocks]
            for b in self.ran:
                x = b.forward(x)
            return x

    def trunk_backward(self, dx, grads):
        """Backward of ``trunk_forward`` from the gradient of its result (float64 NHWC); parameter gradients go to ``grads``."""
        with torch.no_grad():
            ran, self.ran = self.ran, None
            for b in reversed(ran):
                dx = b.backward(dx, grads)
            stem_y, self.stem_y = self.stem_y, None
            self.stem.backward(vh.maxpool3x3s2_bwd_f64(dx, stem_y), grads)

    def forward(self, x_nchw):
        """x (B,3,H,W) fp32 or float64 NCHW -> heat-maps (B,J,H/4,W/4) float64 NCHW."""
        with torch.no_grad():
            x = self.trunk_forward(x_nchw)
            for d in self.deconvs:
                x = d.forward(x)
            return self.head.forward(x)

    def backward(self, dout_nchw):
        """dout (B,J,H,W) float64 NCHW -> {parameter: float64 gradient in the parameter's own shape} for every parameter of the model."""
        if not dout_nchw.is_cuda:
            raise vh.VatlError("the float64 reference step runs on MI355X only (there is deliberately no CPU fallback)")
        if dout_nchw.dtype != torch.float64:
            raise vh.VatlError(f"backward: the cotangent must be float64, got {dout_nchw.dtype}")
        grads = {}
        with torch.no_grad():
            dx = self.head.backward(dout_nchw.detach(), grads)
            for d in reversed(self.deconvs):
                dx = d.backward(dx, grads)
            self.trunk_backward(dx, grads)
        return grads

    def batch_statistics(self):
        """Per BatchNorm module of the last forward: {"mean", "var" (biased), "running_mean", "running_var"} in float64 — the batch
        statistics and the running statistics a training step WOULD write (momentum, unbiased variance); the module keeps its own."""
        return {bn: dict(s) for bn, s in self.stats.items()}


def trainer_for_f64(m: nn.Module) -> SimplePoseTrainerF64:
    """A float64 tape trainer of a SimplePose network (a new one per call: nothing is cached on the module); any other network is
    refused by name."""
    return SimplePoseTrainerF64(m)
