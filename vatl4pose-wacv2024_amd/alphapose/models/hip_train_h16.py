"""Opt-in bf16 training step of SimplePose on the 16-bit matrix pipe (``cfg.RETRAIN.PRECISION: bf16`` for the fine-tune,
``cfg.TRAIN.PRECISION: bf16`` / ``--precision bf16`` for ``alphapose.pretrain``).

The fp32 trainer of ``hip_train`` multiplies on the fp32 matrix pipe; this one stores the input, every conv / deconv output z, every
BatchNorm (+ residual) (+ ReLU) output y, the pooled stem output and every gradient with respect to them as bfloat16 (NHWC, channels
padded to 8) and multiplies on ``v_mfma_f32_16x16x32_bf16`` with fp32 accumulation:

  forward   z = conv(x) (csrc/conv_h16.hip, no write-out affine) ; batch statistics of the stored z -> (scale, bias) and the running
            statistics, fp32 (csrc/train_glue_h16.hip) ; y = relu(z*scale + bias (+ skip))
  backward  g = dy*[y > 0] from the stored y ; (dgamma, dbeta) fp32 ; dz = gamma*invstd*(g - dbeta/M - xhat*dgamma/M) ;
            dW = wgrad(x, dz) (csrc/wgrad_h16.hip: fp32, fixed-chunk split over pixels, partials added in split order) ;
            dx = conv(dz, re-packed filter) on the inference kernel — a stride-2 conv as one launch per input-pixel phase, the skip
            gradient added in the write-out.

Master weights stay the fp32 ``nn.Parameter``s: the bf16 filters (forward and data-gradient layouts) are re-packed whenever a parameter's
(storage, version) has changed, i.e. in every step that follows an ``optimizer.step()``: all of them by ONE launch at the start of the
forward pass (``vatl_hip.PackPlanH16``, csrc/pack_h16.hip; ``_USE_PACK_PLAN``), which is part of the step.
Gradients land as fp32 in each parameter's own layout, straight in the ``GradArena`` slices when one is given, so the optimiser, the
all-reduce buckets and ``retrain_model``'s DataParallel-chunk logic are the fp32 trainer's.  BatchNorm running statistics follow the fp32
trainer's semantics (momentum, unbiased variance, ``num_batches_tracked``).  Every reduction has one fixed order and there are no
atomics: a step is bit-reproducible run to run.  The weight gradients run on the fp32 trainer's side stream (same kernels, same
arguments, same bits); no BatchNorm fusion into conv write-outs, no Winograd.

bf16 only (fp16 would need loss scaling for the heat-map MSE gradients), SimplePose only: FastPose, HRNet and deformable bottlenecks
are refused by name and stay on the fp32 trainer.
"""
from __future__ import annotations

import threading

import torch
import torch.nn as nn

import vatl_hip as vh

from . import hip_train
from .hip_train import _Grads, _gout, _side

DT = torch.bfloat16


def _check_model(m):
    """The networks this trainer serves; everything else is refused by name."""
    from .simplepose import SimplePose
    if not isinstance(m, SimplePose):
        raise NotImplementedError(f"RETRAIN.PRECISION bf16 serves SimplePose only, not {type(m).__name__}: it trains in fp32")
    for blk in (b for stage in m.preact.stages() for b in stage):
        if getattr(blk, "with_dcn", False):
            raise NotImplementedError("RETRAIN.PRECISION bf16 does not serve deformable bottlenecks (DCN): they train in fp32")
        if not hasattr(blk, "conv3"):
            raise NotImplementedError("RETRAIN.PRECISION bf16 serves the bottleneck ResNets (50 / 101 / 152) only")


_USE_PACK_PLAN = True      # False: every re-pack its own launch (same bits; tests/test_gpu_pretrain_h16.py A/Bs it)
_tls = threading.local()   # per host thread: the plan of the trainer whose forward / backward pass is running


class _Packed:
    """A bf16 copy of an fp32 parameter in some packed layout, refreshed when the parameter's (storage, version) has changed: by the
    running trainer's one-launch re-pack (vatl_hip.PackPlanH16) where its plan keeps the copy, otherwise on the spot."""

    def __init__(self, p, pack, kind, stride=1, pad=0):
        self.p, self.pack, self.job, self.key, self.buf = p, pack, (kind, stride, pad), None, None

    def get(self):
        p = self.p
        plan = getattr(_tls, "plan", None) if p.is_contiguous() else None    # the one launch reads the parameter's own storage
        key = (p.data_ptr(), p._version)
        if plan is not None:
            kept = plan.lookup(self, p)
            if kept is not None:
                self.buf, self.key = kept, key
                return kept
        if key != self.key:
            self.buf = self.pack(p.detach())
            self.key = key
        if plan is not None:
            plan.record(self, p.detach(), self.buf, *self.job)
        return self.buf


def _planned(kind):
    """Trainer.forward / Trainer.backward under the trainer's PackPlanH16, as ``hip_train._planned`` runs the fp32 trainers: the forward
    pass starts with ONE launch that refreshes every bf16 filter the step reads (forward and data-gradient layouts).  A forward pass
    without a ready plan records them: it packs per tensor, the data-gradient layouts at its end, and seals the record."""
    def deco(fn):
        def inner(self, *a, **k):
            if not _USE_PACK_PLAN:
                return fn(self, *a, **k)
            plan = self.__dict__.get("_pack_plan")
            if plan is None:
                plan = self.__dict__["_pack_plan"] = vh.PackPlanH16(DT)
            prev = getattr(_tls, "plan", None)
            _tls.plan = plan
            try:
                if kind == "forward":
                    plan.begin()
                else:
                    plan.note_stream()
                out = fn(self, *a, **k)
                if kind == "forward" and not plan.ready:
                    for q in self.packed:
                        q.get()
                    plan.seal()
                return out
            finally:
                _tls.plan = prev
        inner.__name__, inner.__doc__ = fn.__name__, fn.__doc__
        return inner
    return deco


class _ConvBN:
    """Conv2d (bias-free) + BatchNorm2d(train) (+ residual) (+ ReLU)."""

    def __init__(self, conv: nn.Conv2d, bn: nn.BatchNorm2d, relu: bool, need_dx: bool = True):
        if conv.bias is not None or conv.groups != 1 or conv.dilation != (1, 1) or conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1]:
            raise NotImplementedError(f"no bf16 training path for {conv}")
        self.conv, self.bn, self.relu, self.need_dx = conv, bn, relu, need_dx
        self.cout, self.cin, self.r, self.s = conv.weight.shape
        self.stride, self.pad = conv.stride[0], conv.padding[0]
        self.w = _Packed(conv.weight, lambda w: vh.pack_conv_weight_h16(w, DT), vh.PACK_H16_CONV)
        self.wd = _Packed(conv.weight, lambda w: vh.pack_conv_weight_dgrad_h16(w, self.stride, self.pad, DT), vh.PACK_H16_DGRAD, self.stride, self.pad) if need_dx else None

    def forward(self, x, skip=None):
        bn = self.bn
        z = vh.conv2d_fwd_h16(x, self.w.get(), None, None, self.stride, self.pad, False)
        mean, invstd, scale, bias = vh.bn_train_fwd_stats_h16(z, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.momentum, bn.eps)
        hip_train._count_batch(bn)
        y = vh.bn_apply_h16(z, scale, bias, skip, self.relu)
        self.saved = (x, z, y if self.relu else None, mean, invstd, skip is not None)
        return y

    def backward(self, dy, grads, dx_residual=None):
        """dy: gradient of the layer output -> (dx, gradient of the skip input or None); parameter gradients go to ``grads``."""
        x, z, y, mean, invstd, had_skip = self.saved
        self.saved = None
        dz, g, dgamma, dbeta = vh.bn_train_bwd_h16(dy, y, z, self.bn.weight.detach(), mean, invstd, want_g=had_skip and y is not None,
                                                   dgamma=_gout(grads, self.bn.weight), dbeta=_gout(grads, self.bn.bias))
        if had_skip and y is None:
            g = dy
        grads[self.bn.weight] = dgamma
        grads[self.bn.bias] = dbeta
        ow = _gout(grads, self.conv.weight)
        if ow is None:                                     # no arena: the gradient tensor belongs to the calling stream, which reads it after the join
            ow = torch.empty(self.conv.weight.shape, device=x.device, dtype=torch.float32)
        # beside the critical chain (BatchNorm backward -> data gradient -> previous layer), as the fp32 trainer runs its weight gradients
        grads[self.conv.weight] = _side.run(lambda: vh.conv2d_wgrad_h16(x, dz, self.cout, self.cin, self.r, self.s, self.stride, self.pad, out=ow), x, dz)
        dx = vh.conv2d_dgrad_h16(dz, self.wd.get(), x.shape, self.r, self.s, self.stride, self.pad, residual=dx_residual) if self.need_dx else None
        return dx, g


class _DeconvBN:
    """ConvTranspose2d(4,2,1, bias-free) + BatchNorm2d(train) + ReLU."""

    def __init__(self, dc: nn.ConvTranspose2d, bn: nn.BatchNorm2d):
        if dc.kernel_size != (4, 4) or dc.stride != (2, 2) or dc.padding != (1, 1) or dc.output_padding != (0, 0) or dc.groups != 1 or dc.bias is not None:
            raise NotImplementedError(f"no bf16 training path for {dc}")
        self.dc, self.bn = dc, bn
        self.cin, self.cout = dc.weight.shape[:2]
        self.w = _Packed(dc.weight, lambda w: vh.pack_deconv_weight_h16(w, DT), vh.PACK_H16_DECONV)
        # the data gradient is a plain 4x4 / stride 2 / pad 1 conv of dz whose "OIHW" weight is the (Cin,Cout,4,4) parameter itself
        self.wd = _Packed(dc.weight, lambda w: vh.pack_conv_weight_h16(w, DT), vh.PACK_H16_CONV)

    def forward(self, x):
        bn = self.bn
        z = vh.deconv4x4s2_fwd_h16(x, self.w.get(), None, None, False)
        mean, invstd, scale, bias = vh.bn_train_fwd_stats_h16(z, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.momentum, bn.eps)
        hip_train._count_batch(bn)
        y = vh.bn_apply_h16(z, scale, bias, None, True)
        self.saved = (x, z, y, mean, invstd)
        return y

    def backward(self, dy, grads):
        x, z, y, mean, invstd = self.saved
        self.saved = None
        dz, _, dgamma, dbeta = vh.bn_train_bwd_h16(dy, y, z, self.bn.weight.detach(), mean, invstd, dgamma=_gout(grads, self.bn.weight),
                                                   dbeta=_gout(grads, self.bn.bias))
        grads[self.bn.weight] = dgamma
        grads[self.bn.bias] = dbeta
        ow = _gout(grads, self.dc.weight)
        if ow is None:
            ow = torch.empty(self.dc.weight.shape, device=x.device, dtype=torch.float32)
        grads[self.dc.weight] = _side.run(lambda: vh.conv2d_wgrad_h16(x, dz, self.cout, self.cin, 4, 4, 2, 1, transposed=True, out=ow), x, dz)
        return vh.conv2d_fwd_h16(dz, self.wd.get(), None, None, 2, 1, False)


class _BottleneckT:
    def __init__(self, blk):
        self.c1 = _ConvBN(blk.conv1, blk.bn1, True)
        self.c2 = _ConvBN(blk.conv2, blk.bn2, True)
        self.c3 = _ConvBN(blk.conv3, blk.bn3, True)
        self.proj = _ConvBN(blk.downsample[0], blk.downsample[1], False) if blk.downsample is not None else None

    def forward(self, x):
        skip = x if self.proj is None else self.proj.forward(x)
        return self.c3.forward(self.c2.forward(self.c1.forward(x)), skip=skip)

    def backward(self, dy, grads):
        db, g = self.c3.backward(dy, grads)                # g = dy*[y > 0]: the gradient of the skip input
        da, _ = self.c2.backward(db, grads)
        dskip = g if self.proj is None else self.proj.backward(g, grads)[0]
        return self.c1.backward(da, grads, dx_residual=dskip)[0]    # dx = dgrad(c1) + dskip in one write-out


class _HeadT:
    """Conv2d(1x1) with bias and no BatchNorm, heat-maps out as fp32 NCHW."""

    def __init__(self, conv: nn.Conv2d):
        if conv.kernel_size != (1, 1) or conv.stride != (1, 1) or conv.padding != (0, 0):
            raise NotImplementedError(f"no bf16 training path for the head {conv}")
        self.conv = conv
        self.cout, self.cin = conv.weight.shape[:2]
        self.w = _Packed(conv.weight, lambda w: vh.pack_conv_weight_h16(w, DT), vh.PACK_H16_CONV)
        self.wd = _Packed(conv.weight, lambda w: vh.pack_conv_weight_dgrad_h16(w, 1, 0, DT), vh.PACK_H16_DGRAD, 1, 0)

    def forward(self, x):
        self.x = x
        hip_train._flush_batch_counters()
        return vh.conv2d_fwd_h16(x, self.w.get(), None, self.conv.bias.detach(), 1, 0, False, out_f32_nchw=True)

    def backward(self, dout_nchw, grads):
        x, self.x = self.x, None
        dout_nchw = dout_nchw.contiguous()
        # the bias gradient stays on the fp32 reduction of dout
        grads[self.conv.bias] = vh.col_sum(vh.nchw_to_nhwc(dout_nchw, 32))[:self.cout].contiguous()
        dy = vh.nchw_to_nhwc_h16(dout_nchw, DT)                                   # 17 -> 24 channels (zeros), rounded to bf16
        grads[self.conv.weight] = vh.conv2d_wgrad_h16(x, dy, self.cout, self.cin, 1, 1, 1, 0, out=_gout(grads, self.conv.weight))
        return vh.conv2d_dgrad_h16(dy, self.wd.get(), x.shape, 1, 1, 1, 0)


class SimplePoseTrainerH16:
    """Tape-based forward/backward of SimplePose in training mode with bf16 storage; the interface of ``hip_train.SimplePoseTrainer``."""

    def __init__(self, m):
        _check_model(m)
        t = m.preact
        self.stem = _ConvBN(t.conv1, t.bn1, True, need_dx=False)   # the input gradient is never read
        self.blocks = [_BottleneckT(b) for stage in t.stages() for b in stage]
        d = m.deconv_layers
        self.deconvs = [_DeconvBN(d[0], d[1]), _DeconvBN(d[3], d[4]), _DeconvBN(d[6], d[7])]
        self.head = _HeadT(m.final_layer)
        convs = [self.stem] + [c for b in self.blocks for c in (b.c1, b.c2, b.c3, b.proj) if c is not None] + self.deconvs + [self.head]
        self.packed = [q for c in convs for q in (c.w, c.wd) if q is not None]    # every bf16 filter of a step: 57 + 56 for the R50

    def trunk_forward(self, x_nchw, blocks=None):
        """Stem, max-pool and the first ``blocks`` bottlenecks (None: all) -> the last block's output, bf16 NHWC.  ``forward`` runs the
        whole trunk through it; the tests also run a shallow prefix, where bf16 rounding is not yet amplified by the depth."""
        x = vh.nchw_to_nhwc_h16(x_nchw.contiguous(), DT)                          # 3 -> 8 channels (zeros)
        self.stem_y = self.stem.forward(x)
        x = vh.maxpool3x3s2_fwd_h16(self.stem_y)
        self.ran = self.blocks[:blocks]
        for b in self.ran:
            x = b.forward(x)
        return x

    def trunk_backward(self, dx, grads):
        """Backward of ``trunk_forward`` from the gradient of its result (bf16 NHWC); parameter gradients go to ``grads``."""
        ran, self.ran = self.ran, None
        for b in reversed(ran):
            dx = b.backward(dx, grads)
            if isinstance(grads, _Grads):
                grads.flush()
        stem_y, self.stem_y = self.stem_y, None
        self.stem.backward(vh.maxpool3x3s2_bwd_h16(dx, stem_y), grads)
        _side.join()

    @_planned("forward")
    def forward(self, x_nchw):
        """x (B,3,H,W) fp32 NCHW -> heat-maps (B,J,H/4,W/4) fp32 NCHW."""
        x = self.trunk_forward(x_nchw)
        for d in self.deconvs:
            x = d.forward(x)
        return self.head.forward(x)

    @_planned("backward")
    def backward(self, dout_nchw, arena=None, overlap=False):
        """dout (B,J,H,W) fp32 NCHW, any scale -> {parameter: fp32 gradient} for every parameter of the model.  With ``arena`` the
        gradients are its slices; ``overlap`` lets the arena all-reduce finished buckets while the earlier layers are still in flight."""
        grads = _Grads(arena, overlap)
        dx = self.head.backward(dout_nchw, grads)
        for d in reversed(self.deconvs):
            dx = d.backward(dx, grads)
            grads.flush()
        self.trunk_backward(dx, grads)
        return grads.close()


class _TrainFnH16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, trainer, *params):
        ctx.trainer, ctx.params = trainer, params
        with torch.no_grad():
            return trainer.forward(x)

    @staticmethod
    def backward(ctx, dout):
        with torch.no_grad():
            grads = ctx.trainer.backward(dout.contiguous().float())
        return (None, None) + tuple(grads.get(p) for p in ctx.params)


def trainer_for_h16(m: nn.Module):
    """The (cached) bf16 tape trainer of a SimplePose network; any other network is refused by name."""
    tr = m.__dict__.get("_vatl_trainer_h16")
    if tr is None:
        tr = m.__dict__["_vatl_trainer_h16"] = SimplePoseTrainerH16(m)
    return tr


def forward_train_h16(m: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """Training-mode forward through autograd: ``loss.backward()`` fills ``.grad`` of every parameter from the bf16 backward pass."""
    if not x.is_cuda:
        raise vh.VatlError("the pose network trains on MI355X only (there is deliberately no CPU fallback)")
    tr = trainer_for_h16(m)
    params = tuple(p for p in m.parameters() if p.requires_grad)
    return _TrainFnH16.apply(x.detach().float().contiguous(), tr, *params)
