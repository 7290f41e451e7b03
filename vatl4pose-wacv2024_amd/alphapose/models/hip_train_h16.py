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
from . import hip_train_tape as tape
from .hip_train import _Grads, _gout, _side

DT = torch.bfloat16

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


class _Ops:
    """What the bf16 step decides on the shared tape: 16-bit library calls, ``_Packed`` filters built with the layers and fetched under
    the trainer's plan, BatchNorm on the module's own parameters and running statistics (updated in place, counters as the fp32 trainer
    counts them), gradients into the ``GradArena`` slices where there is one, weight gradients on the fp32 trainer's side stream."""

    NAME, HEAD_NEEDS_BIAS = "bf16", False
    REFUSALS = (lambda cls: f"RETRAIN.PRECISION bf16 serves SimplePose only, not {cls}: it trains in fp32",
                "RETRAIN.PRECISION bf16 does not serve deformable bottlenecks (DCN): they train in fp32",
                "RETRAIN.PRECISION bf16 serves the bottleneck ResNets (50 / 101 / 152) only")

    def check_bn(self, bn):
        pass

    def conv_filters(self, l):
        p = l.conv.weight
        return (_Packed(p, lambda w: vh.pack_conv_weight_h16(w, DT), vh.PACK_H16_CONV),
                _Packed(p, lambda w: vh.pack_conv_weight_dgrad_h16(w, l.stride, l.pad, DT), vh.PACK_H16_DGRAD, l.stride, l.pad) if l.need_dx else None)

    head_filters = conv_filters

    def deconv_filters(self, l):
        p = l.dc.weight
        return _Packed(p, lambda w: vh.pack_deconv_weight_h16(w, DT), vh.PACK_H16_DECONV), _Packed(p, lambda w: vh.pack_conv_weight_h16(w, DT), vh.PACK_H16_CONV)

    def input(self, x_nchw):
        return vh.nchw_to_nhwc_h16(x_nchw.contiguous(), DT)                      # 3 -> 8 channels (zeros)

    def conv(self, l, x):
        return vh.conv2d_fwd_h16(x, l.w.get(), None, None, l.stride, l.pad, False)

    def conv_wd(self, l):
        return None                                                              # the backward pass fetches ``l.wd``: the plan keeps it fresh

    deconv_wd = conv_wd

    def deconv(self, l, x):
        return vh.deconv4x4s2_fwd_h16(x, l.w.get(), None, None, False)

    def head(self, l, x):
        hip_train._flush_batch_counters()
        return vh.conv2d_fwd_h16(x, l.w.get(), None, l.conv.bias.detach(), 1, 0, False, out_f32_nchw=True), None

    def bn_fwd(self, bn, z, skip, relu):
        mean, invstd, scale, bias = vh.bn_train_fwd_stats_h16(z, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.momentum, bn.eps)
        hip_train._count_batch(bn)
        return vh.bn_apply_h16(z, scale, bias, skip, relu), (mean, invstd)

    def bn_bwd(self, bn, st, dy, y, z, grads, want_g):
        dz, g, grads[bn.weight], grads[bn.bias] = vh.bn_train_bwd_h16(dy, y, z, bn.weight.detach(), *st, want_g=want_g, dgamma=_gout(grads, bn.weight),
                                                                      dbeta=_gout(grads, bn.bias))
        return dz, g

    def wgrad(self, p, grads, x, dz, cout, cin, r, s, stride, pad, transposed=False, side=True):
        ow = _gout(grads, p)
        if not side:                                       # the head's weight gradient stays on the main stream
            return vh.conv2d_wgrad_h16(x, dz, cout, cin, r, s, stride, pad, out=ow)
        if ow is None:                                     # no arena: the gradient tensor belongs to the calling stream, which reads it after the join
            ow = torch.empty(p.shape, device=x.device, dtype=torch.float32)
        # beside the critical chain (BatchNorm backward -> data gradient -> previous layer), as the fp32 trainer runs its weight gradients
        return _side.run(lambda: vh.conv2d_wgrad_h16(x, dz, cout, cin, r, s, stride, pad, transposed=transposed, out=ow), x, dz)

    def dgrad(self, l, wd, dz, xshape, residual=None):
        return vh.conv2d_dgrad_h16(dz, l.wd.get(), xshape, l.r, l.s, l.stride, l.pad, residual=residual)

    def deconv_dgrad(self, l, wd, dz):
        return vh.conv2d_fwd_h16(dz, l.wd.get(), None, None, 2, 1, False)

    def head_cotangent(self, l, x, dout_nchw, grads):
        dout_nchw = dout_nchw.contiguous()
        # the bias gradient stays on the fp32 reduction of dout
        grads[l.conv.bias] = vh.col_sum(vh.nchw_to_nhwc(dout_nchw, 32))[:l.cout].contiguous()
        return vh.nchw_to_nhwc_h16(dout_nchw, DT)                                # 17 -> 24 channels (zeros), rounded to bf16

    def maxpool_fwd(self, x):
        return vh.maxpool3x3s2_fwd_h16(x)

    def maxpool_bwd(self, dpool, x):
        return vh.maxpool3x3s2_bwd_h16(dpool, x)

    def flush(self, grads):
        if isinstance(grads, _Grads):
            grads.flush()

    def join(self):
        _side.join()


class SimplePoseTrainerH16(tape.SimplePoseTape):
    """Tape-based forward/backward of SimplePose in training mode with bf16 storage; the interface of ``hip_train.SimplePoseTrainer``."""

    def __init__(self, m):
        super().__init__(_Ops(), m)
        convs = [self.stem] + [c for b in self.blocks for c in (b.c1, b.c2, b.c3, b.proj) if c is not None] + self.deconvs + [self.head]
        self.packed = [q for c in convs for q in (c.w, c.wd) if q is not None]    # every bf16 filter of a step: 57 + 56 for the R50

    @_planned("forward")
    def forward(self, x_nchw):
        """x (B,3,H,W) fp32 NCHW -> heat-maps (B,J,H/4,W/4) fp32 NCHW."""
        return super().forward(x_nchw)

    @_planned("backward")
    def backward(self, dout_nchw, arena=None, overlap=False):
        """dout (B,J,H,W) fp32 NCHW, any scale -> {parameter: fp32 gradient} for every parameter of the model.  With ``arena`` the
        gradients are its slices; ``overlap`` lets the arena all-reduce finished buckets while the earlier layers are still in flight."""
        return super().backward(dout_nchw, _Grads(arena, overlap)).close()


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
