"""Optimizers of the fine-tune step on MI355X (reference: ActiveLearning.py:219-231).

``AdamW`` has torch.optim.AdamW's constructor and param-group semantics (the reference builds
three groups with lr x{10, 1, 5}); ``step()`` is one ``vatl_adamw_step_multi`` launch per parameter group
(a device table of tensor pointers) instead of torch's element-wise kernels.  ``lr`` is read from the group at every step, so
``torch.optim.lr_scheduler.ExponentialLR`` works on it unchanged.  ``Adam`` and ``RMSprop`` (the two optimisers of the pose-network
pre-training script, posetrack_train.py:155-158) and ``SGD`` step the same way: one launch per (group, step).
"""
from __future__ import annotations

import torch

import vatl_hip as vh


class _Stepper(torch.optim.Optimizer):
    """The step loop the optimisers share; a subclass names its state buffers, its per-tensor call and, if it has one, its multi call."""
    _buffers = ()                                  # state keys, in the order of the calls' buffer arguments
    _kernel = None                                 # (p, g, *buffers, *hyper): one tensor
    _multi = None                                  # (params, grads, *buffer lists, *hyper): one launch; None: one launch per tensor

    def _hyper(self, group, step):
        """The arguments of ``_kernel`` / ``_multi`` after the tensors."""
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            batch = {}                                   # step count -> tensors: one multi-tensor launch per (group, step)
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    for name in self._buffers:
                        st[name] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["step"] += 1
                batch.setdefault(st["step"], []).append((p, p.grad.contiguous()) + tuple(st[name] for name in self._buffers))
            for step, items in batch.items():
                hyper = self._hyper(group, step)
                if self._multi is not None and all(t[0].is_contiguous() for t in items):
                    self._multi([t[0].data for t in items], *([t[k] for t in items] for k in range(1, 2 + len(self._buffers))), *hyper)
                else:
                    for p, *rest in items:
                        self._kernel(p.data, *rest, *hyper)
                # the in-place update went through the C ABI: bump the version counters ourselves, the
                # inference plans key their packed-weight caches on them
                for p, *_ in items:
                    torch.autograd.graph.increment_version(p)
        return loss


class AdamW(_Stepper):
    _buffers = ("exp_avg", "exp_avg_sq")
    _kernel = staticmethod(vh.adamw_step)
    _multi = staticmethod(vh.adamw_step_multi)     # one launch per parameter group (161 tensors for SimplePose-R50)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("invalid AdamW hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _hyper(self, group, step):
        return step, group["lr"], group["weight_decay"], group["betas"], group["eps"]


class Adam(AdamW):
    """torch.optim.Adam (ActiveLearning.py:222-223): weight decay, if any, is an L2 term on the gradient."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)

    _kernel = staticmethod(vh.adam_step)
    _multi = staticmethod(vh.adam_step_multi)      # one launch per parameter group, the per-tensor kernel's bits


class RMSprop(_Stepper):
    """torch.optim.RMSprop with its defaults (posetrack_train.py:157-158): momentum 0, not centered; weight decay is an L2 term."""
    _buffers = ("square_avg",)
    _kernel = staticmethod(vh.rmsprop_step)
    _multi = staticmethod(vh.rmsprop_step_multi)

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False):
        if lr < 0 or eps < 0 or weight_decay < 0 or alpha < 0:
            raise ValueError("invalid RMSprop hyper-parameters")
        if momentum != 0 or centered:
            raise ValueError("RMSprop: only momentum=0, centered=False (torch's defaults) have a kernel")
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay))

    def _hyper(self, group, step):                 # the update has no step-dependent scalar
        return group["lr"], group["alpha"], group["eps"], group["weight_decay"]


class SGD(_Stepper):
    """torch.optim.SGD with momentum as the reference configures it (ActiveLearning.py:220-221)."""
    _buffers = ("momentum_buffer",)
    _kernel = staticmethod(vh.sgd_step)
    _multi = staticmethod(vh.sgd_step_multi)       # one launch per (group, step count) instead of 878 for HRNet-W32

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("invalid SGD hyper-parameters")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))

    def _hyper(self, group, step):
        return step, group["lr"], group["momentum"], group["weight_decay"]
