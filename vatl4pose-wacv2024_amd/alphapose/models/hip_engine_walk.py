"""The module-tree walker of the float64 reference forward (``hip_engine_f64``) and of the opt-in 16-bit forward (``hip_engine_h16``).

Both engines run the same program: the plans below walk the ``nn.Module`` trees of the three pose networks, send every conv — stems,
heads and the SE gates' Linear layers included — to ONE generic implicit GEMM, transposed convs to the same kernel as four 2x2 phases,
and the glue between them to small kernels.  What differs between the precisions — which ``vh.*`` call, how BatchNorm is folded, how
the SE gate travels, sizes, accepted inputs, the words of the messages — is the ``ops`` object each engine module defines and hands to
every plan.  A change to a plan is made here, once, and both precisions get it.

Nothing is cached: a plan packs its filters from the parameters' current values when it is built, lives for one call and writes no
attribute on any ``nn.Module``.  Importing this module does not load the library.
"""
from __future__ import annotations

import torch
import torch.nn as nn

import vatl_hip as vh


def _fold(ops, bn, conv_bias, cout, device):
    """(scale, bias) of conv (+ bias) + eval-mode BatchNorm, computed in ``ops.fold_dtype`` from the parameters converted to it; (None,
    None) when there is neither.  A bias without BatchNorm comes with a scale of ones if ``ops.unit_scale``, else with None."""
    dtype = ops.fold_dtype

    def cast(t):
        return None if t is None else t.detach().to(dtype)
    cb = cast(conv_bias)
    if bn is None:
        return (None, None) if cb is None else (torch.ones(cout, device=device, dtype=dtype) if ops.unit_scale else None, cb.contiguous())
    if not bn.track_running_stats or bn.running_mean is None:
        raise NotImplementedError(f"the {ops.route} folds eval-mode BatchNorm: running statistics are needed")
    gamma = cast(bn.weight) if bn.weight is not None else torch.ones(cout, device=device, dtype=dtype)
    beta = cast(bn.bias) if bn.bias is not None else torch.zeros(cout, device=device, dtype=dtype)
    scale = gamma / torch.sqrt(cast(bn.running_var) + bn.eps)
    bias = beta - cast(bn.running_mean) * scale
    if cb is not None:
        bias = bias + cb * scale
    return scale.contiguous(), bias.contiguous()


class _Conv:
    __slots__ = ("ops", "w", "scale", "bias", "stride", "pad")

    def __init__(self, ops, conv: nn.Conv2d, bn=None):
        if conv.groups != 1 or conv.dilation != (1, 1) or conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1] \
                or not isinstance(conv.padding[0], int):
            raise NotImplementedError(f"no {ops.plan} for {conv}")
        self.ops = ops
        self.w = ops.pack_conv(conv.weight.detach().float())
        self.stride, self.pad = conv.stride[0], conv.padding[0]
        self.scale, self.bias = _fold(ops, bn, conv.bias, conv.out_channels, conv.weight.device)

    def __call__(self, x, relu, residual=None, final=False, out=None):
        """``final``: the write-out that leaves the engine (NCHW; fp32 on the 16-bit route)."""
        return self.ops.conv(x, self.w, self.scale, self.bias, self.stride, self.pad, relu, residual=residual, final=final, out=out)


class _Linear:
    """nn.Linear as a 1x1 convolution on a 1x1 plane, (B,1,1,C) in: the same kernel, the same K order."""
    __slots__ = ("ops", "w", "scale", "bias")

    def __init__(self, ops, lin: nn.Linear):
        cout, cin = lin.weight.shape
        self.ops = ops
        self.w = ops.pack_conv(lin.weight.detach().float().reshape(cout, cin, 1, 1))
        self.scale, self.bias = _fold(ops, None, lin.bias, cout, lin.weight.device)

    def __call__(self, x, relu, final=False):
        return self.ops.conv(x, self.w, self.scale, self.bias, 1, 0, relu, final=final)


class _Deconv:
    __slots__ = ("ops", "w", "scale", "bias")

    def __init__(self, ops, dc: nn.ConvTranspose2d, bn):
        if dc.kernel_size != (4, 4) or dc.stride != (2, 2) or dc.padding != (1, 1) or dc.output_padding != (0, 0) or dc.groups != 1:
            raise NotImplementedError(f"no {ops.plan} for {dc}")
        self.ops = ops
        self.w = ops.pack_deconv(dc.weight.detach().float())
        self.scale, self.bias = _fold(ops, bn, dc.bias, dc.out_channels, dc.weight.device)

    def __call__(self, x, relu=True):
        return self.ops.deconv(x, self.w, self.scale, self.bias, relu)


class _Block:
    """Bottleneck (conv1-conv2-conv3), BasicBlock (conv1-conv2), with or without projection; with an ``se`` gate the output of the last
    conv + BN is scaled by sigmoid(fc(avgpool)) before the skip is added (SE_Resnet.py:110-137)."""

    def __init__(self, ops, blk):
        names = ("conv1", "conv2", "conv3") if hasattr(blk, "conv3") else ("conv1", "conv2")
        self.ops = ops
        self.convs = [_Conv(ops, getattr(blk, n), getattr(blk, "bn" + n[-1])) for n in names]
        ds = blk.downsample
        self.proj = _Conv(ops, ds[0], ds[1]) if ds is not None else None
        se = getattr(blk, "se", None) if getattr(blk, "reduc", True) else None
        self.fc = (_Linear(ops, se.fc[0]), _Linear(ops, se.fc[2])) if se is not None else None

    def __call__(self, x):
        y = x
        for c in self.convs[:-1]:
            y = c(y, relu=True)
        skip = x if self.proj is None else self.proj(x, relu=False)
        if self.fc is None:
            return self.convs[-1](y, relu=True, residual=skip)
        y = self.convs[-1](y, relu=False)
        gate = self.ops.se_gate(self.ops.gap(y), self.fc[0], self.fc[1])                    # pre-sigmoid
        return self.ops.se_scale_add_relu(y, gate, skip)


class _Trunk:
    def __init__(self, ops, net):
        mp = net.maxpool
        if not (isinstance(mp, nn.MaxPool2d) and mp.kernel_size in (3, (3, 3)) and mp.stride in (2, (2, 2)) and mp.padding in (1, (1, 1)) and not mp.ceil_mode):
            raise NotImplementedError(f"no {ops.plan} for {mp}")
        self.ops = ops
        self.stem = _Conv(ops, net.conv1, net.bn1)
        self.blocks = [_Block(ops, b) for stage in net.stages() for b in stage]

    def __call__(self, x, emb_out=None):
        """``emb_out``: the get_embedding vectors of the same pass, kept where the route offers that."""
        x = self.ops.maxpool(self.stem(x, relu=True))
        for b in self.blocks:
            x = b(x)
        if emb_out is not None:
            self.ops.gap(x, out=emb_out)
        return x


class _SimplePosePlan:
    def __init__(self, ops, m):
        self.trunk = _Trunk(ops, m.preact)
        d = m.deconv_layers
        self.deconvs = [_Deconv(ops, d[k], d[k + 1]) for k in range(0, len(d), 3)]
        self.head = _Conv(ops, m.final_layer)

    def __call__(self, x, out=None, emb_out=None):
        x = self.trunk(x, emb_out)
        for dc in self.deconvs:
            x = dc(x)
        return self.head(x, relu=False, final=True, out=out)


class _DUCPlan:
    def __init__(self, ops, duc):
        self.ops = ops
        self.conv = _Conv(ops, duc.conv, duc.bn)

    def __call__(self, x):
        return self.ops.pixelshuffle(self.conv(x, relu=True))


class _FastPosePlan:
    def __init__(self, ops, m):
        self.ops = ops
        self.trunk = _Trunk(ops, m.preact)
        self.duc1, self.duc2 = _DUCPlan(ops, m.duc1), _DUCPlan(ops, m.duc2)
        self.head = _Conv(ops, m.conv_out)

    def __call__(self, x, out=None, emb_out=None):
        x = self.duc2(self.duc1(self.ops.pixelshuffle(self.trunk(x, emb_out))))
        return self.head(x, relu=False, final=True, out=out)


class _ConvChain:
    """Sequential of Conv-BN(-ReLU) groups (HRNet transitions and strided fusion paths)."""

    def __init__(self, ops, seq):
        groups = [seq] if isinstance(seq[0], nn.Conv2d) else list(seq)
        self.steps = [(_Conv(ops, g[0], g[1]), len(g) > 2 and isinstance(g[2], nn.ReLU)) for g in groups]

    def __call__(self, x, residual=None, final_relu=None):
        for k, (conv, relu) in enumerate(self.steps):
            last = k == len(self.steps) - 1
            x = conv(x, relu=(final_relu if (last and final_relu is not None) else relu), residual=residual if last else None)
        return x


class _HRModulePlan:
    """y_i = relu(x_i + sum_{j<i} down_ij(x_j) + sum_{j>i} up(conv1x1_ij(x_j)))   (hrnet.py:242-260), summed in that order: the strided
    paths through the conv write-out's residual input, the up-sampled terms (and the ReLU) by one fuse launch."""

    def __init__(self, ops, mod):
        self.ops = ops
        self.branches = [[_Block(ops, b) for b in br] for br in mod.branches]
        self.rows = []
        if mod.fuse_layers is not None:
            for i, row in enumerate(mod.fuse_layers):
                downs = [(j, _ConvChain(ops, row[j])) for j in range(i)]
                ups = [(j, _Conv(ops, row[j][0], row[j][1])) for j in range(i + 1, len(row))]
                self.rows.append((i, downs, ups))

    def __call__(self, xs):
        xs = list(xs)
        for i, br in enumerate(self.branches):
            for blk in br:
                xs[i] = blk(xs[i])
        if not self.rows:
            return xs
        out = []
        for i, downs, ups in self.rows:
            acc = xs[i]
            for k, (j, chain) in enumerate(downs):
                acc = chain(xs[j], residual=acc, final_relu=(not ups and k == len(downs) - 1))
            if ups:
                acc = self.ops.fuse_upsample_add(acc, [(conv(xs[j], relu=False), j - i) for j, conv in ups], relu=True)
            out.append(acc)
        return out


class _HRNetPlan:
    def __init__(self, ops, m):
        self.stem1, self.stem2 = _Conv(ops, m.conv1, m.bn1), _Conv(ops, m.conv2, m.bn2)
        self.layer1 = [_Block(ops, b) for b in m.layer1]
        self.stages = []
        for s in (2, 3, 4):
            trans = [None if t is None else _ConvChain(ops, t) for t in getattr(m, f"transition{s - 1}")]
            self.stages.append((trans, [_HRModulePlan(ops, mod) for mod in getattr(m, f"stage{s}")]))
        self.head = _Conv(ops, m.final_layer)

    def __call__(self, x, out=None, emb_out=None):
        x = self.stem2(self.stem1(x, relu=True), relu=True)
        for b in self.layer1:
            x = b(x)
        ys = [x]
        for trans, mods in self.stages:
            xs = [ys[i] if t is None else t(ys[-1]) for i, t in enumerate(trans)]
            for mod in mods:
                xs = mod(xs)
            ys = xs
        return self.head(ys[0], relu=False, final=True, out=out)


def _check_model(ops, m: nn.Module, who: str) -> None:
    """The refusals that need no tensor: raised before anything touches the device."""
    if m.training:
        raise vh.VatlError(f"{who} is an inference entry point (eval-mode BatchNorm is folded): call model.eval() first")
    for name, mod in m.named_modules():
        if getattr(mod, "with_dcn", False):
            raise NotImplementedError(f"{who}: {name or type(mod).__name__} holds a deformable conv (DCN); the {ops.route} does not cover deformable convs")


def _check_input(ops, m: nn.Module, x, who: str) -> None:
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise vh.VatlError(f"{who}: expected an (N,C,H,W) tensor")
    if x.shape[0] == 0:
        raise vh.VatlError(f"{who}: empty batch")
    if not x.is_cuda:
        raise vh.VatlError(f"{who} runs on MI355X only: move the model and inputs to a HIP device (there is deliberately no CPU fallback)")
    if x.dtype not in ops.in_dtypes:
        raise vh.VatlError(f"{who}: expected {ops.in_words}, got {x.dtype}")
    for t in list(m.parameters()) + list(m.buffers()):
        if t.device != x.device:
            raise vh.VatlError(f"model on {t.device}, input on {x.device}")


def _chunks(ops, n: int, per_crop_bytes: int):
    size = max(1, ops.chunk_bytes() // max(per_crop_bytes, 1))
    return [(a, min(a + size, n)) for a in range(0, n, size)]


def _net_bytes(ops, x) -> int:
    """Largest tensor of a crop inside the three networks: the stride-2 stem output, H/2 x W/2 x 64 (HRNet's 256 channels at H/4 are as large)."""
    return max((x.shape[2] // 2) * (x.shape[3] // 2) * 64, ops.in_channels(x.shape[1]) * x.shape[2] * x.shape[3]) * ops.esize


def _net_plan(ops, m):
    from .fastpose import FastPose
    from .hrnet import PoseHighResolutionNet
    from .simplepose import SimplePose
    if isinstance(m, SimplePose):
        return _SimplePosePlan(ops, m)
    if isinstance(m, FastPose):
        return _FastPosePlan(ops, m)
    if isinstance(m, PoseHighResolutionNet):
        return _HRNetPlan(ops, m)
    raise TypeError(f"no {ops.plan} for {type(m).__name__}")


def forward(ops, m, x, out, emb, who: str):
    """Heat-maps of a whole network, chunk by chunk, into ``out`` (or a new tensor); ``emb``: where the embeddings of the same pass go."""
    _check_model(ops, m, who)
    _check_input(ops, m, x, who)
    with torch.no_grad():
        plan = _net_plan(ops, m)
        if emb is not None and not hasattr(plan, "trunk"):
            raise vh.VatlError(f"{type(m).__name__} has no get_embedding")
        x = x.detach().contiguous()
        parts = []
        for a, b in _chunks(ops, x.shape[0], _net_bytes(ops, x)):
            parts.append(plan(ops.to_nhwc(x[a:b]), out=None if out is None else out[a:b], emb_out=None if emb is None else emb[a:b]))
        if out is not None:
            return out
        return parts[0] if len(parts) == 1 else torch.cat(parts, 0)


def embedding(ops, m, x, who: str):
    """trunk -> global average pool -> (N, 2048) of SimplePose / FastPose (simplepose.py:88-91, fastpose.py:70-73)."""
    _check_model(ops, m, who)
    _check_input(ops, m, x, who)
    if not hasattr(m, "preact"):
        raise vh.VatlError(f"{type(m).__name__} has no get_embedding")
    with torch.no_grad():
        trunk = _Trunk(ops, m.preact)
        x = x.detach().contiguous()
        return torch.cat([ops.gap(trunk(ops.to_nhwc(x[a:b]))) for a, b in _chunks(ops, x.shape[0], _net_bytes(ops, x))], 0)


def features(ops, module, x, who: str):
    """A bare sub-module, NCHW in and out: a ``ResNet`` / ``SEResnet`` trunk, one ``Bottleneck`` / ``BasicBlock`` (with or without SE
    gate and projection), a ``DUC``, or a ``HighResolutionModule`` (``x`` = one tensor per branch; returns a list)."""
    from .hrnet import HighResolutionModule
    from .layers.DUC import DUC
    from .layers.Resnet import ResNet
    _check_model(ops, module, who)
    xs = list(x) if isinstance(x, (list, tuple)) else [x]
    for t in xs:
        _check_input(ops, module, t, who)
    with torch.no_grad():
        if isinstance(module, HighResolutionModule):
            if len(xs) != module.num_branches or any(t.shape[0] != xs[0].shape[0] for t in xs):
                raise vh.VatlError(f"{who}: a HighResolutionModule with {module.num_branches} branches takes that many tensors of one batch size")
            plan = _HRModulePlan(ops, module)
        elif not isinstance(x, torch.Tensor):
            raise vh.VatlError(f"{who}: {type(module).__name__} takes one tensor")
        elif isinstance(module, ResNet):
            plan = _Trunk(ops, module)
        elif isinstance(module, DUC):
            plan = _DUCPlan(ops, module)
        elif hasattr(module, "conv2") and hasattr(module, "bn2") and hasattr(module, "downsample"):
            plan = _Block(ops, module)
        else:
            raise TypeError(f"no {ops.plan} for {type(module).__name__}")
        xs = [t.detach().contiguous() for t in xs]
        per_crop = ops.esize * max(4 * sum(t[0].numel() for t in xs), (xs[0].shape[2] // 2) * (xs[0].shape[3] // 2) * 64)
        outs = []
        for a, b in _chunks(ops, xs[0].shape[0], per_crop):
            ins = [ops.to_nhwc(t[a:b]) for t in xs]
            if isinstance(plan, _HRModulePlan):
                outs.append([ops.to_nchw(y) for y in plan(ins)])
            else:
                outs.append(ops.to_nchw(plan(ins[0])))
        if isinstance(plan, _HRModulePlan):
            return [torch.cat([o[i] for o in outs], 0) for i in range(len(outs[0]))]
        return torch.cat(outs, 0)
