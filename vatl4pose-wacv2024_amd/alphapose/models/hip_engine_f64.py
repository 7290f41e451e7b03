"""Float64 REFERENCE forward of the pose networks on the device.

Every parity statement about the fp32 routes rests on a float64 run of the network; this module runs it on the card instead of with
torch on the host: the plans below walk the same ``nn.Module`` trees as ``hip_engine`` does, but every conv — the 3-channel stems, the
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

# The batch is cut by BYTES: float64 NHWC activations are twice the fp32 ones (the stride-2 stem output, the largest tensor of all three
# networks, is 6.3 MB per crop at 256x192) and a handful of them are alive at a time.  One chunk's largest tensor stays below this.
CHUNK_BYTES = 1 << 30


def _d64(t):
    return None if t is None else t.detach().double()


def _fold(bn, conv_bias, cout, device):
    """(scale, bias) float64 of conv (+ bias) + eval-mode BatchNorm; (None, None) when there is neither."""
    cb = _d64(conv_bias)
    if bn is None:
        return (None, None) if cb is None else (torch.ones(cout, device=device, dtype=torch.float64), cb.contiguous())
    if not bn.track_running_stats or bn.running_mean is None:
        raise NotImplementedError("the float64 reference folds eval-mode BatchNorm: running statistics are needed")
    gamma = _d64(bn.weight) if bn.weight is not None else torch.ones(cout, device=device, dtype=torch.float64)
    beta = _d64(bn.bias) if bn.bias is not None else torch.zeros(cout, device=device, dtype=torch.float64)
    scale = gamma / torch.sqrt(_d64(bn.running_var) + bn.eps)
    bias = beta - _d64(bn.running_mean) * scale
    if cb is not None:
        bias = bias + cb * scale
    return scale.contiguous(), bias.contiguous()


class _Conv:
    __slots__ = ("w", "scale", "bias", "stride", "pad")

    def __init__(self, conv: nn.Conv2d, bn=None):
        if conv.groups != 1 or conv.dilation != (1, 1) or conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1] \
                or not isinstance(conv.padding[0], int):
            raise NotImplementedError(f"no float64 plan for {conv}")
        self.w = vh.pack_conv_weight_f64(conv.weight.detach().float())
        self.stride, self.pad = conv.stride[0], conv.padding[0]
        self.scale, self.bias = _fold(bn, conv.bias, conv.out_channels, conv.weight.device)

    def __call__(self, x, relu, residual=None, out_nchw=False, out=None):
        return vh.conv2d_fwd_f64(x, self.w, self.scale, self.bias, self.stride, self.pad, relu, residual=residual, out_nchw=out_nchw, out=out)


class _Linear:
    """nn.Linear as a 1x1 convolution on a 1x1 plane: the same kernel, the same K order."""
    __slots__ = ("w", "scale", "bias")

    def __init__(self, lin: nn.Linear):
        cout, cin = lin.weight.shape
        self.w = vh.pack_conv_weight_f64(lin.weight.detach().float().reshape(cout, cin, 1, 1))
        self.scale, self.bias = _fold(None, lin.bias, cout, lin.weight.device)

    def __call__(self, x2d, relu):
        b, c = x2d.shape
        return vh.conv2d_fwd_f64(x2d.reshape(b, 1, 1, c), self.w, self.scale, self.bias, 1, 0, relu).reshape(b, -1)


class _Deconv:
    __slots__ = ("w", "scale", "bias")

    def __init__(self, dc: nn.ConvTranspose2d, bn):
        if dc.kernel_size != (4, 4) or dc.stride != (2, 2) or dc.padding != (1, 1) or dc.output_padding != (0, 0) or dc.groups != 1:
            raise NotImplementedError(f"no float64 plan for {dc}")
        self.w = vh.pack_deconv_weight_f64(dc.weight.detach().float())
        self.scale, self.bias = _fold(bn, dc.bias, dc.out_channels, dc.weight.device)

    def __call__(self, x, relu=True):
        return vh.deconv4x4s2_fwd_f64(x, self.w, self.scale, self.bias, relu)


class _Block:
    """Bottleneck (conv1-conv2-conv3), BasicBlock (conv1-conv2), with or without projection; with an ``se`` gate the output of the last
    conv + BN is scaled by sigmoid(fc(avgpool)) before the skip is added (SE_Resnet.py:110-137)."""

    def __init__(self, blk):
        names = ("conv1", "conv2", "conv3") if hasattr(blk, "conv3") else ("conv1", "conv2")
        self.convs = [_Conv(getattr(blk, n), getattr(blk, "bn" + n[-1])) for n in names]
        ds = blk.downsample
        self.proj = _Conv(ds[0], ds[1]) if ds is not None else None
        se = getattr(blk, "se", None) if getattr(blk, "reduc", True) else None
        self.fc = (_Linear(se.fc[0]), _Linear(se.fc[2])) if se is not None else None

    def __call__(self, x):
        y = x
        for c in self.convs[:-1]:
            y = c(y, relu=True)
        skip = x if self.proj is None else self.proj(x, relu=False)
        if self.fc is None:
            return self.convs[-1](y, relu=True, residual=skip)
        y = self.convs[-1](y, relu=False)
        gate = self.fc[1](self.fc[0](vh.gap_fwd_f64(y), relu=True), relu=False)          # pre-sigmoid
        return vh.se_scale_add_relu_f64(y, gate, skip)


class _Trunk:
    def __init__(self, net):
        mp = net.maxpool
        if not (isinstance(mp, nn.MaxPool2d) and mp.kernel_size in (3, (3, 3)) and mp.stride in (2, (2, 2)) and mp.padding in (1, (1, 1)) and not mp.ceil_mode):
            raise NotImplementedError(f"no float64 plan for {mp}")
        self.stem = _Conv(net.conv1, net.bn1)
        self.blocks = [_Block(b) for stage in net.stages() for b in stage]

    def __call__(self, x):
        x = vh.maxpool3x3s2_fwd_f64(self.stem(x, relu=True))
        for b in self.blocks:
            x = b(x)
        return x


class _SimplePosePlan:
    def __init__(self, m):
        self.trunk = _Trunk(m.preact)
        d = m.deconv_layers
        self.deconvs = [_Deconv(d[k], d[k + 1]) for k in range(0, len(d), 3)]
        self.head = _Conv(m.final_layer)

    def __call__(self, x, out=None):
        x = self.trunk(x)
        for dc in self.deconvs:
            x = dc(x)
        return self.head(x, relu=False, out_nchw=True, out=out)


class _DUCPlan:
    def __init__(self, duc):
        self.conv = _Conv(duc.conv, duc.bn)

    def __call__(self, x):
        return vh.pixelshuffle2_fwd_f64(self.conv(x, relu=True))


class _FastPosePlan:
    def __init__(self, m):
        self.trunk = _Trunk(m.preact)
        self.duc1, self.duc2 = _DUCPlan(m.duc1), _DUCPlan(m.duc2)
        self.head = _Conv(m.conv_out)

    def __call__(self, x, out=None):
        x = self.duc2(self.duc1(vh.pixelshuffle2_fwd_f64(self.trunk(x))))
        return self.head(x, relu=False, out_nchw=True, out=out)


class _ConvChain:
    """Sequential of Conv-BN(-ReLU) groups (HRNet transitions and strided fusion paths)."""

    def __init__(self, seq):
        groups = [seq] if isinstance(seq[0], nn.Conv2d) else list(seq)
        self.steps = [(_Conv(g[0], g[1]), len(g) > 2 and isinstance(g[2], nn.ReLU)) for g in groups]

    def __call__(self, x, residual=None, final_relu=None):
        for k, (conv, relu) in enumerate(self.steps):
            last = k == len(self.steps) - 1
            x = conv(x, relu=(final_relu if (last and final_relu is not None) else relu), residual=residual if last else None)
        return x


class _HRModulePlan:
    """y_i = relu(x_i + sum_{j<i} down_ij(x_j) + sum_{j>i} up(conv1x1_ij(x_j)))   (hrnet.py:242-260), summed in that order: the strided
    paths through the conv write-out's residual input, the up-sampled terms (and the ReLU) by one fuse launch."""

    def __init__(self, mod):
        self.branches = [[_Block(b) for b in br] for br in mod.branches]
        self.rows = []
        if mod.fuse_layers is not None:
            for i, row in enumerate(mod.fuse_layers):
                downs = [(j, _ConvChain(row[j])) for j in range(i)]
                ups = [(j, _Conv(row[j][0], row[j][1])) for j in range(i + 1, len(row))]
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
                acc = vh.fuse_upsample_add_f64(acc, [(conv(xs[j], relu=False), j - i) for j, conv in ups], relu=True)
            out.append(acc)
        return out


class _HRNetPlan:
    def __init__(self, m):
        self.stem1, self.stem2 = _Conv(m.conv1, m.bn1), _Conv(m.conv2, m.bn2)
        self.layer1 = [_Block(b) for b in m.layer1]
        self.stages = []
        for s in (2, 3, 4):
            trans = [None if t is None else _ConvChain(t) for t in getattr(m, f"transition{s - 1}")]
            self.stages.append((trans, [_HRModulePlan(mod) for mod in getattr(m, f"stage{s}")]))
        self.head = _Conv(m.final_layer)

    def __call__(self, x, out=None):
        x = self.stem2(self.stem1(x, relu=True), relu=True)
        for b in self.layer1:
            x = b(x)
        ys = [x]
        for trans, mods in self.stages:
            xs = [ys[i] if t is None else t(ys[-1]) for i, t in enumerate(trans)]
            for mod in mods:
                xs = mod(xs)
            ys = xs
        return self.head(ys[0], relu=False, out_nchw=True, out=out)


def _check_model(m: nn.Module, who: str) -> None:
    """The refusals that need no tensor: raised before anything touches the device."""
    if m.training:
        raise vh.VatlError(f"{who} is an inference entry point (eval-mode BatchNorm is folded): call model.eval() first")
    for name, mod in m.named_modules():
        if getattr(mod, "with_dcn", False):
            raise NotImplementedError(f"{who}: {name or type(mod).__name__} holds a deformable conv (DCN); the float64 reference does not cover deformable convs")


def _check_input(m: nn.Module, x, who: str) -> None:
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise vh.VatlError(f"{who}: expected an (N,C,H,W) tensor")
    if x.shape[0] == 0:
        raise vh.VatlError(f"{who}: empty batch")
    if not x.is_cuda:
        raise vh.VatlError(f"{who} runs on MI355X only: move the model and inputs to a HIP device (there is deliberately no CPU fallback)")
    if x.dtype not in (torch.float32, torch.float64):
        raise vh.VatlError(f"{who}: expected fp32 or float64 crops, got {x.dtype}")
    for t in list(m.parameters()) + list(m.buffers()):
        if t.device != x.device:
            raise vh.VatlError(f"model on {t.device}, input on {x.device}")


def _chunks(n: int, per_crop_bytes: int):
    size = max(1, CHUNK_BYTES // max(per_crop_bytes, 1))
    return [(a, min(a + size, n)) for a in range(0, n, size)]


def _net_bytes(x) -> int:
    """Largest float64 tensor of a crop inside the three networks: the stride-2 stem output, H/2 x W/2 x 64 (HRNet's 256 channels at H/4 are as large)."""
    return max((x.shape[2] // 2) * (x.shape[3] // 2) * 64, x.shape[1] * x.shape[2] * x.shape[3]) * 8


def _net_plan(m):
    from .fastpose import FastPose
    from .hrnet import PoseHighResolutionNet
    from .simplepose import SimplePose
    if isinstance(m, SimplePose):
        return _SimplePosePlan(m)
    if isinstance(m, FastPose):
        return _FastPosePlan(m)
    if isinstance(m, PoseHighResolutionNet):
        return _HRNetPlan(m)
    raise TypeError(f"no float64 plan for {type(m).__name__}")


def forward_f64(m: nn.Module, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Heat-maps (N, J, H/4, W/4) of SimplePose / FastPose / PoseHighResolutionNet in float64 on the device.  ``x``: fp32 (converted exactly)
    or float64 NCHW crops on the model's device; ``out``: a contiguous float64 device tensor to write into, or None."""
    _check_model(m, "forward_f64")
    _check_input(m, x, "forward_f64")
    with torch.no_grad():
        plan = _net_plan(m)
        x = x.detach().contiguous()
        parts = []
        for a, b in _chunks(x.shape[0], _net_bytes(x)):
            parts.append(plan(vh.nchw_to_nhwc_f64(x[a:b]), out=None if out is None else out[a:b]))
        if out is not None:
            return out
        return parts[0] if len(parts) == 1 else torch.cat(parts, 0)


def embedding_f64(m: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """trunk -> global average pool -> (N, 2048) float64 of SimplePose / FastPose (simplepose.py:88-91, fastpose.py:70-73)."""
    _check_model(m, "embedding_f64")
    _check_input(m, x, "embedding_f64")
    if not hasattr(m, "preact"):
        raise vh.VatlError(f"{type(m).__name__} has no get_embedding")
    with torch.no_grad():
        trunk = _Trunk(m.preact)
        x = x.detach().contiguous()
        return torch.cat([vh.gap_fwd_f64(trunk(vh.nchw_to_nhwc_f64(x[a:b]))) for a, b in _chunks(x.shape[0], _net_bytes(x))], 0)


def features_f64(module: nn.Module, x):
    """A bare sub-module in float64, NCHW in and out: a ``ResNet`` / ``SEResnet`` trunk, one ``Bottleneck`` / ``BasicBlock`` (with or
    without SE gate and projection), a ``DUC``, or a ``HighResolutionModule`` (``x`` = one tensor per branch; returns a list)."""
    from .hrnet import HighResolutionModule
    from .layers.DUC import DUC
    from .layers.Resnet import ResNet
    _check_model(module, "features_f64")
    xs = list(x) if isinstance(x, (list, tuple)) else [x]
    for t in xs:
        _check_input(module, t, "features_f64")
    with torch.no_grad():
        if isinstance(module, HighResolutionModule):
            if len(xs) != module.num_branches or any(t.shape[0] != xs[0].shape[0] for t in xs):
                raise vh.VatlError(f"features_f64: a HighResolutionModule with {module.num_branches} branches takes that many tensors of one batch size")
            plan = _HRModulePlan(module)
        elif not isinstance(x, torch.Tensor):
            raise vh.VatlError(f"features_f64: {type(module).__name__} takes one tensor")
        elif isinstance(module, ResNet):
            plan = _Trunk(module)
        elif isinstance(module, DUC):
            plan = _DUCPlan(module)
        elif hasattr(module, "conv2") and hasattr(module, "bn2") and hasattr(module, "downsample"):
            plan = _Block(module)
        else:
            raise TypeError(f"no float64 plan for {type(module).__name__}")
        xs = [t.detach().contiguous() for t in xs]
        per_crop = 8 * max(4 * sum(t[0].numel() for t in xs), (xs[0].shape[2] // 2) * (xs[0].shape[3] // 2) * 64)
        outs = []
        for a, b in _chunks(xs[0].shape[0], per_crop):
            ins = [vh.nchw_to_nhwc_f64(t[a:b]) for t in xs]
            if isinstance(plan, _HRModulePlan):
                outs.append([vh.nhwc_to_nchw_f64(y) for y in plan(ins)])
            else:
                outs.append(vh.nhwc_to_nchw_f64(plan(ins[0])))
        if isinstance(plan, _HRModulePlan):
            return [torch.cat([o[i] for o in outs], 0) for i in range(len(outs[0]))]
        return torch.cat(outs, 0)
