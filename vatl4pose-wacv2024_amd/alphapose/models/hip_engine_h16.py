"""Opt-in 16-bit (float16 / bfloat16) inference forward of the pose networks on the device.

The fp32 routes of ``hip_engine`` multiply on the fp32 matrix pipe; this module trades bits for the 16-bit pipe where a caller can
afford it — the evaluation pass of an active-learning round ranks frames and does not need fp32 heat-maps to do so
(``cfg.VAL.PRECISION``).  The plans below walk the same ``nn.Module`` trees as ``hip_engine_f64`` does: every conv — the 3-channel stems
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

# The batch is cut by BYTES, as in the float64 engine: one chunk's largest tensor (the stride-2 stem output, H/2 x W/2 x 64 values of
# 2 bytes) stays below this.  Results do not depend on the cut.
CHUNK_BYTES = 1 << 28

DTYPES = (torch.float16, torch.bfloat16)


def _f32(t):
    return None if t is None else t.detach().float()


def _fold(bn, conv_bias, cout, device):
    """(scale, bias) fp32 of conv (+ bias) + eval-mode BatchNorm; (None, None) when there is neither."""
    cb = _f32(conv_bias)
    if bn is None:
        return (None, None) if cb is None else (None, cb.contiguous())
    if not bn.track_running_stats or bn.running_mean is None:
        raise NotImplementedError("the 16-bit route folds eval-mode BatchNorm: running statistics are needed")
    gamma = _f32(bn.weight) if bn.weight is not None else torch.ones(cout, device=device, dtype=torch.float32)
    beta = _f32(bn.bias) if bn.bias is not None else torch.zeros(cout, device=device, dtype=torch.float32)
    scale = gamma / torch.sqrt(_f32(bn.running_var) + bn.eps)
    bias = beta - _f32(bn.running_mean) * scale
    if cb is not None:
        bias = bias + cb * scale
    return scale.contiguous(), bias.contiguous()


class _Conv:
    __slots__ = ("w", "scale", "bias", "stride", "pad")

    def __init__(self, conv: nn.Conv2d, bn, dt):
        if conv.groups != 1 or conv.dilation != (1, 1) or conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1] \
                or not isinstance(conv.padding[0], int):
            raise NotImplementedError(f"no 16-bit plan for {conv}")
        self.w = vh.pack_conv_weight_h16(conv.weight.detach().float(), dt)
        self.stride, self.pad = conv.stride[0], conv.padding[0]
        self.scale, self.bias = _fold(bn, conv.bias, conv.out_channels, conv.weight.device)

    def __call__(self, x, relu, residual=None, out_f32_nchw=False, out=None):
        return vh.conv2d_fwd_h16(x, self.w, self.scale, self.bias, self.stride, self.pad, relu, residual=residual, out_f32_nchw=out_f32_nchw, out=out)


class _Linear:
    """nn.Linear as a 1x1 convolution on a 1x1 plane: the same kernel, the same K order."""
    __slots__ = ("w", "scale", "bias")

    def __init__(self, lin: nn.Linear, dt):
        cout, cin = lin.weight.shape
        self.w = vh.pack_conv_weight_h16(lin.weight.detach().float().reshape(cout, cin, 1, 1), dt)
        self.scale, self.bias = _fold(None, lin.bias, cout, lin.weight.device)

    def __call__(self, x, relu, out_f32):
        """x (B,1,1,C) 16-bit -> (B,1,1,Cout) 16-bit, or fp32 (B,Cout)."""
        y = vh.conv2d_fwd_h16(x, self.w, self.scale, self.bias, 1, 0, relu, out_f32_nchw=out_f32)
        return y.reshape(y.shape[0], -1) if out_f32 else y


class _Deconv:
    __slots__ = ("w", "scale", "bias")

    def __init__(self, dc: nn.ConvTranspose2d, bn, dt):
        if dc.kernel_size != (4, 4) or dc.stride != (2, 2) or dc.padding != (1, 1) or dc.output_padding != (0, 0) or dc.groups != 1:
            raise NotImplementedError(f"no 16-bit plan for {dc}")
        self.w = vh.pack_deconv_weight_h16(dc.weight.detach().float(), dt)
        self.scale, self.bias = _fold(bn, dc.bias, dc.out_channels, dc.weight.device)

    def __call__(self, x, relu=True):
        return vh.deconv4x4s2_fwd_h16(x, self.w, self.scale, self.bias, relu)


class _Block:
    """Bottleneck (conv1-conv2-conv3), BasicBlock (conv1-conv2), with or without projection; with an ``se`` gate the output of the last
    conv + BN is scaled by sigmoid(fc(avgpool)) before the skip is added (SE_Resnet.py:110-137).  The pooled vector and the gate are fp32."""

    def __init__(self, blk, dt):
        names = ("conv1", "conv2", "conv3") if hasattr(blk, "conv3") else ("conv1", "conv2")
        self.dt = dt
        self.convs = [_Conv(getattr(blk, n), getattr(blk, "bn" + n[-1]), dt) for n in names]
        ds = blk.downsample
        self.proj = _Conv(ds[0], ds[1], dt) if ds is not None else None
        se = getattr(blk, "se", None) if getattr(blk, "reduc", True) else None
        self.fc = (_Linear(se.fc[0], dt), _Linear(se.fc[2], dt)) if se is not None else None

    def __call__(self, x):
        y = x
        for c in self.convs[:-1]:
            y = c(y, relu=True)
        skip = x if self.proj is None else self.proj(x, relu=False)
        if self.fc is None:
            return self.convs[-1](y, relu=True, residual=skip)
        y = self.convs[-1](y, relu=False)
        pooled = vh.gap_fwd_h16(y)                                                          # fp32 (B, C)
        hidden = self.fc[0](vh.nchw_to_nhwc_h16(pooled.reshape(*pooled.shape, 1, 1), self.dt), relu=True, out_f32=False)
        gate = self.fc[1](hidden, relu=False, out_f32=True)                                 # fp32, pre-sigmoid
        return vh.se_scale_add_relu_h16(y, gate, skip)


class _Trunk:
    def __init__(self, net, dt):
        mp = net.maxpool
        if not (isinstance(mp, nn.MaxPool2d) and mp.kernel_size in (3, (3, 3)) and mp.stride in (2, (2, 2)) and mp.padding in (1, (1, 1)) and not mp.ceil_mode):
            raise NotImplementedError(f"no 16-bit plan for {mp}")
        self.stem = _Conv(net.conv1, net.bn1, dt)
        self.blocks = [_Block(b, dt) for stage in net.stages() for b in stage]

    def __call__(self, x):
        x = vh.maxpool3x3s2_fwd_h16(self.stem(x, relu=True))
        for b in self.blocks:
            x = b(x)
        return x


class _SimplePosePlan:
    def __init__(self, m, dt):
        self.trunk = _Trunk(m.preact, dt)
        d = m.deconv_layers
        self.deconvs = [_Deconv(d[k], d[k + 1], dt) for k in range(0, len(d), 3)]
        self.head = _Conv(m.final_layer, None, dt)

    def __call__(self, x, out=None, emb_out=None):
        x = self.trunk(x)
        if emb_out is not None:
            vh.gap_fwd_h16(x, out=emb_out)
        for dc in self.deconvs:
            x = dc(x)
        return self.head(x, relu=False, out_f32_nchw=True, out=out)


class _DUCPlan:
    def __init__(self, duc, dt):
        self.conv = _Conv(duc.conv, duc.bn, dt)

    def __call__(self, x):
        return vh.pixelshuffle2_fwd_h16(self.conv(x, relu=True))


class _FastPosePlan:
    def __init__(self, m, dt):
        self.trunk = _Trunk(m.preact, dt)
        self.duc1, self.duc2 = _DUCPlan(m.duc1, dt), _DUCPlan(m.duc2, dt)
        self.head = _Conv(m.conv_out, None, dt)

    def __call__(self, x, out=None, emb_out=None):
        x = self.trunk(x)
        if emb_out is not None:
            vh.gap_fwd_h16(x, out=emb_out)
        x = self.duc2(self.duc1(vh.pixelshuffle2_fwd_h16(x)))
        return self.head(x, relu=False, out_f32_nchw=True, out=out)


class _ConvChain:
    """Sequential of Conv-BN(-ReLU) groups (HRNet transitions and strided fusion paths)."""

    def __init__(self, seq, dt):
        groups = [seq] if isinstance(seq[0], nn.Conv2d) else list(seq)
        self.steps = [(_Conv(g[0], g[1], dt), len(g) > 2 and isinstance(g[2], nn.ReLU)) for g in groups]

    def __call__(self, x, residual=None, final_relu=None):
        for k, (conv, relu) in enumerate(self.steps):
            last = k == len(self.steps) - 1
            x = conv(x, relu=(final_relu if (last and final_relu is not None) else relu), residual=residual if last else None)
        return x


class _HRModulePlan:
    """y_i = relu(x_i + sum_{j<i} down_ij(x_j) + sum_{j>i} up(conv1x1_ij(x_j)))   (hrnet.py:242-260), summed in that order: the strided
    paths through the conv write-out's residual input, the up-sampled terms (and the ReLU) by one fuse launch."""

    def __init__(self, mod, dt):
        self.branches = [[_Block(b, dt) for b in br] for br in mod.branches]
        self.rows = []
        if mod.fuse_layers is not None:
            for i, row in enumerate(mod.fuse_layers):
                downs = [(j, _ConvChain(row[j], dt)) for j in range(i)]
                ups = [(j, _Conv(row[j][0], row[j][1], dt)) for j in range(i + 1, len(row))]
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
                acc = vh.fuse_upsample_add_h16(acc, [(conv(xs[j], relu=False), j - i) for j, conv in ups], relu=True)
            out.append(acc)
        return out


class _HRNetPlan:
    def __init__(self, m, dt):
        self.stem1, self.stem2 = _Conv(m.conv1, m.bn1, dt), _Conv(m.conv2, m.bn2, dt)
        self.layer1 = [_Block(b, dt) for b in m.layer1]
        self.stages = []
        for s in (2, 3, 4):
            trans = [None if t is None else _ConvChain(t, dt) for t in getattr(m, f"transition{s - 1}")]
            self.stages.append((trans, [_HRModulePlan(mod, dt) for mod in getattr(m, f"stage{s}")]))
        self.head = _Conv(m.final_layer, None, dt)

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
        return self.head(ys[0], relu=False, out_f32_nchw=True, out=out)


def _check_dtype(dtype, who: str) -> None:
    if dtype not in DTYPES:
        raise vh.VatlError(f"{who}: dtype must be torch.float16 or torch.bfloat16, got {dtype}")


def _check_model(m: nn.Module, who: str) -> None:
    """The refusals that need no tensor: raised before anything touches the device."""
    if m.training:
        raise vh.VatlError(f"{who} is an inference entry point (eval-mode BatchNorm is folded): call model.eval() first")
    for name, mod in m.named_modules():
        if getattr(mod, "with_dcn", False):
            raise NotImplementedError(f"{who}: {name or type(mod).__name__} holds a deformable conv (DCN); the 16-bit route does not cover deformable convs")


def _check_input(m: nn.Module, x, who: str) -> None:
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise vh.VatlError(f"{who}: expected an (N,C,H,W) tensor")
    if x.shape[0] == 0:
        raise vh.VatlError(f"{who}: empty batch")
    if not x.is_cuda:
        raise vh.VatlError(f"{who} runs on MI355X only: move the model and inputs to a HIP device (there is deliberately no CPU fallback)")
    if x.dtype != torch.float32:
        raise vh.VatlError(f"{who}: expected fp32 crops (they are rounded to the 16-bit type on the device), got {x.dtype}")
    for t in list(m.parameters()) + list(m.buffers()):
        if t.device != x.device:
            raise vh.VatlError(f"model on {t.device}, input on {x.device}")


def _check_out(t, shape, device, who: str, what: str) -> None:
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or t.device != device or not t.is_contiguous():
        raise vh.VatlError(f"{who}: {what} must be a contiguous fp32 tensor of shape {tuple(shape)} on {device}")


def _chunks(n: int, per_crop_bytes: int):
    size = max(1, CHUNK_BYTES // max(per_crop_bytes, 1))
    return [(a, min(a + size, n)) for a in range(0, n, size)]


def _net_bytes(x) -> int:
    """Largest 16-bit tensor of a crop inside the three networks: the stride-2 stem output, H/2 x W/2 x 64 (HRNet's 256 channels at H/4 are as large)."""
    return max((x.shape[2] // 2) * (x.shape[3] // 2) * 64, 8 * x.shape[2] * x.shape[3]) * 2


def _net_plan(m, dt):
    from .fastpose import FastPose
    from .hrnet import PoseHighResolutionNet
    from .simplepose import SimplePose
    if isinstance(m, SimplePose):
        return _SimplePosePlan(m, dt)
    if isinstance(m, FastPose):
        return _FastPosePlan(m, dt)
    if isinstance(m, PoseHighResolutionNet):
        return _HRNetPlan(m, dt)
    raise TypeError(f"no 16-bit plan for {type(m).__name__}")


def _run(m, x, out, emb, dtype, who):
    _check_dtype(dtype, who)
    _check_model(m, who)
    _check_input(m, x, who)
    with torch.no_grad():
        plan = _net_plan(m, dtype)
        if emb is not None and not hasattr(plan, "trunk"):
            raise vh.VatlError(f"{type(m).__name__} has no get_embedding")
        x = x.detach().contiguous()
        parts = []
        for a, b in _chunks(x.shape[0], _net_bytes(x)):
            parts.append(plan(vh.nchw_to_nhwc_h16(x[a:b], dtype), out=None if out is None else out[a:b], emb_out=None if emb is None else emb[a:b]))
        if out is not None:
            return out
        return parts[0] if len(parts) == 1 else torch.cat(parts, 0)


def forward_h16(m: nn.Module, x: torch.Tensor, out: torch.Tensor | None = None, dtype=torch.float16) -> torch.Tensor:
    """fp32 heat-maps (N, J, H/4, W/4) of SimplePose / FastPose / PoseHighResolutionNet computed in ``dtype`` (float16 or bfloat16) on the
    device — the shape and dtype ``hip_engine.forward_into`` fills, so every scorer takes them unchanged.  ``x``: fp32 NCHW crops on the
    model's device; ``out``: a contiguous fp32 device tensor to write into (it is returned), or None."""
    if out is not None:
        if not (isinstance(out, torch.Tensor) and out.dim() == 4 and out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()
                and isinstance(x, torch.Tensor) and out.shape[0] == x.shape[0]):
            raise vh.VatlError("forward_h16: out must be a contiguous fp32 device tensor with one row per crop")
    return _run(m, x, out, None, dtype, "forward_h16")


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
    _run(m, x, out, emb, dtype, "forward_with_embedding_h16")


def embedding_h16(m: nn.Module, x: torch.Tensor, dtype=torch.float16) -> torch.Tensor:
    """trunk -> global average pool -> (N, 2048) fp32 of SimplePose / FastPose (simplepose.py:88-91, fastpose.py:70-73), the trunk in ``dtype``."""
    _check_dtype(dtype, "embedding_h16")
    _check_model(m, "embedding_h16")
    _check_input(m, x, "embedding_h16")
    if not hasattr(m, "preact"):
        raise vh.VatlError(f"{type(m).__name__} has no get_embedding")
    with torch.no_grad():
        trunk = _Trunk(m.preact, dtype)
        x = x.detach().contiguous()
        return torch.cat([vh.gap_fwd_h16(trunk(vh.nchw_to_nhwc_h16(x[a:b], dtype))) for a, b in _chunks(x.shape[0], _net_bytes(x))], 0)


def features_h16(module: nn.Module, x, dtype=torch.float16):
    """A bare sub-module in ``dtype``, fp32 NCHW in and out (the input is rounded to ``dtype``, the output converted exactly): a ``ResNet``
    / ``SEResnet`` trunk, one ``Bottleneck`` / ``BasicBlock`` (with or without SE gate and projection), a ``DUC``, or a
    ``HighResolutionModule`` (``x`` = one tensor per branch; returns a list).  Input channels must be a multiple of 8 except for a trunk."""
    from .hrnet import HighResolutionModule
    from .layers.DUC import DUC
    from .layers.Resnet import ResNet
    _check_dtype(dtype, "features_h16")
    _check_model(module, "features_h16")
    xs = list(x) if isinstance(x, (list, tuple)) else [x]
    for t in xs:
        _check_input(module, t, "features_h16")
    with torch.no_grad():
        if isinstance(module, HighResolutionModule):
            if len(xs) != module.num_branches or any(t.shape[0] != xs[0].shape[0] for t in xs):
                raise vh.VatlError(f"features_h16: a HighResolutionModule with {module.num_branches} branches takes that many tensors of one batch size")
            plan = _HRModulePlan(module, dtype)
        elif not isinstance(x, torch.Tensor):
            raise vh.VatlError(f"features_h16: {type(module).__name__} takes one tensor")
        elif isinstance(module, ResNet):
            plan = _Trunk(module, dtype)
        elif isinstance(module, DUC):
            plan = _DUCPlan(module, dtype)
        elif hasattr(module, "conv2") and hasattr(module, "bn2") and hasattr(module, "downsample"):
            plan = _Block(module, dtype)
        else:
            raise TypeError(f"no 16-bit plan for {type(module).__name__}")
        xs = [t.detach().contiguous() for t in xs]
        per_crop = 2 * max(4 * sum(t[0].numel() for t in xs), (xs[0].shape[2] // 2) * (xs[0].shape[3] // 2) * 64)
        outs = []
        for a, b in _chunks(xs[0].shape[0], per_crop):
            ins = [vh.nchw_to_nhwc_h16(t[a:b], dtype) for t in xs]
            if isinstance(plan, _HRModulePlan):
                outs.append([vh.nhwc_to_nchw_h16(y) for y in plan(ins)])
            else:
                outs.append(vh.nhwc_to_nchw_h16(plan(ins[0])))
        if isinstance(plan, _HRModulePlan):
            return [torch.cat([o[i] for o in outs], 0) for i in range(len(outs[0]))]
        return torch.cat(outs, 0)
