"""The tape the float64 reference step and the bf16 step of SimplePose share: ONE copy of the graph walk, so that the yardstick and the
step it judges cannot come to measure different graphs.

The layers (``_ConvBN``, ``_DeconvBN``, ``_BottleneckT``, ``_HeadT``) and the trainer (``SimplePoseTape``) hold what the two steps
have in common: the order of the layers, the skip wiring of the bottleneck, which tensors a layer keeps for its backward pass, the
``want_g`` logic, the transposed conv's data gradient as a plain 4x4 / 2 / 1 conv of dz, the geometry refusals.  Everything a precision
decides comes in through an ``ops`` object (the ``_Ops`` class of the precision's own module, as the plans of ``hip_engine_walk`` take
theirs): which library call is made, where the packed filters come from, where the BatchNorm statistics and the gradients go, the
side stream, the wording of the messages.  Nothing here names a precision, loads the library or knows the fp32 trainer.
"""
import torch.nn as nn


def check_model(m, not_simplepose, dcn: str, basic_block: str):
    """The networks the tape serves; everything else is refused by name, before anything touches the device, in the precision's own
    words (``not_simplepose``: class name -> message)."""
    from .simplepose import SimplePose
    if not isinstance(m, SimplePose):
        raise NotImplementedError(not_simplepose(type(m).__name__))
    for blk in (b for stage in m.preact.stages() for b in stage):
        if getattr(blk, "with_dcn", False):
            raise NotImplementedError(dcn)
        if not hasattr(blk, "conv3"):
            raise NotImplementedError(basic_block)


class _ConvBN:
    """Conv2d (bias-free) + BatchNorm2d(train) (+ residual) (+ ReLU)."""

    def __init__(self, ops, conv: nn.Conv2d, bn: nn.BatchNorm2d, relu: bool, need_dx: bool = True):
        if conv.bias is not None or conv.groups != 1 or conv.dilation != (1, 1) or conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1]:
            raise NotImplementedError(f"no {ops.NAME} training path for {conv}")
        ops.check_bn(bn)
        self.ops, self.conv, self.bn, self.relu, self.need_dx = ops, conv, bn, relu, need_dx
        self.cout, self.cin, self.r, self.s = conv.weight.shape
        self.stride, self.pad = conv.stride[0], conv.padding[0]
        self.w, self.wd = ops.conv_filters(self)

    def forward(self, x, skip=None):
        z = self.ops.conv(self, x)
        y, st = self.ops.bn_fwd(self.bn, z, skip, self.relu)
        self.saved = (x, z, y if self.relu else None, st, skip is not None, self.ops.conv_wd(self))
        return y

    def backward(self, dy, grads, dx_residual=None):
        """dy: gradient of the layer output -> (dx, gradient of the skip input or None); parameter gradients go to ``grads``."""
        x, z, y, st, had_skip, wd = self.saved
        self.saved = None
        dz, g = self.ops.bn_bwd(self.bn, st, dy, y, z, grads, had_skip and y is not None)
        if had_skip and y is None:
            g = dy
        grads[self.conv.weight] = self.ops.wgrad(self.conv.weight, grads, x, dz, self.cout, self.cin, self.r, self.s, self.stride, self.pad)
        dx = self.ops.dgrad(self, wd, dz, x.shape, dx_residual) if self.need_dx else None
        return dx, g


class _DeconvBN:
    """ConvTranspose2d(4,2,1, bias-free) + BatchNorm2d(train) + ReLU."""

    def __init__(self, ops, dc: nn.ConvTranspose2d, bn: nn.BatchNorm2d):
        if dc.kernel_size != (4, 4) or dc.stride != (2, 2) or dc.padding != (1, 1) or dc.output_padding != (0, 0) or dc.groups != 1 or dc.bias is not None:
            raise NotImplementedError(f"no {ops.NAME} training path for {dc}")
        ops.check_bn(bn)
        self.ops, self.dc, self.bn = ops, dc, bn
        self.cin, self.cout = dc.weight.shape[:2]
        # the data gradient is a plain 4x4 / stride 2 / pad 1 conv of dz whose "OIHW" weight is the (Cin,Cout,4,4) parameter itself
        self.w, self.wd = ops.deconv_filters(self)

    def forward(self, x):
        z = self.ops.deconv(self, x)
        y, st = self.ops.bn_fwd(self.bn, z, None, True)
        self.saved = (x, z, y, st, self.ops.deconv_wd(self))
        return y

    def backward(self, dy, grads):
        x, z, y, st, wd = self.saved
        self.saved = None
        dz, _ = self.ops.bn_bwd(self.bn, st, dy, y, z, grads, False)
        grads[self.dc.weight] = self.ops.wgrad(self.dc.weight, grads, x, dz, self.cout, self.cin, 4, 4, 2, 1, transposed=True)
        return self.ops.deconv_dgrad(self, wd, dz)


class _BottleneckT:
    def __init__(self, ops, blk):
        self.c1 = _ConvBN(ops, blk.conv1, blk.bn1, True)
        self.c2 = _ConvBN(ops, blk.conv2, blk.bn2, True)
        self.c3 = _ConvBN(ops, blk.conv3, blk.bn3, True)
        self.proj = _ConvBN(ops, blk.downsample[0], blk.downsample[1], False) if blk.downsample is not None else None

    def forward(self, x):
        skip = x if self.proj is None else self.proj.forward(x)
        return self.c3.forward(self.c2.forward(self.c1.forward(x)), skip=skip)

    def backward(self, dy, grads):
        db, g = self.c3.backward(dy, grads)                # g = dy*[y > 0]: the gradient of the skip input
        da, _ = self.c2.backward(db, grads)
        dskip = g if self.proj is None else self.proj.backward(g, grads)[0]
        return self.c1.backward(da, grads, dx_residual=dskip)[0]    # dx = dgrad(c1) + dskip in one write-out


class _HeadT:
    """Conv2d(1x1) with bias and no BatchNorm, heat-maps out as NCHW."""

    def __init__(self, ops, conv: nn.Conv2d):
        if conv.kernel_size != (1, 1) or conv.stride != (1, 1) or conv.padding != (0, 0) or (ops.HEAD_NEEDS_BIAS and conv.bias is None):
            raise NotImplementedError(f"no {ops.NAME} training path for the head {conv}")
        self.ops, self.conv = ops, conv
        self.cout, self.cin = conv.weight.shape[:2]
        self.r, self.s, self.stride, self.pad, self.need_dx = 1, 1, 1, 0, True
        self.w, self.wd = ops.head_filters(self)

    def forward(self, x):
        out, wd = self.ops.head(self, x)
        self.saved = (x, wd)
        return out

    def backward(self, dout_nchw, grads):
        x, wd = self.saved
        self.saved = None
        dy = self.ops.head_cotangent(self, x, dout_nchw, grads)       # NHWC, and the bias gradient
        grads[self.conv.weight] = self.ops.wgrad(self.conv.weight, grads, x, dy, self.cout, self.cin, 1, 1, 1, 0, side=False)
        return self.ops.dgrad(self, wd, dy, x.shape)


class SimplePoseTape:
    """Tape-based forward / backward of SimplePose in training mode; ``ops`` decides the precision."""

    def __init__(self, ops, m):
        check_model(m, *ops.REFUSALS)
        self.ops = ops
        t = m.preact
        self.stem = _ConvBN(ops, t.conv1, t.bn1, True, need_dx=False)   # the input gradient is never read
        self.blocks = [_BottleneckT(ops, b) for stage in t.stages() for b in stage]
        d = m.deconv_layers
        self.deconvs = [_DeconvBN(ops, d[0], d[1]), _DeconvBN(ops, d[3], d[4]), _DeconvBN(ops, d[6], d[7])]
        self.head = _HeadT(ops, m.final_layer)

    def trunk_forward(self, x_nchw, blocks=None):
        """Stem, max-pool and the first ``blocks`` bottlenecks (None: all) -> the last block's output, NHWC.  ``forward`` runs the whole
        trunk through it; the tests also run a shallow prefix, where rounding is not yet amplified by the depth."""
        x = self.ops.input(x_nchw)
        self.stem_y = self.stem.forward(x)
        x = self.ops.maxpool_fwd(self.stem_y)
        self.ran = self.blocks[:blocks]
        for b in self.ran:
            x = b.forward(x)
        return x

    def trunk_backward(self, dx, grads):
        """Backward of ``trunk_forward`` from the gradient of its result (NHWC); parameter gradients go to ``grads``."""
        ran, self.ran = self.ran, None
        for b in reversed(ran):
            dx = b.backward(dx, grads)
            self.ops.flush(grads)
        stem_y, self.stem_y = self.stem_y, None
        self.stem.backward(self.ops.maxpool_bwd(dx, stem_y), grads)
        self.ops.join()

    def forward(self, x_nchw):
        x = self.trunk_forward(x_nchw)
        for d in self.deconvs:
            x = d.forward(x)
        return self.head.forward(x)

    def backward(self, dout_nchw, grads):
        """The whole backward pass into ``grads`` (returned)."""
        dx = self.head.backward(dout_nchw, grads)
        for d in reversed(self.deconvs):
            dx = d.backward(dx, grads)
            self.ops.flush(grads)
        self.trunk_backward(dx, grads)
        return grads
