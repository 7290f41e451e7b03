"""The float64 reference kernels (csrc/conv_f64.hip, csrc/glue_f64.hip) against torch float64 on the host.

The bound on a convolution is derived, not tuned.  Both sides sum the same K = R*S*Cin products of float64 numbers, in different
orders; the folded BatchNorm multiplies by `scale` and adds `bias`.  Element-wise

    |got - ref| <= 4 * K * 2^-53 * (|x| conv |w|) * |scale|        (+ 4 * 2^-53 * |residual| for the residual's one addition)

where `|x| conv |w|` is the same convolution of the absolute values, computed here: no difference of summation order can exceed it,
and a single fp32 operation anywhere (2^-24 instead of 2^-53) exceeds it by six orders.  The shapes are the smallest at which the
kernel can still go wrong: K that is no multiple of the k-tile, partial tiles in pixels and channels, tiles that straddle images,
odd and even extents under stride 2, single pixels, the longest K of the networks.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import dev, record

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def _rs(seed):
    return np.random.RandomState(seed)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(dev())


def _bn(r, c):
    """fp32 eval-mode BatchNorm parameters as the modules hold them."""
    t = lambda a: torch.from_numpy(a.astype(np.float32))
    return {"gamma": t(r.uniform(0.5, 1.5, c)), "beta": t(0.1 * r.standard_normal(c)), "mean": t(0.1 * r.standard_normal(c)),
            "var": t(r.uniform(0.5, 1.5, c)), "eps": 1e-5}


def _fold(bn, conv_bias, c):
    """The fold the engine computes: float64 from the fp32 parameters."""
    cb = None if conv_bias is None else conv_bias.double()
    if bn is None:
        return (None, None) if cb is None else (torch.ones(c, dtype=torch.float64), cb)
    scale = bn["gamma"].double() / torch.sqrt(bn["var"].double() + bn["eps"])
    bias = bn["beta"].double() - bn["mean"].double() * scale
    return scale, bias if cb is None else bias + cb * scale


def _host(z, bn):
    return z if bn is None else F.batch_norm(z, bn["mean"].double(), bn["var"].double(), bn["gamma"].double(), bn["beta"].double(), False, 0.0, bn["eps"])


def _check(name, got, ref, bound):
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    record(f"conv_f64_{name}", max_abs=float(err.max()), worst_over_bound=worst, ref_absmax=float(ref.abs().max()))
    print(f"{name}: max |got - ref| {float(err.max()):.3e}, worst error / bound {worst:.3e}")
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (name, float(err.max()), worst)


CONV_CASES = {   # name: (N, Cin, Cout, H, W, R, stride, pad, batch norm, conv bias, residual, relu)
    "stem7x7s2_3to64_9x7": (2, 3, 64, 9, 7, 7, 2, 3, True, False, False, True),            # K = 147: no multiple of 4 or 16, odd planes
    "3x3_16to17_5x3_n3": (3, 16, 17, 5, 3, 3, 1, 1, True, False, False, False),            # M = 45: partial tile in pixels and in channels
    "3x3s2_8to24_6x4": (2, 8, 24, 6, 4, 3, 2, 1, True, False, False, True),                # even extent under stride 2
    "3x3s2_8to24_7x5": (2, 8, 24, 7, 5, 3, 2, 1, True, False, False, True),                # odd extent under stride 2
    "1x1s2_8to32_5x5": (2, 8, 32, 5, 5, 1, 2, 0, True, False, False, False),               # projection shortcut: every other pixel
    "1x1_32to32_1x1_res_relu": (1, 32, 32, 1, 1, 1, 1, 0, True, False, True, True),        # one output pixel: the shape of an SE Linear
    "3x3_512to16_2x2": (2, 512, 16, 2, 2, 3, 1, 1, True, False, False, False),             # K = 4608: the longest K of the networks
    "3x3_8to8_4x4_n5": (5, 8, 8, 4, 4, 3, 1, 1, True, False, True, True),                  # M = 80: a tile straddles images
    "head1x1_16to17_bias": (2, 16, 17, 6, 5, 1, 1, 0, False, True, False, False),          # conv bias, no BatchNorm
}


def _conv_inputs(case, seed):
    n, cin, cout, h, w, r, stride, pad, has_bn, has_bias, has_res, relu = case
    rs = _rs(seed)
    x = torch.from_numpy(rs.standard_normal((n, cin, h, w)))                               # float64 values fp32 cannot hold
    wt = torch.from_numpy((np.sqrt(2.0 / (cin * r * r)) * rs.standard_normal((cout, cin, r, r))).astype(np.float32))
    bn = _bn(rs, cout) if has_bn else None
    cb = torch.from_numpy((0.1 * rs.standard_normal(cout)).astype(np.float32)) if has_bias else None
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1
    res = torch.from_numpy(rs.standard_normal((n, cout, ho, wo))) if has_res else None
    return x, wt, bn, cb, res


# every case NHWC; the NCHW write-out (the heads': no residual there) on the head and on the two cases with partial tiles
@pytest.mark.parametrize("name,out_nchw", [(k, False) for k in CONV_CASES] + [(k, True) for k in ("head1x1_16to17_bias", "3x3_16to17_5x3_n3", "stem7x7s2_3to64_9x7")])
def test_conv_against_host_float64(vh, name, out_nchw):
    case = CONV_CASES[name]
    n, cin, cout, h, w, r, stride, pad, has_bn, has_bias, has_res, relu = case
    x, wt, bn, cb, res = _conv_inputs(case, 11)
    ref = _host(F.conv2d(x, wt.double(), None if cb is None else cb.double(), stride, pad), bn)
    scale, bias = _fold(bn, cb, cout)
    bound = 4 * cin * r * r * U * F.conv2d(x.abs(), wt.double().abs(), None, stride, pad) * (1.0 if scale is None else scale.abs().view(1, -1, 1, 1))
    if res is not None:
        ref = ref + res
        bound = bound + 4 * U * res.abs()
    if relu:
        ref = ref.relu()
    d = lambda t: None if t is None else t.to(dev())
    got = vh.conv2d_fwd_f64(_nhwc(x), vh.pack_conv_weight_f64(wt.to(dev())), d(scale), d(bias), stride, pad, relu,
                            residual=None if res is None else _nhwc(res), out_nchw=out_nchw)
    torch.cuda.synchronize()
    got = got.cpu() if out_nchw else got.cpu().permute(0, 3, 1, 2)
    assert got.shape == ref.shape
    _check(name + ("_nchw" if out_nchw else ""), got, ref, bound)


@pytest.mark.parametrize("hw", [(3, 2), (1, 1)])
def test_transposed_conv_against_host_float64(vh, hw):
    """ConvTranspose2d(4, 2, 1), 8 -> 5 channels: on 3x2 and on 1x1 planes every one of the four output phases has clipped taps."""
    n, cin, cout = 2, 8, 5
    rs = _rs(23)
    x = torch.from_numpy(rs.standard_normal((n, cin) + hw))
    wt = torch.from_numpy((np.sqrt(2.0 / cin) * rs.standard_normal((cin, cout, 4, 4))).astype(np.float32))
    bn = _bn(rs, cout)
    ref = _host(F.conv_transpose2d(x, wt.double(), None, 2, 1), bn).relu()
    scale, bias = _fold(bn, None, cout)
    bound = 4 * (4 * cin) * U * F.conv_transpose2d(x.abs(), wt.double().abs(), None, 2, 1) * scale.abs().view(1, -1, 1, 1)     # K = 2x2 taps x Cin per output
    got = vh.deconv4x4s2_fwd_f64(_nhwc(x), vh.pack_deconv_weight_f64(wt.to(dev())), scale.to(dev()), bias.to(dev()), True)
    torch.cuda.synchronize()
    got = got.cpu().permute(0, 3, 1, 2)
    assert got.shape == ref.shape == (n, cout, 2 * hw[0], 2 * hw[1])
    _check(f"deconv_{hw[0]}x{hw[1]}", got, ref, bound)


def _run(vh, case, x, wt, bn, cb, res):
    n, cin, cout, h, w, r, stride, pad, has_bn, has_bias, has_res, relu = case
    scale, bias = _fold(bn, cb, cout)
    d = lambda t: None if t is None else t.to(dev())
    return vh.conv2d_fwd_f64(_nhwc(x), vh.pack_conv_weight_f64(wt.to(dev())), d(scale), d(bias), stride, pad, relu, residual=None if res is None else _nhwc(res))


@pytest.mark.parametrize("name", ["stem7x7s2_3to64_9x7", "3x3_512to16_2x2", "3x3_8to8_4x4_n5"])
def test_two_calls_give_the_same_bits(vh, name):
    ins = _conv_inputs(CONV_CASES[name], 5)
    a, b = _run(vh, CONV_CASES[name], *ins), _run(vh, CONV_CASES[name], *ins)
    assert torch.equal(a, b)
    rs = _rs(6)
    x = _nhwc(torch.from_numpy(rs.standard_normal((2, 8, 3, 2))))
    wd = vh.pack_deconv_weight_f64(torch.from_numpy(rs.standard_normal((8, 5, 4, 4)).astype(np.float32)).to(dev()))
    assert torch.equal(vh.deconv4x4s2_fwd_f64(x, wd, None, None, False), vh.deconv4x4s2_fwd_f64(x, wd, None, None, False))


@pytest.mark.parametrize("crop", [0, 3])
def test_a_crops_bits_do_not_depend_on_its_batch(vh, crop):
    """3x3, 8 -> 8 on 4x4 planes: in the N = 5 call (M = 80) crop 3 straddles the first tile's end; alone it starts a tile."""
    case = CONV_CASES["3x3_8to8_4x4_n5"]
    x, wt, bn, cb, res = _conv_inputs(case, 7)
    whole = _run(vh, case, x, wt, bn, cb, res)
    alone = _run(vh, (1,) + case[1:], x[crop:crop + 1], wt, bn, cb, res[crop:crop + 1])
    assert torch.equal(whole[crop:crop + 1], alone)


# ------------------------------------------------------------------------------------------------------------------------- glue
def _close15(got, ref):
    """1e-15 relative: these are exact, or a short sum."""
    return float((got - ref).abs().max()) <= 1e-15 * float(ref.abs().max())


def test_layout_changes_are_exact(vh):
    rs = _rs(31)
    x32 = torch.from_numpy(rs.standard_normal((3, 3, 5, 7)).astype(np.float32))
    x64 = torch.from_numpy(rs.standard_normal((2, 5, 3, 4)))
    assert torch.equal(vh.nchw_to_nhwc_f64(x32.to(dev())).cpu(), x32.double().permute(0, 2, 3, 1))
    y = vh.nchw_to_nhwc_f64(x64.to(dev()))
    assert torch.equal(y.cpu(), x64.permute(0, 2, 3, 1))
    assert torch.equal(vh.nhwc_to_nchw_f64(y).cpu(), x64)


def test_maxpool_on_odd_planes(vh):
    x = torch.from_numpy(_rs(32).standard_normal((2, 7, 5, 7)))                             # 5x7 planes: border windows on every side, C = 7
    got = vh.maxpool3x3s2_fwd_f64(_nhwc(x)).cpu().permute(0, 3, 1, 2)
    ref = F.max_pool2d(x, 3, 2, 1)
    assert got.shape == ref.shape == (2, 7, 3, 4) and _close15(got, ref)


def test_global_average_pool(vh):
    """Multiples of 2^-10: the sum over the 35 pixels is exact in any order, so the two sides differ by the rounding of one division at most."""
    x = torch.from_numpy(_rs(33).randint(-4096, 4097, (3, 7, 5, 7)).astype(np.float64) / 1024.0)
    got = vh.gap_fwd_f64(_nhwc(x)).cpu()
    ref = x.mean(dim=(2, 3))
    assert got.shape == ref.shape and _close15(got, ref)


def test_pixelshuffle(vh):
    x = torch.from_numpy(_rs(34).standard_normal((2, 12, 3, 5)))
    got = vh.pixelshuffle2_fwd_f64(_nhwc(x)).cpu().permute(0, 3, 1, 2)
    ref = F.pixel_shuffle(x, 2)
    assert got.shape == ref.shape and _close15(got, ref)


@pytest.mark.parametrize("relu", [False, True])
def test_nearest_upsampling_and_add(vh, relu):
    """Three sources at 2x, 4x, 8x below an 8x8 plane with 5 channels, added in argument order like the host sum below."""
    rs = _rs(35)
    base = torch.from_numpy(rs.standard_normal((2, 5, 8, 8)))
    zs = [torch.from_numpy(rs.standard_normal((2, 5, 8 >> s, 8 >> s))) for s in (1, 2, 3)]
    ref = base
    for s, z in zip((1, 2, 3), zs):
        ref = ref + F.interpolate(z, scale_factor=2 ** s, mode="nearest")
    ref = ref.relu() if relu else ref
    got = vh.fuse_upsample_add_f64(_nhwc(base), [(_nhwc(z), s) for s, z in zip((1, 2, 3), zs)], relu).cpu().permute(0, 3, 1, 2)
    assert _close15(got, ref)
    one = vh.fuse_upsample_add_f64(_nhwc(base), [(_nhwc(zs[1]), 2)], relu).cpu().permute(0, 3, 1, 2)
    ref1 = base + F.interpolate(zs[1], scale_factor=4, mode="nearest")
    assert _close15(one, ref1.relu() if relu else ref1)


def test_se_gate_skip_relu(vh):
    """y = relu(x * sigmoid(g) + skip).  Each side rounds the exponential, the division, the product and the sum once or fuses the last
    two: at most a handful of 2^-53 relative steps on |x| * sigmoid <= |x| and on |skip| — 16 * 2^-53 * (|x| + |skip|) covers both sides."""
    rs = _rs(36)
    x, skip = torch.from_numpy(rs.standard_normal((3, 6, 3, 5))), torch.from_numpy(rs.standard_normal((3, 6, 3, 5)))
    g = torch.from_numpy(3.0 * rs.standard_normal((3, 6)))
    got = vh.se_scale_add_relu_f64(_nhwc(x), g.to(dev()), _nhwc(skip)).cpu().permute(0, 3, 1, 2)
    ref = (x * torch.sigmoid(g)[:, :, None, None] + skip).relu()
    assert ((got - ref).abs() <= 16 * U * (x.abs() + skip.abs())).all()
