"""The 16-bit inference kernels (csrc/conv_h16.hip, csrc/glue_h16.hip) against torch float64 on the host, for float16 and bfloat16.

The host inputs are ALREADY rounded to the storage type T (x.to(T).double(), the same for weights and residual), so both sides
multiply the same numbers.  A product of two fp16 numbers (11 + 11 significand bits) or two bf16 numbers (8 + 8) is exact in fp32:
only the fp32 accumulation and the write-out remain as error sources, and the bound is derived from them, not tuned.  With
u = 2^-24, K = R*S*Cin and `|x| conv |w|` the same convolution of the absolute values,

    |got - ref| <= 4 * K * u * (|x| conv |w|) * |scale|  +  4 * u * (|ref| + |residual|)

plus, where the result is stored as T, half the spacing of T at |ref| (relative 2^-11 for fp16, 2^-8 for bf16, never below 2^-25
absolute for fp16).  The float64 kernel sat at <= 9.2e-2 of the same form with u = 2^-53; `worst / bound` is recorded per case.
The shapes (tests/h16_cases.py) are the smallest at which the kernel can still go wrong.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import h16_cases as HC
from tests.gpu_util import dev, record

pytestmark = pytest.mark.gpu

U = HC.U32
TYPES = list(HC.DTYPES)


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def _rs(seed):
    return np.random.RandomState(seed)


def _nhwc_t(t, dt):
    """Host NCHW float64 holding T values -> device NHWC tensor of T (exact)."""
    return t.permute(0, 2, 3, 1).contiguous().to(dt).to(dev())


def _back(y):
    """Device NHWC T -> host NCHW float64 (exact)."""
    return y.cpu().double().permute(0, 3, 1, 2)


def _fold32(rs, cout, has_bn, cb):
    """(scale, bias) in fp32, as the engine folds eval-mode BatchNorm on the device; the host reference uses these very numbers."""
    if not has_bn:
        return None, cb
    t = lambda a: torch.from_numpy(a.astype(np.float32))
    gamma, beta, mean, var = t(rs.uniform(0.5, 1.5, cout)), t(0.1 * rs.standard_normal(cout)), t(0.1 * rs.standard_normal(cout)), t(rs.uniform(0.5, 1.5, cout))
    scale = gamma / torch.sqrt(var + 1e-5)
    bias = beta - mean * scale
    return scale, bias if cb is None else bias + cb * scale


def _inputs(c, dt, seed):
    """Host tensors of a case, the 16-bit operands already rounded to T (float64 holding T values); weights fp32 holding T values."""
    rs = _rs(seed)
    x = HC.round_to(torch.from_numpy(rs.standard_normal((c["n"], c["cin"], c["h"], c["w"]))), dt)
    wt = HC.round_to(torch.from_numpy(np.sqrt(2.0 / (c["cin"] * c["r"] ** 2)) * rs.standard_normal((c["cout"], c["cin"], c["r"], c["r"]))), dt).float()
    cb = torch.from_numpy((0.1 * rs.standard_normal(c["cout"])).astype(np.float32)) if c["bias"] else None
    scale, bias = _fold32(rs, c["cout"], c["bn"], cb)
    ho, wo = (c["h"] + 2 * c["pad"] - c["r"]) // c["stride"] + 1, (c["w"] + 2 * c["pad"] - c["r"]) // c["stride"] + 1
    res = HC.round_to(torch.from_numpy(rs.standard_normal((c["n"], c["cout"], ho, wo))), dt) if c["res"] else None
    return x, wt, scale, bias, res


def _launch(vh, c, dt, x, wt, scale, bias, res, out_f32_nchw, relu=None):
    """One launch of the case; returns host NCHW float64."""
    d = lambda t: None if t is None else t.to(dev())
    xd = vh.nchw_to_nhwc_h16(x.float().to(dev()), dt) if c["via_converter"] else _nhwc_t(x, dt)       # the stem: 3 channels padded to 8 by the converter
    got = vh.conv2d_fwd_h16(xd, vh.pack_conv_weight_h16(wt.to(dev()), dt), d(scale), d(bias), c["stride"], c["pad"], c["relu"] if relu is None else relu,
                            residual=None if res is None else _nhwc_t(res, dt), out_f32_nchw=out_f32_nchw)
    torch.cuda.synchronize()
    assert got.dtype == (torch.float32 if out_f32_nchw else dt)
    return got.cpu().double() if out_f32_nchw else _back(got)


def _t_rounding(ref, tname):
    _, _, half_rel, half_abs = HC.DTYPES[tname]
    return (half_rel * ref.abs()).clamp_min(half_abs)


def _check(name, got, ref, bound):
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    record(f"conv_h16_{name}", max_abs=float(err.max()), worst_over_bound=worst, ref_absmax=float(ref.abs().max()))
    print(f"{name}: max |got - ref| {float(err.max()):.3e}, worst error / bound {worst:.3e}")
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (name, float(err.max()), worst)


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("name,out_nchw", [(k, False) for k, c in HC.CONV_CASES.items() if c["t_out"]] + [(k, True) for k in HC.NCHW_CASES])
def test_conv_against_host_float64(vh, name, out_nchw, tname):
    c, dt = HC.CONV_CASES[name], HC.DTYPES[tname][0]
    x, wt, scale, bias, res = _inputs(c, dt, 11)
    s64 = torch.ones(c["cout"], dtype=torch.float64) if scale is None else scale.double()
    z = F.conv2d(x, wt.double(), None, c["stride"], c["pad"])
    ref = z * s64.view(1, -1, 1, 1) + (0.0 if bias is None else bias.double().view(1, -1, 1, 1))
    bound = 4 * c["cin"] * c["r"] ** 2 * U * F.conv2d(x.abs(), wt.double().abs(), None, c["stride"], c["pad"]) * s64.abs().view(1, -1, 1, 1)
    if res is not None:
        ref = ref + res
    bound = bound + 4 * U * (ref.abs() + (0.0 if res is None else res.abs()))
    if c["relu"]:
        ref = ref.relu()
    if not out_nchw:
        bound = bound + _t_rounding(ref, tname)
    got = _launch(vh, c, dt, x, wt, scale, bias, res, out_nchw)
    assert got.shape == ref.shape
    _check(f"{name}_{tname}" + ("_nchw" if out_nchw else ""), got, ref, bound)


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("name", list(HC.DECONV_CASES))
def test_transposed_conv_against_host_float64(vh, name, tname):
    """ConvTranspose2d(4, 2, 1), 8 -> 8 channels: on 3x2 and on 1x1 planes every one of the four output phases has clipped taps."""
    n, cin, cout, h, w = HC.DECONV_CASES[name]
    dt = HC.DTYPES[tname][0]
    rs = _rs(23)
    x = HC.round_to(torch.from_numpy(rs.standard_normal((n, cin, h, w))), dt)
    wt = HC.round_to(torch.from_numpy(np.sqrt(2.0 / cin) * rs.standard_normal((cin, cout, 4, 4))), dt).float()
    scale, bias = _fold32(rs, cout, True, None)
    z = F.conv_transpose2d(x, wt.double(), None, 2, 1)
    pre = z * scale.double().view(1, -1, 1, 1) + bias.double().view(1, -1, 1, 1)
    ref = pre.relu()
    bound = 4 * (4 * cin) * U * F.conv_transpose2d(x.abs(), wt.double().abs(), None, 2, 1) * scale.double().abs().view(1, -1, 1, 1)     # K = 2x2 taps x Cin per output
    bound = bound + 4 * U * pre.abs() + _t_rounding(ref, tname)
    got = vh.deconv4x4s2_fwd_h16(_nhwc_t(x, dt), vh.pack_deconv_weight_h16(wt.to(dev()), dt), scale.to(dev()), bias.to(dev()), True)
    torch.cuda.synchronize()
    assert got.dtype == dt
    got = _back(got)
    assert got.shape == ref.shape == (n, cout, 2 * h, 2 * w)
    _check(f"{name}_{tname}", got, ref, bound)


# ------------------------------------------------------------------------------------------------------------------------ exact
def _int_inputs(c, seed):
    rs = _rs(seed)
    x = torch.from_numpy(rs.randint(-4, 5, (c["n"], c["cin"], c["h"], c["w"])).astype(np.float64))
    wt = torch.from_numpy(rs.randint(-1, 2, (c["cout"], c["cin"], c["r"], c["r"])).astype(np.float32))
    bias = torch.from_numpy(rs.randint(-3, 4, c["cout"]).astype(np.float32))
    ho, wo = (c["h"] + 2 * c["pad"] - c["r"]) // c["stride"] + 1, (c["w"] + 2 * c["pad"] - c["r"]) // c["stride"] + 1
    res = torch.from_numpy(rs.randint(-4, 5, (c["n"], c["cout"], ho, wo)).astype(np.float64)) if c["res"] else None
    return x, wt, bias, res


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("name", HC.EXACT_CASES)
def test_integer_data_is_exact(vh, name, tname):
    """x integers in [-4, 4], w in {-1, 0, 1}, no scale, integer bias (and residual), fp32 NCHW write-out: every operand is a T value and
    every partial sum an integer below 2^24, so the result must EQUAL the host's.  Any indexing, padding or lane-map mistake is a wrong integer."""
    c, dt = HC.CONV_CASES[name], HC.DTYPES[tname][0]
    x, wt, bias, res = _int_inputs(c, 17)
    ref = F.conv2d(x, wt.double(), bias.double(), c["stride"], c["pad"])
    if res is not None:
        ref = ref + res
    if c["relu"]:
        ref = ref.relu()
    assert float(ref.abs().max()) < 2 ** 24 and c["cin"] * c["r"] ** 2 * 4 + 7 < 2 ** 24
    got = _launch(vh, c, dt, x, wt, None, bias, res, True)
    assert torch.equal(got.float(), ref.float()), (name, float((got - ref).abs().max()))


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("name", list(HC.DECONV_CASES))
def test_integer_data_is_exact_transposed(vh, name, tname):
    """The four phases on integer data.  The transposed conv writes T only: |result| <= 4 * 4 * 8 + 3 = 131 is an integer both types hold exactly."""
    n, cin, cout, h, w = HC.DECONV_CASES[name]
    dt = HC.DTYPES[tname][0]
    rs = _rs(19)
    x = torch.from_numpy(rs.randint(-4, 5, (n, cin, h, w)).astype(np.float64))
    wt = torch.from_numpy(rs.randint(-1, 2, (cin, cout, 4, 4)).astype(np.float32))
    bias = torch.from_numpy(rs.randint(-3, 4, cout).astype(np.float32))
    ref = F.conv_transpose2d(x, wt.double(), bias.double(), 2, 1)
    got = _back(vh.deconv4x4s2_fwd_h16(_nhwc_t(x, dt), vh.pack_deconv_weight_h16(wt.to(dev()), dt), None, bias.to(dev()), False))
    assert float(ref.abs().max()) <= 131 and torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("name", ["stem7x7s2_3to64_9x7", "3x3_512to16_2x2", "3x3_8to8_6x5_n11"])
def test_two_calls_give_the_same_bits(vh, name, tname):
    c, dt = HC.CONV_CASES[name], HC.DTYPES[tname][0]
    ins = _inputs(c, dt, 5)
    assert torch.equal(_launch(vh, c, dt, *ins, False), _launch(vh, c, dt, *ins, False))
    rs = _rs(6)
    x = _nhwc_t(torch.from_numpy(rs.standard_normal((2, 8, 3, 2))), dt)
    wd = vh.pack_deconv_weight_h16(torch.from_numpy(rs.standard_normal((8, 8, 4, 4)).astype(np.float32)).to(dev()), dt)
    assert torch.equal(vh.deconv4x4s2_fwd_h16(x, wd, None, None, False), vh.deconv4x4s2_fwd_h16(x, wd, None, None, False))


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("crop", [0, 2, 10])
def test_a_crops_bits_do_not_depend_on_its_batch(vh, crop, tname):
    """3x3, 8 -> 8 on 6x5 planes: in the N = 11 call (M = 330) crop 2 straddles the end of the first 64-pixel span, crop 10 ends the last,
    partial tile; alone each starts a tile.  Both write-outs."""
    c, dt = HC.CONV_CASES["3x3_8to8_6x5_n11"], HC.DTYPES[tname][0]
    x, wt, scale, bias, res = _inputs(c, dt, 7)
    one = dict(c, n=1)
    for nchw in (False, True):
        whole = _launch(vh, c, dt, x, wt, scale, bias, res, nchw)
        alone = _launch(vh, one, dt, x[crop:crop + 1], wt, scale, bias, res[crop:crop + 1], nchw)
        assert torch.equal(whole[crop:crop + 1], alone)


# -------------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("name", list(HC.REFUSED_CASES))
def test_shapes_outside_the_contract_are_refused(vh, name, tname):
    """Cin = 12, and Cout = 17 with a 16-bit output, at the C ABI itself: a non-zero status, an error text, and `y` untouched."""
    c = HC.REFUSED_CASES[name]
    dt, code = HC.DTYPES[tname][:2]
    x = torch.zeros((1, 3, 3, c["cin"]), dtype=dt, device=dev())
    w = torch.zeros((c["cout"], 1, 1, c["cin"]), dtype=dt, device=dev())
    y = torch.full((1, 3, 3, 32), 7.0, dtype=dt, device=dev())
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = vh.lib().vatl_conv2d_fwd_h16(p(x), p(w), None, None, None, p(y), 1, 3, 3, c["cin"], c["cout"], 1, 1, 1, 0, 0, 0, code, None)
    torch.cuda.synchronize()
    assert rc != 0 and b"multiple of 8" in vh.lib().vatl_last_error()
    assert bool((y == 7.0).all())
    if name == "cout17_t_out":                           # the fp32 NCHW write-out does serve 17 channels
        yf = torch.empty((1, 17, 3, 3), device=dev())
        assert vh.lib().vatl_conv2d_fwd_h16(p(x), p(w), None, None, None, p(yf), 1, 3, 3, c["cin"], c["cout"], 1, 1, 1, 0, 0, 1, code, None) == 0
        torch.cuda.synchronize()
        assert bool((yf == 0).all())
    with pytest.raises(vh.VatlError):                    # and a dtype the route does not have
        vh.nchw_to_nhwc_h16(torch.zeros((1, 3, 2, 2), device=dev()), torch.float32)
    with pytest.raises(vh.VatlError):                    # CPU tensors
        vh.maxpool3x3s2_fwd_h16(torch.zeros((1, 3, 3, 8), dtype=dt))


# ------------------------------------------------------------------------------------------------------------------------- glue
@pytest.mark.parametrize("tname", TYPES)
def test_converter_pads_with_exact_zeros_and_rounds_like_torch(vh, tname):
    dt = HC.DTYPES[tname][0]
    rs = _rs(31)
    for ch in (3, 8, 20):
        x = torch.from_numpy(rs.standard_normal((2, ch, 5, 7)).astype(np.float32))
        x[0, 0, 0, 0], x[0, 0, 0, 1] = 70000.0, 1e-7                                         # beyond fp16's range: inf, as torch rounds; and a subnormal
        y = vh.nchw_to_nhwc_h16(x.to(dev()), dt).cpu()
        c8 = (ch + 7) // 8 * 8
        assert y.dtype == dt and y.shape == (2, 5, 7, c8)
        assert torch.equal(y[..., :ch], x.to(dt).permute(0, 2, 3, 1))
        assert bool((y[..., ch:].view(torch.int16) == 0).all())                              # +0.0 bit patterns
    for h, w, ch in HC.GLUE_PLANES:                                                          # and back to fp32 NCHW: exact
        t = torch.from_numpy(rs.standard_normal((2, ch, h, w))).to(dt)
        back = vh.nhwc_to_nchw_h16(t.permute(0, 2, 3, 1).contiguous().to(dev())).cpu()
        assert back.dtype == torch.float32 and torch.equal(back, t.float())


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("h,w,ch", HC.GLUE_PLANES)
def test_moves_and_maxima_are_exact(vh, tname, h, w, ch):
    """MaxPool2d(3,2,1) on odd planes (border windows on every side) and PixelShuffle(2): the results are input values."""
    dt = HC.DTYPES[tname][0]
    x = HC.round_to(torch.from_numpy(_rs(32).standard_normal((2, ch, h, w))), dt)
    got = _back(vh.maxpool3x3s2_fwd_h16(_nhwc_t(x, dt)))
    ref = F.max_pool2d(x, 3, 2, 1)
    assert got.shape == ref.shape == (2, ch, 3, 4) and torch.equal(got, ref)
    got = _back(vh.pixelshuffle2_fwd_h16(_nhwc_t(x, dt)))
    ref = F.pixel_shuffle(x, 2)
    assert got.shape == ref.shape == (2, ch // 4, 2 * h, 2 * w) and torch.equal(got, ref)


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("h,w,ch", HC.GLUE_PLANES)
def test_global_average_pool_sums_in_fp32(vh, tname, h, w, ch):
    """fp32 out.  HW - 1 fp32 additions of exactly converted T values and one division: (HW + 1) * u * sum|x| / HW bounds any order."""
    dt = HC.DTYPES[tname][0]
    x = HC.round_to(torch.from_numpy(_rs(33).standard_normal((3, ch, h, w))), dt)
    got = vh.gap_fwd_h16(_nhwc_t(x, dt)).cpu()
    assert got.dtype == torch.float32 and got.shape == (3, ch)
    assert ((got.double() - x.mean(dim=(2, 3))).abs() <= (h * w + 1) * U * x.abs().mean(dim=(2, 3))).all()
    ints = torch.from_numpy(_rs(34).randint(-8, 9, (3, ch, h, w)).astype(np.float64))        # exact sums in any order: the division alone rounds (2 u: faithful)
    got = vh.gap_fwd_h16(_nhwc_t(ints, dt)).cpu()
    assert ((got.double() - ints.mean(dim=(2, 3))).abs() <= 2 * U * ints.mean(dim=(2, 3)).abs()).all()


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("ch", [8, 24])
@pytest.mark.parametrize("relu", [False, True])
def test_nearest_upsampling_and_add(vh, tname, ch, relu):
    """Three sources at 2x, 4x, 8x below an 8x8 plane (the up-sampling needs divisible extents), summed in fp32 in argument order and rounded
    once: three fp32 additions (3 u on the partial sums, bounded by the sum of the absolute terms) and half a spacing of T."""
    dt = HC.DTYPES[tname][0]
    rs = _rs(35)
    base = HC.round_to(torch.from_numpy(rs.standard_normal((2, ch, 8, 8))), dt)
    zs = [HC.round_to(torch.from_numpy(rs.standard_normal((2, ch, 8 >> s, 8 >> s))), dt) for s in (1, 2, 3)]
    ref, mag = base, base.abs()
    for s, z in zip((1, 2, 3), zs):
        up = F.interpolate(z, scale_factor=2 ** s, mode="nearest")
        ref, mag = ref + up, mag + up.abs()
    ref = ref.relu() if relu else ref
    got = _back(vh.fuse_upsample_add_h16(_nhwc_t(base, dt), [(_nhwc_t(z, dt), s) for s, z in zip((1, 2, 3), zs)], relu))
    assert ((got - ref).abs() <= 4 * U * mag + _t_rounding(ref, tname)).all()
    one = _back(vh.fuse_upsample_add_h16(_nhwc_t(base, dt), [(_nhwc_t(zs[1], dt), 2)], relu))
    ref1 = base + F.interpolate(zs[1], scale_factor=4, mode="nearest")
    ref1 = ref1.relu() if relu else ref1
    assert ((one - ref1).abs() <= 4 * U * (base.abs() + ref1.abs()) + _t_rounding(ref1, tname)).all()


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("h,w,ch", HC.GLUE_PLANES)
def test_se_gate_skip_relu(vh, tname, h, w, ch):
    """y = relu(x * sigmoid(g) + skip), g in fp32, computed in fp32 and rounded once.  The fp32 side rounds the exponential, the division,
    the product and the sum: 16 u (|x| + |skip|) covers them (the float64 test uses the same count); then half a spacing of T."""
    dt = HC.DTYPES[tname][0]
    rs = _rs(36)
    x, skip = (HC.round_to(torch.from_numpy(rs.standard_normal((3, ch, h, w))), dt) for _ in range(2))
    g = torch.from_numpy((3.0 * rs.standard_normal((3, ch))).astype(np.float32))
    got = _back(vh.se_scale_add_relu_h16(_nhwc_t(x, dt), g.to(dev()), _nhwc_t(skip, dt)))
    ref = (x * torch.sigmoid(g.double())[:, :, None, None] + skip).relu()
    assert ((got - ref).abs() <= 16 * U * (x.abs() + skip.abs()) + _t_rounding(ref, tname)).all()
