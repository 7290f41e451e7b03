"""The 16-bit data gradient (vatl_conv2d_dgrad_h16 + vatl_pack_conv_weight_dgrad_h16: launch logic on the inference kernel of
csrc/conv_h16.hip) against float64 `conv_transpose2d` on the host, for float16 and bfloat16, with and without a residual.

Exact: integer operands in [-2, 2]; every sum is an integer far below 2^24, so the fp32 accumulator holds it exactly and the stored
result must be BIT-equal to the float64 result rounded once to T.  Random: operands already rounded to T; with u = 2^-24 and
K = R*S*Cout8 the bound is the forward kernel's (tests/test_gpu_conv_h16.py), 4*K*u*(|dz| convT |w|) + 4*u*(|ref| + |residual|), plus half
the spacing of T at |ref|.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import h16_cases as HC
from tests import train_h16_cases as TC
from tests.gpu_util import dev, record

pytestmark = pytest.mark.gpu

U = HC.U32
TYPES = list(HC.DTYPES)


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def _nhwc_t(t, dt, pad_to=None):
    t = t.permute(0, 2, 3, 1)
    if pad_to is not None and pad_to != t.shape[-1]:
        t = torch.cat([t, torch.zeros(*t.shape[:-1], pad_to - t.shape[-1], dtype=t.dtype)], dim=-1)
    return t.contiguous().to(dt).to(dev())


def _back(y):
    return y.cpu().double().permute(0, 3, 1, 2)


def _t_rounding(ref, tname):
    _, _, half_rel, half_abs = HC.DTYPES[tname]
    return (half_rel * ref.abs()).clamp_min(half_abs)


def _operands(case, dt, exact, with_res, seed):
    n, cin, cout, h, w, r, stride, pad = case
    rs = np.random.RandomState(seed)
    ho, wo = TC.out_size(h, r, stride, pad), TC.out_size(w, r, stride, pad)
    if exact:
        gen = lambda *s: torch.from_numpy(rs.randint(-2, 3, s).astype(np.float64))
        dz, wt, res = gen(n, cout, ho, wo), gen(cout, cin, r, r), gen(n, cin, h, w)
    else:
        gen = lambda sc, *s: HC.round_to(torch.from_numpy(sc * rs.standard_normal(s)), dt)
        dz, wt, res = gen(1.0, n, cout, ho, wo), gen(np.sqrt(2.0 / (cout * r * r)), cout, cin, r, r), gen(1.0, n, cin, h, w)
    return dz, wt, (res if with_res else None)


def _run(vh, case, dt, dz, wt, res):
    n, cin, cout, h, w, r, stride, pad = case
    cin8, cout8 = (cin + 7) // 8 * 8, (cout + 7) // 8 * 8
    wd = vh.pack_conv_weight_dgrad_h16(wt.float().to(dev()), stride, pad, dt)
    assert wd.numel() == cin8 * r * r * cout8
    got = vh.conv2d_dgrad_h16(_nhwc_t(dz, dt, cout8), wd, (n, h, w, cin8), r, r, stride, pad, residual=None if res is None else _nhwc_t(res, dt, cin8))
    torch.cuda.synchronize()
    assert got.dtype == dt and tuple(got.shape) == (n, h, w, cin8)
    return got


def _ref(case, dz, wt, res):
    n, cin, cout, h, w, r, stride, pad = case
    opad = (h + 2 * pad - r) % stride, (w + 2 * pad - r) % stride          # input rows / columns the strided conv never read
    ref = F.conv_transpose2d(dz, wt, None, stride, pad, output_padding=opad)
    assert tuple(ref.shape) == (n, cin, h, w)
    return ref if res is None else ref + res


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("name", list(TC.DGRAD_CASES))
def test_dgrad_exact_on_small_integers(vh, name, with_res, tname):
    case, dt = TC.DGRAD_CASES[name], HC.DTYPES[tname][0]
    dz, wt, res = _operands(case, dt, True, with_res, 3)
    ref = HC.round_to(_ref(case, dz, wt, res), dt)
    got = _back(_run(vh, case, dt, dz, wt, res))[:, :case[1]]
    bad = int((got != ref).sum())
    record(f"dgrad_h16_exact_{name}_{tname}_{'res' if with_res else 'nores'}", mismatches=bad)
    assert bad == 0, (name, bad, float((got - ref).abs().max()))


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("name", list(TC.DGRAD_CASES))
def test_dgrad_against_host_float64(vh, name, with_res, tname):
    case, dt = TC.DGRAD_CASES[name], HC.DTYPES[tname][0]
    n, cin, cout, h, w, r, stride, pad = case
    dz, wt, res = _operands(case, dt, False, with_res, 19)
    ref = _ref(case, dz, wt, res)
    k = r * r * ((cout + 7) // 8 * 8)
    bound = 4 * k * U * _ref(case, dz.abs(), wt.abs(), None) + 4 * U * (ref.abs() + (0.0 if res is None else res.abs())) + _t_rounding(ref, tname)
    full = _back(_run(vh, case, dt, dz, wt, res))
    got = full[:, :cin]
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    record(f"dgrad_h16_{name}_{tname}_{'res' if with_res else 'nores'}", max_abs=float(err.max()), worst_over_bound=worst)
    assert torch.isfinite(full).all()
    assert (err <= bound).all(), (name, float(err.max()), worst)


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("with_res", [False, True])
def test_1x1_stride2_odd_pixels_are_the_residual_or_plus_zero(vh, with_res, tname):
    """The 1x1 / stride 2 data gradient reaches the even pixels only; the other three quarters of dx are defined all the same: the
    residual exactly, or +0.0 (sign bit clear) without one."""
    case, dt = TC.DGRAD_CASES["1x1s2_8to32_5x5"], HC.DTYPES[tname][0]
    dz, wt, res = _operands(case, dt, False, with_res, 41)
    got = _run(vh, case, dt, dz, wt, res)                               # (N,H,W,C) T
    odd = torch.ones(case[3], case[4], dtype=torch.bool)
    odd[::2, ::2] = False
    bits = got.view(torch.int16).cpu()[:, odd]
    if with_res:
        want = res.permute(0, 2, 3, 1).to(dt).view(torch.int16)[:, odd]
        assert torch.equal(bits, want)
    else:
        assert int(bits.ne(0).sum()) == 0
    assert bool(_back(got)[:, :, ::2, ::2].abs().sum() > 0)


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("regime", ["exact", "random"])
def test_transposed_conv_dgrad(vh, regime, with_res, tname):
    """The data gradient of ConvTranspose2d(4,2,1) is the plain 4x4 / stride 2 / pad 1 conv of dz with the (Cin,Cout,4,4) parameter read as
    an OIHW filter: vatl_pack_conv_weight_h16 with the two counts exchanged + vatl_conv2d_fwd_h16."""
    n, cin, cout, h, w = TC.DGRAD_DECONV_CASE
    dt = HC.DTYPES[tname][0]
    rs = np.random.RandomState(43)
    if regime == "exact":
        gen = lambda *s: torch.from_numpy(rs.randint(-2, 3, s).astype(np.float64))
    else:
        gen = lambda *s: HC.round_to(torch.from_numpy(rs.standard_normal(s)), dt)
    dy, wt, res = gen(n, cout, 2 * h, 2 * w), gen(cin, cout, 4, 4), (gen(n, cin, h, w) if with_res else None)
    ref = F.conv2d(dy, wt, None, 2, 1)
    if res is not None:
        ref = ref + res
    got = vh.conv2d_fwd_h16(_nhwc_t(dy, dt), vh.pack_conv_weight_h16(wt.float().to(dev()), dt), None, None, 2, 1, False,
                            residual=None if res is None else _nhwc_t(res, dt))
    torch.cuda.synchronize()
    got = _back(got)
    assert got.shape == ref.shape
    if regime == "exact":
        assert int((got != HC.round_to(ref, dt)).sum()) == 0
    else:
        bound = 4 * 16 * cout * U * F.conv2d(dy.abs(), wt.abs(), None, 2, 1) + 4 * U * (ref.abs() + (0.0 if res is None else res.abs())) + _t_rounding(ref, tname)
        assert ((got - ref).abs() <= bound).all()
