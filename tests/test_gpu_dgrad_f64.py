"""The float64 data gradient (the launcher and packer at the end of csrc/conv_f64.hip, on conv_f64_kernel as it is) against float64
autograd on the host, in two regimes.

Exact: integer operands in [-2, 2]: every partial sum is an integer below 2^53, so the device must equal autograd BIT FOR BIT.
Random: standard normal operands.  An element of dx adds at most K = R*S*Cout fused products in one chain (+ the residual): bound,
derived and not tuned, (K + 2) * 2^-53 * sum |terms| with the sum of absolute terms evaluated as the transposed conv of |dz| with |w|
(+ |residual|).  The packed filter is compared bit for bit with the host statement of its layout (tests/train_f64_cases.py), which
tests/test_train_f64_cpu.py holds to autograd.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_f64_cases as FC
from tests import train_h16_cases as TC
from tests.gpu_util import dev, record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def _case(name, exact, seed):
    """-> dz, w (fp32-representable float64), residual, autograd dx, sum of absolute terms (all host NCHW float64)."""
    n, cin, cout, h, w, r, stride, pad = TC.DGRAD_CASES[name]
    rs = np.random.RandomState(seed)
    ho, wo = TC.out_size(h, r, stride, pad), TC.out_size(w, r, stride, pad)
    if exact:
        gen = lambda *s: torch.from_numpy(rs.randint(-2, 3, s).astype(np.float64))
    else:
        gen = lambda *s: torch.from_numpy(rs.standard_normal(s))
    dz, res = gen(n, cout, ho, wo), gen(n, cin, h, w)
    wt = gen(cout, cin, r, r).float().double()                            # the packer reads the fp32 parameter
    x = torch.zeros(n, cin, h, w, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, wt, None, stride, pad).backward(dz)
    opad = ((h + 2 * pad - r) % stride, (w + 2 * pad - r) % stride)
    mag = F.conv_transpose2d(dz.abs(), wt.abs(), None, stride, pad, output_padding=opad)
    return dz, wt, res, x.grad.clone(), mag


def _device_dgrad(vh, name, dz, wt, res):
    n, cin, cout, h, w, r, stride, pad = TC.DGRAD_CASES[name]
    wd = vh.pack_conv_weight_dgrad_f64(wt.float().to(dev()), stride, pad)
    assert torch.equal(wd.cpu(), FC.pack_dgrad_filter(wt, stride, pad))   # the packer writes the layout the host states
    dx = vh.conv2d_dgrad_f64(FC.nhwc(dz).to(dev()), wd, (n, h, w, cin), r, r, stride, pad, residual=None if res is None else FC.nhwc(res).to(dev()))
    torch.cuda.synchronize()
    assert dx.dtype == torch.float64 and tuple(dx.shape) == (n, h, w, cin)
    return dx.cpu().permute(0, 3, 1, 2)


@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("name", list(TC.DGRAD_CASES))
def test_dgrad_exact_on_small_integers(vh, name, with_residual):
    dz, wt, res, ref, _ = _case(name, True, 7)
    got = _device_dgrad(vh, name, dz, wt, res if with_residual else None)
    want = ref + res if with_residual else ref
    bad = int((got != want).sum())
    record(f"dgrad_f64_exact_{name}_{int(with_residual)}", mismatches=bad)
    assert bad == 0, (name, bad)


@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("name", list(TC.DGRAD_CASES))
def test_dgrad_against_host_autograd(vh, name, with_residual):
    n, cin, cout, h, w, r, stride, pad = TC.DGRAD_CASES[name]
    dz, wt, res, ref, mag = _case(name, False, 19)
    got = _device_dgrad(vh, name, dz, wt, res if with_residual else None)
    want = ref + res if with_residual else ref
    bound = (r * r * cout + 2) * FC.U * (mag + (res.abs() if with_residual else 0.0))
    err = (got - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    record(f"dgrad_f64_{name}_{int(with_residual)}", max_abs=float(err.max()), worst_over_bound=worst)
    print(f"{name}: max |got - ref| {float(err.max()):.3e}, worst error / bound {worst:.3e}")
    assert torch.isfinite(got).all() and (err <= bound).all(), (name, float(err.max()), worst)


def test_odd_extent_stride2_case_has_four_different_phase_grids(vh):
    n, cin, cout, h, w, r, stride, pad = TC.DGRAD_CASES["3x3s2_8to24_7x5"]
    grids = {(len(range(py, h, 2)), len(range(px, w, 2))) for py in (0, 1) for px in (0, 1)}
    assert stride == 2 and len(grids) == 4
    # an impulse in dz reaches exactly the 3x3 input pixels of its window, through all four phases
    dz = torch.zeros(n, cout, TC.out_size(h, r, stride, pad), TC.out_size(w, r, stride, pad), dtype=torch.float64)
    dz[1, 5, 2, 1] = 1.0
    wt = torch.from_numpy(np.random.RandomState(2).randint(1, 4, (cout, cin, r, r)).astype(np.float64))
    got = _device_dgrad(vh, "3x3s2_8to24_7x5", dz, wt, None)
    want = torch.zeros(n, cin, h, w, dtype=torch.float64)
    want[1, :, 3:6, 1:4] = wt[5]
    assert torch.equal(got, want)


@pytest.mark.parametrize("with_residual", [False, True])
def test_unreached_phases_are_filled(vh, with_residual):
    """1x1 / stride 2: the odd pixels receive no tap.  They are the residual bit for bit, or +0.0 (not -0.0, not stale memory)."""
    name = "1x1s2_8to32_5x5"
    dz, wt, res, ref, _ = _case(name, False, 31)
    res = -res.abs() - 1.0 if with_residual else None                     # negative everywhere: a fill of zeros would show
    got = _device_dgrad(vh, name, dz, wt, res)
    odd = torch.ones(5, 5, dtype=torch.bool)
    odd[0::2, 0::2] = False
    if with_residual:
        assert torch.equal(got[:, :, odd], res[:, :, odd])
    else:
        assert bool((got[:, :, odd] == 0).all()) and not bool(torch.signbit(got[:, :, odd]).any())
    assert float(got[:, :, ~odd].abs().min()) > 0


def test_deconv_data_gradient(vh):
    """ConvTranspose2d(4,2,1): the plain 4x4 / stride 2 / pad 1 conv of dz with the (Cin,Cout,4,4) parameter as its OIHW filter."""
    n, cin, cout, h, w = TC.DGRAD_DECONV_CASE
    for regime in ("exact", "random"):
        rs = np.random.RandomState(37)
        gen = (lambda *s: torch.from_numpy(rs.randint(-2, 3, s).astype(np.float64))) if regime == "exact" else (lambda *s: torch.from_numpy(rs.standard_normal(s)))
        wt, dz = gen(cin, cout, 4, 4).float().double(), gen(n, cout, 2 * h, 2 * w)
        x = torch.zeros(n, cin, h, w, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(x, wt, None, 2, 1).backward(dz)
        got = vh.conv2d_fwd_f64(FC.nhwc(dz).to(dev()), vh.pack_conv_weight_f64(wt.float().to(dev())), None, None, 2, 1, False)
        torch.cuda.synchronize()
        got = got.cpu().permute(0, 3, 1, 2)
        if regime == "exact":
            assert torch.equal(got, x.grad)
        else:
            bound = (16 * cout + 2) * FC.U * F.conv2d(dz.abs(), wt.abs(), None, 2, 1)
            assert ((got - x.grad).abs() <= bound).all()


@pytest.mark.parametrize("name", ["3x3s2_8to24_7x5", "head1x1_16to17_6x5"])
def test_two_runs_are_bit_equal(vh, name):
    dz, wt, res, _, _ = _case(name, False, 41)
    a = _device_dgrad(vh, name, dz, wt, res)
    b = _device_dgrad(vh, name, dz, wt, res)
    assert torch.equal(a, b) and float(a.abs().sum()) > 0


def test_refusals(vh):
    lib = vh.lib()
    dz = torch.zeros((1, 4, 4, 5), device=dev(), dtype=torch.float64)
    wd = torch.zeros((3 * 9 * 5,), device=dev(), dtype=torch.float64)
    dx = torch.full((1, 4, 4, 3), 7.0, device=dev(), dtype=torch.float64)
    call = lambda a, b, c, stride=1, r=3: lib.vatl_conv2d_dgrad_f64(a, b, None, c, 1, 4, 4, 3, 5, r, r, stride, 1, None)
    assert call(None, wd.data_ptr(), dx.data_ptr()) != 0
    assert call(dz.data_ptr(), wd.data_ptr(), dx.data_ptr(), stride=3) != 0
    assert call(dz.data_ptr(), wd.data_ptr(), dx.data_ptr(), r=8) != 0
    assert lib.vatl_pack_conv_weight_dgrad_f64(None, wd.data_ptr(), 5, 3, 3, 3, 1, 1, None) != 0
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all())
    with pytest.raises(vh.VatlError):
        vh.conv2d_dgrad_f64(dz, wd, (1, 4, 4, 4), 3, 3, 1, 1)
    with pytest.raises(vh.VatlError):
        vh.conv2d_dgrad_f64(dz, wd, (1, 4, 4, 3), 3, 3, 1, 1, residual=dz)
