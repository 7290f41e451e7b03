"""The 16-bit weight-gradient kernel (csrc/wgrad_h16.hip) against float64 on the host, for float16 and bfloat16, in two regimes.

Exact: operands are integers in [-2, 2].  Every product and every partial sum is an integer of magnitude <= 4 * M < 2^24 (M pixels; the
largest case has M = 4158), so fp32 accumulates without rounding whatever the order and the result must be BIT-equal to float64.
Random: operands are already rounded to T, so both sides multiply the same numbers and a product is exact in fp32; what remains is the
fp32 accumulation over the M pixels and over the split partials, bounded — derived, not tuned, the form of tests/test_gpu_conv_h16.py —
by 4 * (M + splits) * 2^-24 * sum |terms|.  `worst / bound` is recorded per case.
"""
import numpy as np
import pytest
import torch

from tests import h16_cases as HC
from tests import train_h16_cases as TC
from tests.gpu_util import dev, record

pytestmark = pytest.mark.gpu

U = HC.U32
TYPES = list(HC.DTYPES)
ALL_CASES = dict(TC.WGRAD_CASES, split_1x1_8to8_7x9_n66=TC.WGRAD_SPLIT_CASE)


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def _nhwc_t(t, dt, pad_to=None):
    """Host NCHW float64 holding T values -> device NHWC tensor of T (exact), the channels padded with zeros to `pad_to`."""
    t = t.permute(0, 2, 3, 1)
    if pad_to is not None and pad_to != t.shape[-1]:
        t = torch.cat([t, torch.zeros(*t.shape[:-1], pad_to - t.shape[-1], dtype=t.dtype)], dim=-1)
    return t.contiguous().to(dt).to(dev())


def _operands(case, dt, exact, seed):
    n, cin, cout, h, w, r, stride, pad, _ = case
    rs = np.random.RandomState(seed)
    ho, wo = TC.out_size(h, r, stride, pad), TC.out_size(w, r, stride, pad)
    if exact:
        x = torch.from_numpy(rs.randint(-2, 3, (n, cin, h, w)).astype(np.float64))
        dz = torch.from_numpy(rs.randint(-2, 3, (n, cout, ho, wo)).astype(np.float64))
    else:
        x = HC.round_to(torch.from_numpy(rs.standard_normal((n, cin, h, w))), dt)
        dz = HC.round_to(torch.from_numpy(rs.standard_normal((n, cout, ho, wo))), dt)
    return x, dz


def _device_wgrad(vh, case, dt, x, dz):
    n, cin, cout, h, w, r, stride, pad, via_converter = case
    c8 = lambda c: (c + 7) // 8 * 8
    if via_converter:                                   # the stem: 3 -> 8 channels by the input converter (T values convert exactly)
        xd = vh.nchw_to_nhwc_h16(x.float().to(dev()), dt)
    else:
        xd = _nhwc_t(x, dt)
    dzd = vh.nchw_to_nhwc_h16(dz.float().to(dev()), dt) if cout % 8 else _nhwc_t(dz, dt)      # the head: 17 -> 24 by the converter
    assert xd.shape[-1] == c8(cin) and dzd.shape[-1] == c8(cout)
    got = vh.conv2d_wgrad_h16(xd, dzd, cout, cin, r, r, stride, pad)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (cout, cin, r, r)
    return got.cpu().double()


def _check(name, got, ref, bound):
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    record(f"wgrad_h16_{name}", max_abs=float(err.max()), worst_over_bound=worst, ref_absmax=float(ref.abs().max()))
    print(f"{name}: max |got - ref| {float(err.max()):.3e}, worst error / bound {worst:.3e}")
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (name, float(err.max()), worst)


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("name", list(ALL_CASES))
def test_wgrad_exact_on_small_integers(vh, name, tname):
    case, dt = ALL_CASES[name], HC.DTYPES[tname][0]
    x, dz = _operands(case, dt, True, 5)
    ref = TC.wgrad_ref(x, dz, case[5], case[5], case[6], case[7])
    m = dz.shape[0] * dz.shape[2] * dz.shape[3]
    assert 4 * m < 2 ** 24 and float(ref.abs().max()) <= 4 * m
    got = _device_wgrad(vh, case, dt, x, dz)
    bad = int((got != ref).sum())
    record(f"wgrad_h16_exact_{name}_{tname}", mismatches=bad, ref_absmax=float(ref.abs().max()))
    assert bad == 0, (name, bad, float((got - ref).abs().max()))


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("name", list(ALL_CASES))
def test_wgrad_against_host_float64(vh, name, tname):
    case, dt = ALL_CASES[name], HC.DTYPES[tname][0]
    x, dz = _operands(case, dt, False, 17)
    r, stride, pad = case[5], case[6], case[7]
    ref = TC.wgrad_ref(x, dz, r, r, stride, pad)
    m = dz.shape[0] * dz.shape[2] * dz.shape[3]
    splits = -(-m // TC.WGRAD_CHUNK)
    bound = 4 * (m + splits) * U * TC.wgrad_ref(x.abs(), dz.abs(), r, r, stride, pad)
    _check(f"{name}_{tname}", _device_wgrad(vh, case, dt, x, dz), ref, bound)


def test_split_count_of_the_split_case(vh):
    n, _, _, h, w = TC.WGRAD_SPLIT_CASE[:5]
    m = n * h * w
    assert m == 2 * TC.WGRAD_CHUNK + 62 and (m - 2 * TC.WGRAD_CHUNK) % 32 != 0
    for edge in (TC.WGRAD_CHUNK, 2 * TC.WGRAD_CHUNK):
        assert edge % (h * w) != 0                       # an image straddles the chunk boundary
    assert vh.wgrad_h16_splits(m) == 3
    assert [vh.wgrad_h16_splits(k) for k in (1, TC.WGRAD_CHUNK, TC.WGRAD_CHUNK + 1)] == [1, 1, 2]


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("regime", ["exact", "random"])
@pytest.mark.parametrize("name", list(TC.WGRAD_DECONV_CASES))
def test_transposed_conv_wgrad(vh, name, regime, tname):
    """ConvTranspose2d(4,2,1): the forward input is the "dz side", the result is written in the parameter's (Cin,Cout,4,4) layout."""
    n, cin, cout, h, w = TC.WGRAD_DECONV_CASES[name]
    dt = HC.DTYPES[tname][0]
    rs = np.random.RandomState(29)
    if regime == "exact":
        x = torch.from_numpy(rs.randint(-2, 3, (n, cin, h, w)).astype(np.float64))
        dy = torch.from_numpy(rs.randint(-2, 3, (n, cout, 2 * h, 2 * w)).astype(np.float64))
    else:
        x = HC.round_to(torch.from_numpy(rs.standard_normal((n, cin, h, w))), dt)
        dy = HC.round_to(torch.from_numpy(rs.standard_normal((n, cout, 2 * h, 2 * w))), dt)
    ref = TC.deconv_wgrad_ref(x, dy)
    got = vh.conv2d_wgrad_h16(_nhwc_t(x, dt), _nhwc_t(dy, dt), cout, cin, 4, 4, 2, 1, transposed=True)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (cin, cout, 4, 4)
    got = got.cpu().double()
    if regime == "exact":
        assert int((got != ref).sum()) == 0
    else:
        m = n * h * w
        _check(f"{name}_{tname}", got, ref, 4 * (m + 1) * U * TC.deconv_wgrad_ref(x.abs(), dy.abs()))


def test_refusals(vh):
    """Cin % 8 != 0 at the ABI, a null workspace and a workspace that is too small return VATL_EINVAL and launch nothing."""
    lib = vh.lib()
    dt = torch.bfloat16
    x = torch.zeros((1, 4, 4, 16), device=dev(), dtype=dt)
    dz = torch.zeros((1, 4, 4, 8), device=dev(), dtype=dt)
    need = int(lib.vatl_conv2d_wgrad_h16_workspace_floats(8, 16, 3, 3, 16))
    assert need == 8 * 9 * 16
    ws = torch.full((need,), 7.0, device=dev())
    args = lambda cin8, wsp, floats: (x.data_ptr(), dz.data_ptr(), wsp, floats, 1, 4, 4, cin8, 8, 3, 3, 1, 1, 0, 1, None)
    assert lib.vatl_conv2d_wgrad_h16(*args(12, ws.data_ptr(), need)) != 0
    assert b"multiple of 8" in lib.vatl_last_error()
    assert lib.vatl_conv2d_wgrad_h16(*args(16, None, need)) != 0
    assert b"workspace" in lib.vatl_last_error()
    assert lib.vatl_conv2d_wgrad_h16(*args(16, ws.data_ptr(), need - 1)) != 0
    assert b"workspace" in lib.vatl_last_error()
    torch.cuda.synchronize()
    assert bool((ws == 7.0).all())                       # nothing was launched
    assert lib.vatl_conv2d_wgrad_h16(*args(16, ws.data_ptr(), need)) == 0
    torch.cuda.synchronize()
    assert bool((ws == 0.0).all())
