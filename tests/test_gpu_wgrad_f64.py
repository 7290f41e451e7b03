"""The float64 weight-gradient kernel (csrc/wgrad_f64.hip) against the sum's definition on the host, in two regimes.

Exact: operands are integers in [-2, 2].  Every product and every partial sum is an integer of magnitude <= 4 * M < 2^53 (M pixels; the
largest case has M = 4158), so float64 accumulates without rounding whatever the order and the result must equal the definition BIT FOR BIT.
Random: standard normal operands.  The device adds M products per element (fused, so a product is not rounded on its own) in a chain
cut into splits whose slabs are then added in order: at most M + splits - 1 roundings, each of relative size 2^-53 on a partial sum that
is bounded by the sum of the absolute terms.  The host reference (tests/train_h16_cases.wgrad_ref, float64) rounds too, pairwise and by
far less.  Bound, derived and not tuned: (M + 2) * 2^-53 * sum |terms|, the sum of absolute terms evaluated as wgrad_ref(|x|, |dz|);
`worst / bound` is recorded per case.  Channel counts 3, 17 and 24 run unpadded: the kernel takes NHWC tensors of any channel count.
"""
import numpy as np
import pytest
import torch

from tests import train_f64_cases as FC
from tests import train_h16_cases as TC
from tests.gpu_util import dev, record

pytestmark = pytest.mark.gpu

ALL_CASES = dict(TC.WGRAD_CASES, split_1x1_8to8_7x9_n66=TC.WGRAD_SPLIT_CASE)


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def _operands(case, exact, seed):
    n, cin, cout, h, w, r, stride, pad, _ = case
    rs = np.random.RandomState(seed)
    ho, wo = TC.out_size(h, r, stride, pad), TC.out_size(w, r, stride, pad)
    if exact:
        return (torch.from_numpy(rs.randint(-2, 3, (n, cin, h, w)).astype(np.float64)), torch.from_numpy(rs.randint(-2, 3, (n, cout, ho, wo)).astype(np.float64)))
    return torch.from_numpy(rs.standard_normal((n, cin, h, w))), torch.from_numpy(rs.standard_normal((n, cout, ho, wo)))


def _device_wgrad(vh, case, x, dz):
    n, cin, cout, h, w, r, stride, pad, _ = case
    xd, dzd = FC.nhwc(x).to(dev()), FC.nhwc(dz).to(dev())
    assert xd.shape[-1] == cin and dzd.shape[-1] == cout                  # unpadded: 3, 17 and 24 channels as they are
    got = vh.conv2d_wgrad_f64(xd, dzd, cout, cin, r, r, stride, pad)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and tuple(got.shape) == (cout, cin, r, r)
    return got.cpu()


def _check(name, got, ref, bound):
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    record(f"wgrad_f64_{name}", max_abs=float(err.max()), worst_over_bound=worst, ref_absmax=float(ref.abs().max()))
    print(f"{name}: max |got - ref| {float(err.max()):.3e}, worst error / bound {worst:.3e}")
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (name, float(err.max()), worst)


def test_the_cases_cover_unpadded_channel_counts():
    chans = {c for case in ALL_CASES.values() for c in case[1:3]}
    assert {3, 17, 24} <= chans


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_wgrad_exact_on_small_integers(vh, name):
    case = ALL_CASES[name]
    x, dz = _operands(case, True, 5)
    ref = TC.wgrad_ref(x, dz, case[5], case[5], case[6], case[7])
    m = dz.shape[0] * dz.shape[2] * dz.shape[3]
    assert 4 * m < 2 ** 53 and float(ref.abs().max()) <= 4 * m
    got = _device_wgrad(vh, case, x, dz)
    bad = int((got != ref).sum())
    record(f"wgrad_f64_exact_{name}", mismatches=bad, ref_absmax=float(ref.abs().max()))
    assert bad == 0, (name, bad, float((got - ref).abs().max()))


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_wgrad_against_the_definition(vh, name):
    case = ALL_CASES[name]
    x, dz = _operands(case, False, 17)
    r, stride, pad = case[5], case[6], case[7]
    ref = TC.wgrad_ref(x, dz, r, r, stride, pad)
    m = dz.shape[0] * dz.shape[2] * dz.shape[3]
    bound = (m + 2) * FC.U * TC.wgrad_ref(x.abs(), dz.abs(), r, r, stride, pad)
    _check(name, _device_wgrad(vh, case, x, dz), ref, bound)


def test_split_count_of_the_split_case(vh):
    n, _, _, h, w = TC.WGRAD_SPLIT_CASE[:5]
    m = n * h * w
    assert m == 2 * FC.WGRAD_CHUNK + 62 and m % FC.K_TILE != 0 and 62 % FC.K_TILE != 0
    for edge in (FC.WGRAD_CHUNK, 2 * FC.WGRAD_CHUNK):
        assert edge % (h * w) != 0                       # an image straddles the chunk boundary
    assert vh.wgrad_f64_splits(m) == 3
    assert [vh.wgrad_f64_splits(k) for k in (1, FC.WGRAD_CHUNK, FC.WGRAD_CHUNK + 1)] == [1, 1, 2]


@pytest.mark.parametrize("regime", ["exact", "random"])
@pytest.mark.parametrize("name", list(TC.WGRAD_DECONV_CASES))
def test_transposed_conv_wgrad(vh, name, regime):
    """ConvTranspose2d(4,2,1): the forward input is the "dz side", the result is written in the parameter's (Cin,Cout,4,4) layout."""
    n, cin, cout, h, w = TC.WGRAD_DECONV_CASES[name]
    rs = np.random.RandomState(29)
    if regime == "exact":
        x = torch.from_numpy(rs.randint(-2, 3, (n, cin, h, w)).astype(np.float64))
        dy = torch.from_numpy(rs.randint(-2, 3, (n, cout, 2 * h, 2 * w)).astype(np.float64))
    else:
        x, dy = torch.from_numpy(rs.standard_normal((n, cin, h, w))), torch.from_numpy(rs.standard_normal((n, cout, 2 * h, 2 * w)))
    ref = TC.deconv_wgrad_ref(x, dy)
    got = vh.conv2d_wgrad_f64(FC.nhwc(x).to(dev()), FC.nhwc(dy).to(dev()), cout, cin, 4, 4, 2, 1, transposed=True)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (cin, cout, 4, 4) and got.dtype == torch.float64
    got = got.cpu()
    if regime == "exact":
        assert int((got != ref).sum()) == 0
    else:
        _check(f"{name}", got, ref, (n * h * w + 2) * FC.U * TC.deconv_wgrad_ref(x.abs(), dy.abs()))


@pytest.mark.parametrize("name", ["split_1x1_8to8_7x9_n66", "stem7x7s2_3to64_9x7", "head1x1_16to17_6x5"])
def test_two_runs_and_another_stream_are_bit_equal(vh, name):
    case = ALL_CASES[name]
    n, cin, cout, h, w, r, stride, pad, _ = case
    x, dz = _operands(case, False, 23)
    xd, dzd = FC.nhwc(x).to(dev()), FC.nhwc(dz).to(dev())
    a = vh.conv2d_wgrad_f64(xd, dzd, cout, cin, r, r, stride, pad)
    b = vh.conv2d_wgrad_f64(xd, dzd, cout, cin, r, r, stride, pad)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        c = vh.conv2d_wgrad_f64(xd, dzd, cout, cin, r, r, stride, pad)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    assert float(a.abs().sum()) > 0 and torch.equal(a, b) and torch.equal(a, c)


def test_refusals(vh):
    """Bad arguments, a null workspace and a workspace that is too small return an error code and launch nothing."""
    lib = vh.lib()
    x = torch.zeros((1, 4, 4, 3), device=dev(), dtype=torch.float64)
    dz = torch.zeros((1, 4, 4, 17), device=dev(), dtype=torch.float64)
    need = int(lib.vatl_conv2d_wgrad_f64_workspace_doubles(17, 3, 3, 3, 16))
    assert need == 17 * 9 * 3
    ws = torch.full((need,), 7.0, device=dev(), dtype=torch.float64)
    args = lambda wsp, doubles, r=3, stride=1, pad=1, tr=0, cin=3: (x.data_ptr(), dz.data_ptr(), wsp, doubles, 1, 4, 4, cin, 17, r, r, stride, pad, tr, None)
    assert lib.vatl_conv2d_wgrad_f64(*args(None, need)) != 0
    assert b"workspace" in lib.vatl_last_error()
    assert lib.vatl_conv2d_wgrad_f64(*args(ws.data_ptr(), need - 1)) != 0
    assert b"workspace" in lib.vatl_last_error()
    assert lib.vatl_conv2d_wgrad_f64(*args(ws.data_ptr(), need, stride=3)) != 0
    assert lib.vatl_conv2d_wgrad_f64(*args(ws.data_ptr(), need, r=8)) != 0
    assert lib.vatl_conv2d_wgrad_f64(*args(ws.data_ptr(), need, cin=0)) != 0
    assert lib.vatl_conv2d_wgrad_f64(*args(ws.data_ptr(), need, tr=1)) != 0
    assert b"ConvTranspose2d" in lib.vatl_last_error()
    assert lib.vatl_conv2d_wgrad_f64(None, dz.data_ptr(), ws.data_ptr(), need, 1, 4, 4, 3, 17, 3, 3, 1, 1, 0, None) != 0
    torch.cuda.synchronize()
    assert bool((ws == 7.0).all())                       # nothing was launched
    with pytest.raises(vh.VatlError):
        vh.conv2d_wgrad_f64(x, dz, 17, 4, 3, 3, 1, 1)    # the wrapper: channel counts that do not match the tensors
    with pytest.raises(vh.VatlError):
        vh.conv2d_wgrad_f64(x, dz[:, :3].contiguous(), 17, 3, 3, 3, 1, 1)
    assert lib.vatl_conv2d_wgrad_f64(*args(ws.data_ptr(), need)) == 0
    torch.cuda.synchronize()
    assert bool((ws == 0.0).all())
