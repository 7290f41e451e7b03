"""Training-mode glue of the bf16 fine-tune step (csrc/train_glue_h16.hip) against float64 on the host, for float16 and bfloat16, on
the odd planes of tests/h16_cases.GLUE_PLANES with N = 1 and 3.

The inputs are already rounded to T, so both sides start from the same numbers; the bounds are derived from the fp32 operations the
kernels perform (u = 2^-24), not tuned.  A sum of `count` fp32 terms, whatever its order, is within (count - 1) * u * sum |terms| of the
exact sum of those terms; every rounding that a TERM sees before it is added, and every rounding the TOTAL sees afterwards, adds one
more u * sum |terms|.  Counted per quantity (m = N*H*W terms per channel):
  sum z      terms exact (converted from T)            total -> float mean: 1                        (m - 1) + 1     <= (m + 2) u
  sum z^2    term z*z enters through one fma: 0        total used in double; var -> invstd float: 1  (m - 1) + 1     <= (m + 2) u
  sum g      terms exact                               total -> float dbeta: 1 (asserted apart)      (m - 1)         <= (m + 1) u
  sum g*xhat term: z - mean, * invstd, fma product: 3  total -> float dgamma: 1 (asserted apart)     (m - 1) + 3     <= (m + 4) u
(the partials of the row lanes and row blocks are added in double: no further fp32 rounding).  A stored T result adds half the spacing
of T.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import h16_cases as HC
from tests.gpu_util import dev, record

pytestmark = pytest.mark.gpu

U = HC.U32
TYPES = list(HC.DTYPES)
EPS, MOM = 1e-5, 0.1


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def _nhwc_t(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(dt).to(dev())


def _back(y):
    return y.cpu().double().permute(0, 3, 1, 2)


def _t_rounding(ref, tname):
    _, _, half_rel, half_abs = HC.DTYPES[tname]
    return (half_rel * ref.abs()).clamp_min(half_abs)


def _per_c(t):
    return t.sum(dim=(0, 2, 3))


def _data(n, plane, dt, seed):
    h, w, c = plane
    rs = np.random.RandomState(seed)
    gen = lambda: HC.round_to(torch.from_numpy(rs.standard_normal((n, c, h, w)) * rs.uniform(0.5, 2.0, (1, c, 1, 1)) + rs.standard_normal((1, c, 1, 1))), dt)
    f32 = lambda a: torch.from_numpy(a.astype(np.float32))
    return gen(), gen(), gen(), f32(rs.uniform(0.5, 1.5, c)), f32(0.1 * rs.standard_normal(c)), rs


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("plane", HC.GLUE_PLANES)
def test_bn_statistics_and_running_update(vh, plane, n, tname):
    dt = HC.DTYPES[tname][0]
    z, _, _, gamma, beta, rs = _data(n, plane, dt, 7)
    c = plane[2]
    m = n * plane[0] * plane[1]
    rm0 = torch.from_numpy((0.1 * rs.standard_normal(c)).astype(np.float32))
    rv0 = torch.from_numpy(rs.uniform(0.5, 1.5, c).astype(np.float32))
    rm, rv = rm0.clone().to(dev()), rv0.clone().to(dev())
    mean, invstd, scale, bias = [t.cpu().double() for t in vh.bn_train_fwd_stats_h16(_nhwc_t(z, dt), gamma.to(dev()), beta.to(dev()), rm, rv, MOM, EPS)]
    torch.cuda.synchronize()
    # float64 on the same stored values
    mean64, sq64, abs64 = _per_c(z) / m, _per_c(z * z) / m, _per_c(z.abs())
    var64 = sq64 - mean64 ** 2
    b_mean = (m + 2) * U * abs64 / m
    b_var = (m + 2) * U * sq64 + 2 * mean64.abs() * b_mean + b_mean ** 2
    inv64 = 1 / torch.sqrt(var64 + EPS)
    b_inv = 0.5 * (var64 - b_var + EPS).clamp_min(1e-300) ** -1.5 * b_var + U * inv64
    assert ((mean - mean64).abs() <= b_mean).all()
    assert ((invstd - inv64).abs() <= b_inv).all()
    # (scale, bias) are formed in fp32 from the saved statistics
    sc64 = gamma.double() * invstd
    assert ((scale - sc64).abs() <= 2 * U * sc64.abs()).all()
    assert ((bias - (beta.double() - mean * sc64)).abs() <= 4 * U * (beta.double().abs() + (mean * sc64).abs())).all()
    # running statistics: nn.BatchNorm2d (float64) on the same stored values
    bn = nn.BatchNorm2d(c, eps=EPS, momentum=MOM).double().train()
    with torch.no_grad():
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
        bn(z)
    unb = m / max(m - 1, 1)
    assert ((rm.cpu().double() - bn.running_mean).abs() <= MOM * b_mean + 4 * U * (rm0.double().abs() + MOM * mean64.abs())).all()
    assert ((rv.cpu().double() - bn.running_var).abs() <= MOM * unb * b_var + 4 * U * (rv0.double().abs() + MOM * unb * var64.abs())).all()
    record(f"glue_h16_bn_stats_{plane}_{n}_{tname}", mean_worst=float(((mean - mean64).abs() / b_mean).max()), invstd_worst=float(((invstd - inv64).abs() / b_inv).max()))


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("plane", HC.GLUE_PLANES)
def test_bn_apply(vh, plane, n, with_res, relu, tname):
    dt = HC.DTYPES[tname][0]
    z, res, _, scale, bias, _ = _data(n, plane, dt, 9)
    v = lambda t: t.double().view(1, -1, 1, 1)
    pre = z * v(scale) + v(bias) + (res if with_res else 0.0)
    ref = pre.relu() if relu else pre
    bound = 2 * U * ((z * v(scale)).abs() + v(bias).abs() + (res.abs() if with_res else 0.0)) + _t_rounding(ref, tname)
    got = _back(vh.bn_apply_h16(_nhwc_t(z, dt), scale.to(dev()), bias.to(dev()), _nhwc_t(res, dt) if with_res else None, relu))
    assert ((got - ref).abs() <= bound).all()


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("plane", HC.GLUE_PLANES)
def test_bn_backward(vh, plane, n, masked, tname):
    dt = HC.DTYPES[tname][0]
    z, dy, yraw, gamma, _, rs = _data(n, plane, dt, 13)
    c = plane[2]
    m = n * plane[0] * plane[1]
    y = yraw.relu() if masked else None                  # about half of the mask is off; zeros are "not positive"
    f32 = lambda a: torch.from_numpy(a.astype(np.float32))
    mean, invstd = f32((_per_c(z) / m).numpy()), f32(rs.uniform(0.5, 2.0, c))
    v = lambda t: t.double().view(1, -1, 1, 1)
    g = dy * (y > 0) if masked else dy
    xhat = (z - v(mean)) * v(invstd)
    dbeta64, dgamma64 = _per_c(g), _per_c(g * xhat)
    b_dbeta, b_dgamma = (m + 1) * U * _per_c(g.abs()), (m + 4) * U * _per_c((g * xhat).abs())
    s = v(gamma) * v(invstd)
    ref = s * (g - v(dbeta64) / m - xhat * v(dgamma64) / m)
    kb = s * v(invstd) * v(dgamma64) / m
    bound = (4 * U * ((s * g).abs() + (kb * z).abs() + (kb * v(mean)).abs() + (s * v(dbeta64) / m).abs()) + s.abs() * v(b_dbeta) / m + (s * xhat).abs() * v(b_dgamma) / m
             + _t_rounding(ref, tname))
    dz, gout, dgamma, dbeta = vh.bn_train_bwd_h16(_nhwc_t(dy, dt), None if y is None else _nhwc_t(y, dt), _nhwc_t(z, dt), gamma.to(dev()), mean.to(dev()),
                                                  invstd.to(dev()), want_g=True)
    torch.cuda.synchronize()
    assert ((dbeta.cpu().double() - dbeta64).abs() <= b_dbeta + U * dbeta64.abs()).all()
    assert ((dgamma.cpu().double() - dgamma64).abs() <= b_dgamma + U * dgamma64.abs()).all()
    assert torch.equal(_back(gout), g)                   # the skip gradient: T values masked, stored exactly
    err = (_back(dz) - ref).abs()
    record(f"glue_h16_bn_bwd_{plane}_{n}_{masked}_{tname}", worst_over_bound=float((err / bound).max()))
    assert (err <= bound).all()


@pytest.mark.parametrize("tname", TYPES)
def test_maxpool_backward_with_tied_maxima(vh, tname):
    """Post-ReLU planes are full of tied zeros: the gradient goes to the FIRST maximum of a window in scan order, as F.max_pool2d's
    autograd on the CPU sends it.  The plane holds few distinct values (ties everywhere) and an all-zero region (whole windows of zeros)."""
    dt = HC.DTYPES[tname][0]
    rs = np.random.RandomState(31)
    n, c, h, w = 2, 16, 9, 7
    x = torch.from_numpy(rs.randint(0, 3, (n, c, h, w)).astype(np.float64))
    x[:, :, :4, :4] = 0.0
    x[0, 3] = 0.0
    dp = torch.from_numpy(rs.randint(-4, 5, (n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1)).astype(np.float64))
    xr = x.clone().float().requires_grad_(True)
    F.max_pool2d(xr, 3, 2, 1).backward(dp.float())
    ref = xr.grad.double()                               # integer sums of at most four window gradients: exact in T
    got = _back(vh.maxpool3x3s2_bwd_h16(_nhwc_t(dp, dt), _nhwc_t(x, dt)))
    assert float(ref.abs().max()) <= 16
    assert torch.equal(got, ref)
