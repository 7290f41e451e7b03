"""The float64 training glue (csrc/train_glue_f64.hip) against the float64 definitions on the host: BatchNorm batch statistics with the
would-be running statistics, the apply map, the BatchNorm backward with its skip output, the max-pool backward and the column sum.

Shapes: C in {1, 3, 17, 64} (one channel, odd counts, more than one 32-channel slab); M in {1, 45, one row block + 1}.  M = 1 has zero
variance, so invstd = 1 / sqrt(eps).

Bounds, derived and not tuned (u = 2^-53):
  * sums (mean, dbeta, dgamma, column sum): M terms added in some fixed order, at most M - 1 roundings plus the fused product and the
    division: (M + 8) * u * sum |terms|;
  * biased variance = q / M - mean^2 (bn_train.hip's formula): the terms of the expanded definition sum z^2 / M - 2 mean sum z / M +
    mean^2 carry the errors of q (M roundings on sum z^2 / M), of mean (M roundings on sum |z| / M, entering twice) and one rounding of
    mean^2: (M + 8) * u * (sum z^2 / M + 2 |mean| sum |z| / M + mean^2);
  * element-wise maps: the same formula evaluated by torch in float64 FROM THE DEVICE'S OWN STATISTICS differs by a handful of
    roundings (fused or not, association): 16 * u relative to the sum of the formula's absolute terms.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import dev, record

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROW_BLOCK = 512
CS = [1, 3, 17, 64]
MS = [1, 45, ROW_BLOCK + 1]
EPS, MOM = 1e-5, 0.1


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def _data(m, c, seed):
    rs = np.random.RandomState(seed)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s))
    return dict(z=t(m, c) * 2.0 + t(c) * 3.0, gamma=t(c).abs() + 0.5, beta=t(c), rm=t(c), rv=t(c).abs() + 0.5, skip=t(m, c), dy=t(m, c))


def _d(t):
    return None if t is None else t.to(dev())


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("c", CS)
def test_batch_statistics_and_would_be_running_statistics(vh, m, c):
    d = _data(m, c, 100 * c + m)
    z = d["z"]
    st = vh.bn_train_fwd_stats_f64(_d(z.reshape(1, m, 1, c)), _d(d["gamma"]), _d(d["beta"]), _d(d["rm"]), _d(d["rv"]), MOM, EPS)
    torch.cuda.synchronize()
    assert tuple(st.shape) == (7, c) and st.dtype == torch.float64
    mean, var, invstd, scale, bias, rm, rv = st.cpu()
    mean_ref = z.sum(0) / m
    var_ref = ((z - mean_ref) ** 2).sum(0) / m
    b_mean = (m + 8) * U * z.abs().sum(0) / m
    b_var = (m + 8) * U * ((z * z).sum(0) / m + 2 * mean_ref.abs() * z.abs().sum(0) / m + mean_ref ** 2)
    e_mean, e_var = (mean - mean_ref).abs(), (var - var_ref).abs()
    record(f"glue_f64_stats_c{c}_m{m}", mean_over_bound=float((e_mean / b_mean.clamp_min(1e-300)).max()), var_over_bound=float((e_var / b_var.clamp_min(1e-300)).max()))
    assert (e_mean <= b_mean).all() and (e_var <= b_var).all() and (var >= 0).all()
    if m == 1:
        assert bool((var == 0).all()) and bool(((invstd - 1.0 / np.sqrt(EPS)).abs() <= 16 * U / np.sqrt(EPS)).all())
    # everything derived from (mean, var): the same formulas in torch from the device's own statistics
    tight = lambda got, want, terms: bool(((got - want).abs() <= 16 * U * terms).all())
    inv = 1.0 / torch.sqrt(var + EPS)
    assert tight(invstd, inv, inv)
    assert tight(scale, d["gamma"] * invstd, scale.abs())
    assert tight(bias, d["beta"] - mean * scale, d["beta"].abs() + (mean * scale).abs())
    unbiased = var * m / (m - 1) if m > 1 else var
    assert tight(rm, (1 - MOM) * d["rm"] + MOM * mean, d["rm"].abs() + mean.abs())
    assert tight(rv, (1 - MOM) * d["rv"] + MOM * unbiased, d["rv"].abs() + unbiased.abs())


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("c", CS)
def test_apply(vh, m, c, with_skip, relu):
    d = _data(m, c, 200 * c + m)
    scale, bias = d["gamma"], d["beta"]
    skip = d["skip"] if with_skip else None
    y = vh.bn_apply_f64(_d(d["z"]), _d(scale), _d(bias), _d(skip), relu)
    torch.cuda.synchronize()
    want = d["z"] * scale + bias + (skip if with_skip else 0.0)
    terms = (d["z"] * scale).abs() + bias.abs() + (skip.abs() if with_skip else 0.0)
    y = y.cpu()
    if relu:
        assert bool((y >= 0).all())
        want = want.clamp_min(0.0)
    assert ((y - want).abs() <= 16 * U * terms).all()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("c", CS)
def test_batchnorm_backward(vh, m, c, masked):
    d = _data(m, c, 300 * c + m)
    z, dy, gamma = d["z"], d["dy"], d["gamma"]
    st = vh.bn_train_fwd_stats_f64(_d(z), _d(gamma), _d(d["beta"]), None, None, MOM, EPS).cpu()
    mean, invstd, scale, bias = st[0], st[2], st[3], st[4]
    y = vh.bn_apply_f64(_d(z), _d(scale), _d(bias), None, True).cpu() if masked else None
    dz, g, dgamma, dbeta = (t if t is None else t.cpu() for t in vh.bn_train_bwd_f64(_d(dy), _d(y), _d(z), _d(gamma), _d(mean), _d(invstd), want_g=True))
    torch.cuda.synchronize()
    # the ReLU mask is taken from the STORED y, and g is the skip output
    g_ref = dy * (y > 0) if masked else dy
    assert torch.equal(g, g_ref)
    if masked and m > 1:
        assert 0 < int((y > 0).sum()) < y.numel()
    xhat = (z - mean) * invstd
    b_beta = (m + 8) * U * g_ref.abs().sum(0)
    b_gamma = (m + 8) * U * (g_ref * xhat).abs().sum(0)
    e_beta, e_gamma = (dbeta - g_ref.sum(0)).abs(), (dgamma - (g_ref * xhat).sum(0)).abs()
    record(f"glue_f64_bwd_c{c}_m{m}_{int(masked)}", dbeta_over_bound=float((e_beta / b_beta.clamp_min(1e-300)).max()),
           dgamma_over_bound=float((e_gamma / b_gamma.clamp_min(1e-300)).max()))
    assert (e_beta <= b_beta).all() and (e_gamma <= b_gamma).all()
    # dz from the device's own dgamma / dbeta
    s = gamma * invstd
    want = s * (g_ref - dbeta / m - xhat * dgamma / m)
    terms = s.abs() * (g_ref.abs() + (dbeta / m).abs() + (xhat * dgamma / m).abs())
    assert ((dz - want).abs() <= 16 * U * terms).all()
    # without the skip output nothing else changes
    dz2, g2, dgamma2, dbeta2 = vh.bn_train_bwd_f64(_d(dy), _d(y), _d(z), _d(gamma), _d(mean), _d(invstd))
    assert g2 is None and torch.equal(dz2.cpu(), dz) and torch.equal(dgamma2.cpu(), dgamma) and torch.equal(dbeta2.cpu(), dbeta)


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("hw", [(7, 5), (6, 4), (1, 1), (9, 2)])
def test_maxpool_backward_with_tied_maxima(vh, hw, c):
    """Post-ReLU planes: many exact zeros, all-zero windows, odd H and W.  torch's rule (first maximum in scan order) exactly."""
    h, w = hw
    rs = np.random.RandomState(h * 10 + w + c)
    x = torch.from_numpy(rs.randint(-2, 3, (2, c, h, w)).astype(np.float64)).clamp_min(0.0)
    x[0, :, : (h + 1) // 2] = 0.0                                             # all-zero windows
    x.requires_grad_(True)
    p = F.max_pool2d(x, 3, 2, 1)
    dp = torch.from_numpy(rs.standard_normal(tuple(p.shape)))
    p.backward(dp)
    got = vh.maxpool3x3s2_bwd_f64(_d(dp.permute(0, 2, 3, 1).contiguous()), _d(x.detach().permute(0, 2, 3, 1).contiguous()))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu().permute(0, 3, 1, 2), x.grad)
    assert torch.equal(vh.maxpool3x3s2_fwd_f64(_d(x.detach().permute(0, 2, 3, 1).contiguous())).cpu().permute(0, 3, 1, 2), p.detach())


@pytest.mark.parametrize("m", MS + [3 * ROW_BLOCK + 7])
@pytest.mark.parametrize("c", CS)
def test_column_sum(vh, m, c):
    d = _data(m, c, 400 * c + m)
    got = vh.col_sum_f64(_d(d["z"]))
    again = vh.col_sum_f64(_d(d["z"]))
    torch.cuda.synchronize()
    assert torch.equal(got, again)
    assert ((got.cpu() - d["z"].sum(0)).abs() <= (m + 8) * U * d["z"].abs().sum(0)).all()
    ints = torch.from_numpy(np.random.RandomState(m).randint(-3, 4, (m, c)).astype(np.float64))
    assert torch.equal(vh.col_sum_f64(_d(ints)).cpu(), ints.sum(0))


def test_refusals(vh):
    lib = vh.lib()
    z = torch.zeros((4, 3), device=dev(), dtype=torch.float64)
    out = torch.full((7, 3), 7.0, device=dev(), dtype=torch.float64)
    ws = torch.zeros(6, device=dev(), dtype=torch.float64)
    assert lib.vatl_bn_train_fwd_stats_f64(None, 4, 3, None, None, None, None, 0.1, 1e-5, out.data_ptr(), ws.data_ptr(), None) != 0
    assert lib.vatl_bn_train_fwd_stats_f64(z.data_ptr(), 0, 3, None, None, None, None, 0.1, 1e-5, out.data_ptr(), ws.data_ptr(), None) != 0
    assert lib.vatl_bn_train_fwd_stats_f64(z.data_ptr(), 4, 0, None, None, None, None, 0.1, 1e-5, out.data_ptr(), ws.data_ptr(), None) != 0
    assert lib.vatl_bn_train_fwd_stats_f64(z.data_ptr(), 4, 3, None, None, z.data_ptr(), None, 0.1, 1e-5, out.data_ptr(), ws.data_ptr(), None) != 0
    assert lib.vatl_col_sum_f64(z.data_ptr(), 4, 3, None, ws.data_ptr(), None) != 0
    assert lib.vatl_maxpool3x3s2_bwd_f64(z.data_ptr(), z.data_ptr(), None, 1, 2, 2, 3, None) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(vh.VatlError):
        vh.bn_apply_f64(z, z[0].contiguous(), z[0, :2].contiguous(), None, True)
    with pytest.raises(vh.VatlError):
        vh.bn_train_fwd_stats_f64(z.float(), None, None, None, None, 0.1, 1e-5)
