"""Host-only checks of the bf16 fine-tune step's test infrastructure and configuration: the float64 references of
tests/train_h16_cases.py against autograd, the rounding simulation's plumbing, and the ``RETRAIN.PRECISION`` key."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_h16_cases as TC


def _rand(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape))


@pytest.mark.parametrize("name", list(TC.WGRAD_CASES))
def test_wgrad_reference_equals_autograd(name):
    n, cin, cout, h, w, r, stride, pad, _ = TC.WGRAD_CASES[name]
    rs = np.random.RandomState(1)
    x, wt = _rand(rs, n, cin, h, w), _rand(rs, cout, cin, r, r).requires_grad_(True)
    y = F.conv2d(x, wt, None, stride, pad)
    dz = _rand(rs, *y.shape)
    y.backward(dz)
    torch.testing.assert_close(TC.wgrad_ref(x, dz, r, r, stride, pad), wt.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", list(TC.WGRAD_DECONV_CASES))
def test_transposed_wgrad_reference_equals_autograd(name):
    n, cin, cout, h, w = TC.WGRAD_DECONV_CASES[name]
    rs = np.random.RandomState(2)
    x, wt = _rand(rs, n, cin, h, w), _rand(rs, cin, cout, 4, 4).requires_grad_(True)
    y = F.conv_transpose2d(x, wt, None, 2, 1)
    dy = _rand(rs, *y.shape)
    y.backward(dy)
    torch.testing.assert_close(TC.deconv_wgrad_ref(x, dy), wt.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", list(TC.DGRAD_CASES))
def test_phase_decomposition_equals_conv_transpose_and_autograd(name):
    n, cin, cout, h, w, r, stride, pad = TC.DGRAD_CASES[name]
    rs = np.random.RandomState(3)
    x, wt = _rand(rs, n, cin, h, w).requires_grad_(True), _rand(rs, cout, cin, r, r)
    y = F.conv2d(x, wt, None, stride, pad)
    dz = _rand(rs, *y.shape)
    y.backward(dz)
    got = TC.dgrad_ref_phases(dz, wt, h, w, stride, pad)
    torch.testing.assert_close(got, x.grad, rtol=1e-12, atol=1e-12)
    opad = ((h + 2 * pad - r) % stride, (w + 2 * pad - r) % stride)
    torch.testing.assert_close(got, F.conv_transpose2d(dz, wt, None, stride, pad, output_padding=opad), rtol=1e-12, atol=1e-12)


def test_split_case_geometry():
    n, _, _, h, w = TC.WGRAD_SPLIT_CASE[:5]
    m = n * h * w
    assert m // TC.WGRAD_CHUNK == 2 and (m % TC.WGRAD_CHUNK) % 32 != 0
    assert all(edge % (h * w) for edge in (TC.WGRAD_CHUNK, 2 * TC.WGRAD_CHUNK))
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vatl_hip.h")).read()
    assert int(re.search(r"#define VATL_WGRAD_H16_CHUNK (\d+)", header).group(1)) == TC.WGRAD_CHUNK


def test_simulation_without_rounding_is_the_oracle_graph():
    """The layer-by-layer walk of the simulation equals SimplePoseRef.forward in train mode (values and gradients) when nothing is rounded,
    and rounding moves the result without breaking it."""
    from oracle import nets
    torch.manual_seed(0)
    ref = nets.SimplePoseRef(50).double().train()
    import copy
    a, b, c = copy.deepcopy(ref), copy.deepcopy(ref), copy.deepcopy(ref)
    x = torch.randn(3, 3, 96, 64, dtype=torch.float64)
    ya, yb = a(x), TC.simulate_train_forward(b, x, None)
    torch.testing.assert_close(ya, yb, rtol=1e-12, atol=1e-14)
    ya.square().sum().backward()
    yb.square().sum().backward()
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-9, atol=1e-16, msg=k)
    torch.testing.assert_close(a.preact.bn1.running_var, b.preact.bn1.running_var)
    yc = TC.simulate_train_forward(c, x, torch.bfloat16)
    rel = float((yc - ya).detach().norm() / ya.detach().norm())
    assert 0.0 < rel < 1.0, rel
    yc.square().sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in c.parameters())


def _cfg(**retrain):
    from alphapose.utils.config import edict
    return edict({"MODEL": {"TYPE": "SimplePose"}, "RETRAIN": dict({"BATCH_SIZE": 8}, **retrain)})


def test_retrain_precision_parsing():
    from active_learning.ActiveLearning import retrain_precision
    assert retrain_precision(_cfg()) == "fp32"                         # absent -> fp32
    assert retrain_precision(_cfg(PRECISION="fp32")) == "fp32"
    assert retrain_precision(_cfg(PRECISION="bf16")) == "bf16"


@pytest.mark.parametrize("bad", ["fp16", "half", "BF16", 16, None])
def test_retrain_precision_rejects_other_values(bad):
    from active_learning.ActiveLearning import retrain_precision
    with pytest.raises(ValueError, match="RETRAIN.PRECISION"):
        retrain_precision(_cfg(PRECISION=bad))


@pytest.mark.parametrize("model", ["FastPose", "HRNet"])
def test_retrain_precision_bf16_refuses_other_networks_by_name(model):
    from active_learning.ActiveLearning import retrain_precision
    cfg = _cfg(PRECISION="bf16")
    cfg.MODEL.TYPE = model
    with pytest.raises(NotImplementedError, match=f"RETRAIN.PRECISION.*{model}"):
        retrain_precision(cfg)
    cfg.RETRAIN.PRECISION = "fp32"
    assert retrain_precision(cfg) == "fp32"
