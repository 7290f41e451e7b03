"""Host-side checks of the opt-in 16-bit route's test infrastructure and public switch: the case tables of tests/h16_cases.py, the
rounding simulation the GPU tests are judged by, and the `cfg.VAL.PRECISION` parser.  No device call is made."""
import importlib

import numpy as np
import pytest
import torch

from oracle import nets
from tests import h16_cases as HC
from tests.gpu_util import rel_err


def test_case_tables_are_well_formed():
    keys = {"n", "cin", "cout", "h", "w", "r", "stride", "pad", "bn", "bias", "res", "relu", "via_converter", "contract", "t_out", "note"}
    for name, c in HC.CONV_CASES.items():
        assert set(c) == keys, name
        assert c["n"] >= 1 and 1 <= c["r"] <= 7 and c["stride"] in (1, 2) and c["pad"] >= 0 and c["h"] + 2 * c["pad"] >= c["r"] and c["w"] + 2 * c["pad"] >= c["r"]
        cin_abi = (c["cin"] + 7) // 8 * 8 if c["via_converter"] else c["cin"]
        assert c["contract"] is (cin_abi % 8 == 0) and c["t_out"] is (c["cout"] % 8 == 0)
        assert c["contract"], f"{name}: a case that is launched must meet the Cin contract"
    assert [n for n, c in HC.CONV_CASES.items() if not c["t_out"]] == ["head1x1_16to17_bias"]
    assert set(HC.NCHW_CASES) <= set(HC.CONV_CASES) and set(HC.EXACT_CASES) <= set(HC.CONV_CASES)
    # the shapes the table exists for: the longest K, a tile that straddles images, the padded stem
    assert HC.CONV_CASES["3x3_512to16_2x2"]["cin"] * 9 == 4608
    c = HC.CONV_CASES["3x3_8to8_6x5_n11"]
    assert c["n"] * c["h"] * c["w"] == 330 and c["res"] and c["relu"]
    assert HC.CONV_CASES["stem7x7s2_3to64_9x7"]["via_converter"] and HC.CONV_CASES["stem7x7s2_3to64_9x7"]["cin"] == 3
    for name, (n, cin, cout, h, w) in HC.DECONV_CASES.items():
        assert cin % 8 == 0 and cout % 8 == 0 and min(h, w) >= 1, name
    for name, c in HC.REFUSED_CASES.items():
        assert c["contract"] is False and (c["cin"] % 8 != 0 or (c["t_out"] and c["cout"] % 8 != 0)), name
    assert all(ch % 8 == 0 and h % 2 == 1 and w % 2 == 1 for h, w, ch in HC.GLUE_PLANES)
    assert {k: v[1] for k, v in HC.DTYPES.items()} == {"fp16": 0, "bf16": 1}


@pytest.mark.parametrize("name", list(HC.DTYPES))
def test_rounding_follows_torch(name):
    dt, _, half_rel, half_abs = HC.DTYPES[name]
    x = torch.from_numpy(np.random.RandomState(3).standard_normal(4096))
    r = HC.round_to(x, dt)
    assert r.dtype == torch.float64 and torch.equal(HC.round_to(r, dt), r)
    assert ((r - x).abs() <= (half_rel * x.abs()).clamp_min(half_abs)).all()               # half a spacing: relative, or the subnormal spacing near zero
    big = torch.tensor([1e5, -1e5], dtype=torch.float64)
    assert torch.isinf(HC.round_to(big, torch.float16)).all() and torch.isfinite(HC.round_to(big, torch.bfloat16)).all()      # no saturation; bf16 has the range


@pytest.mark.parametrize("name", list(HC.DTYPES))
def test_rounding_simulation_on_a_duc(name):
    """oracle.nets._DUC(16, 32): conv 3x3 + BatchNorm + functional ReLU + pixel shuffle.  The simulation differs from the float64 run
    (q > 0), by about the type's unit round-off and no more than a few of them; run on an input that is already in T it gives the same
    bits as on that input rounded again (the input rounding is idempotent), and it leaves the oracle module itself untouched."""
    dt, _, half_rel, _ = HC.DTYPES[name]
    torch.manual_seed(5)
    ref = nets._DUC(16, 32).double().eval()
    with torch.no_grad():
        ref.bn.running_mean.normal_(0, 0.1)
        ref.bn.running_var.uniform_(0.5, 1.5)
    w0 = ref.conv.weight.clone()
    x = torch.from_numpy(np.random.RandomState(44).standard_normal((3, 16, 4, 3)))
    with torch.no_grad():
        want = ref(x)
    got = HC.simulate(ref, x, dt)
    assert got.shape == want.shape == (3, 8, 8, 6) and got.dtype == torch.float64
    q = rel_err(got.numpy(), want.numpy())
    assert 0 < q <= 32 * half_rel, q
    assert torch.equal(HC.round_to(got, dt), got)                                          # BatchNorm's output was rounded; relu and the shuffle keep T values
    xt = HC.round_to(x, dt)
    assert torch.equal(HC.simulate(ref, xt, dt), got)
    assert torch.equal(ref.conv.weight, w0) and not ref.bn._forward_hooks
    with torch.no_grad():
        assert torch.equal(ref(x), want)


def test_precision_string_parser():
    mod = importlib.import_module("active_learning.ActiveLearning")
    assert mod.precision_dtype("fp32") is None
    assert mod.precision_dtype("fp16") is torch.float16 and mod.precision_dtype("bf16") is torch.bfloat16
    for bad in ("fp8", "FP16", "half", "", None, 16):
        with pytest.raises(ValueError):
            mod.precision_dtype(bad)
