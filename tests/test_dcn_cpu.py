"""Deformable convolution without a GPU: the float64 oracle of tests/dcn_cases.py against closed forms, the builder surface of a DCN
FastPose (keys, shapes, strict loading) and the untouched key list of a config without ``DCN``."""
import pytest
import torch
import torch.nn.functional as F

from tests import dcn_cases as D


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dg", [1, 2])
def test_oracle_zero_offsets_is_conv2d(stride, dg):
    x, w = _rand(2, 8, 7, 5, seed=1), _rand(6, 8, 3, 3, seed=2)
    ho, wo = D.out_hw(7, 5, stride)
    off = torch.zeros(2, 18 * dg, ho, wo, dtype=torch.float64)
    want = F.conv2d(x, w, stride=stride, padding=1)
    torch.testing.assert_close(D.deform_conv_ref(x, w, off, None, stride, dg), want, rtol=1e-12, atol=1e-12)
    ones = torch.ones(2, 9 * dg, ho, wo, dtype=torch.float64)
    torch.testing.assert_close(D.deform_conv_ref(x, w, off, ones, stride, dg), want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(D.deform_conv_ref(x, w, off, 0.5 * ones, stride, dg), 0.5 * want, rtol=1e-12, atol=1e-12)


def test_oracle_integer_offsets_shift_the_taps():
    """Every tap moved by the same integer (dy, dx) = the taps of the plain conv read (dy, dx) further on in the zero-extended image:
    out[y, x] = sum_ij w[i, j] * xp[y - 1 + i + dy, x - 1 + j + dx], a window of the valid conv of the image padded by 3."""
    x, w = _rand(1, 4, 6, 7, seed=3), _rand(5, 4, 3, 3, seed=4)
    full = F.conv2d(F.pad(x, (3, 3, 3, 3)), w)                          # full[u, v] = sum_ij w[i, j] * xp[u + i - 3, v + j - 3]
    for dy, dx in ((1, 0), (0, -2), (-1, 1), (2, 2)):
        off = torch.zeros(1, 18, 6, 7, dtype=torch.float64)
        off[:, 0::2], off[:, 1::2] = dy, dx
        want = full[:, :, 2 + dy:2 + dy + 6, 2 + dx:2 + dx + 7]
        torch.testing.assert_close(D.deform_conv_ref(x, w, off, None, 1, 1), want, rtol=1e-12, atol=1e-12)


def test_oracle_tap_pushed_outside_contributes_nothing():
    x, w = _rand(1, 4, 5, 5, seed=5), _rand(3, 4, 3, 3, seed=6)
    for bad in (1e4, -1e4, float("inf"), float("nan")):
        off = torch.zeros(1, 18, 5, 5, dtype=torch.float64)
        off[:, 2 * 4] = bad                                             # the centre tap's dy, everywhere
        w0 = w.clone()
        w0[:, :, 1, 1] = 0
        got = D.deform_conv_ref(x, w, off, None, 1, 1)
        assert torch.isfinite(got).all()
        torch.testing.assert_close(got, F.conv2d(x, w0, padding=1), rtol=1e-12, atol=1e-12)
    # exactly -1 and exactly H are outside, just inside them is not
    off = torch.zeros(1, 18, 5, 5, dtype=torch.float64)
    off[:, 0] = 0.0                                                     # tap 0 of row 0 sits at py = -1
    assert D.deform_columns_ref(x, off, None, 1, 1)[0, :, 0, 0].abs().max() == 0
    off[:, 0] = 1e-9
    assert D.deform_columns_ref(x, off, None, 1, 1)[0, :, 0, 0, 1:].abs().max() > 0


def test_committed_gradient_cases_keep_clear_of_cell_edges():
    for k, spec in enumerate(D.ALL_CASES):
        assert D.fractional_parts_ok(D.smooth_offsets(D.make_case(*spec), 900 + k)), spec[0]


def _cfg(dcn=None):
    from alphapose.utils.config import edict
    cfg = {"TYPE": "FastPose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50}
    if dcn is not None:
        cfg.update(DCN=dcn, STAGE_WITH_DCN=[False, True, True, True])
    preset = edict({"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]})
    return edict(cfg), preset


@pytest.mark.parametrize("modulated", [False, True])
@pytest.mark.parametrize("dg", [1, 2])
def test_builder_builds_fastpose_dcn(modulated, dg):
    from alphapose.models import builder
    from alphapose.models.layers.dcn import DeformConv, ModulatedDeformConv
    cfg, preset = _cfg({"MODULATED": modulated, "DEFORM_GROUP": dg, "FALLBACK_ON_STRIDE": False})
    m = builder.build_sppe(cfg, preset_cfg=preset)
    sd = m.state_dict()
    per = 27 if modulated else 18
    blk = m.preact.layer2[0]
    assert isinstance(blk.conv2, ModulatedDeformConv if modulated else DeformConv) and blk.conv2.deformable_groups == dg
    assert tuple(sd["preact.layer2.0.conv2_offset.weight"].shape) == (dg * per, 128, 3, 3)
    assert tuple(sd["preact.layer2.0.conv2_offset.bias"].shape) == (dg * per,)
    assert tuple(sd["preact.layer2.0.conv2.weight"].shape) == (128, 128, 3, 3)
    assert "preact.layer2.0.conv2.bias" not in sd and blk.conv2_offset.stride == (2, 2) and blk.conv2.stride in (2, (2, 2))
    keys = [k for k in sd if k.startswith("preact.layer2.0.")]
    assert keys.index("preact.layer2.0.conv2_offset.weight") < keys.index("preact.layer2.0.conv2.weight") < keys.index("preact.layer2.0.bn2.weight")
    assert not any("conv2_offset" in k for k in sd if k.startswith("preact.layer1."))           # STAGE_WITH_DCN[0] is False
    for stage, n in (("layer2", 4), ("layer3", 6), ("layer4", 3)):                                  # every block of a DCN stage (SE_Resnet.py:189-211)
        assert sum(k.endswith("conv2_offset.weight") for k in sd if k.startswith(f"preact.{stage}.")) == n
    other = builder.build_sppe(cfg, preset_cfg=preset)
    other.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_fallback_on_stride_keeps_the_plain_conv():
    from alphapose.models import builder
    cfg, preset = _cfg({"MODULATED": True, "DEFORM_GROUP": 1, "FALLBACK_ON_STRIDE": True})
    plain, _ = _cfg()
    assert list(builder.build_sppe(cfg, preset_cfg=preset).state_dict()) == list(builder.build_sppe(plain, preset_cfg=preset).state_dict())


def test_config_without_dcn_has_todays_keys():
    from alphapose.models import builder
    cfg, preset = _cfg()
    m = builder.build_sppe(cfg, preset_cfg=preset)
    keys = list(m.state_dict())
    assert len(keys) == len(set(keys)) and not any("offset" in k for k in keys)
    assert all(type(b.conv2) is torch.nn.Conv2d and not b.with_dcn for s in m.preact.stages() for b in s)
    # the plain FastPose-50 key list: stem (conv + 5 BatchNorm entries), 16 bottlenecks x (3 convs + 3 x 5), 4 projections x (1 + 5),
    # 4 SE gates x 4, two DUC stages x (1 + 5), the biased output conv
    assert len(keys) == 6 + 16 * 18 + 4 * 6 + 4 * 4 + 2 * 6 + 2


def test_seeded_construction_consumes_the_generator_in_module_order():
    """conv2_offset is created before conv2 (the reference's order), so a seeded build draws conv2_offset's initial weights first."""
    from alphapose.models.layers.Resnet import Bottleneck
    torch.manual_seed(5)
    blk = Bottleneck(64, 16, dcn={"MODULATED": True, "DEFORM_GROUP": 2})
    torch.manual_seed(5)
    c1 = torch.nn.Conv2d(64, 16, kernel_size=1, bias=False)
    torch.nn.BatchNorm2d(16)
    off = torch.nn.Conv2d(16, 54, kernel_size=3, padding=1)
    assert torch.equal(c1.weight, blk.conv1.weight) and torch.equal(off.weight, blk.conv2_offset.weight) and torch.equal(off.bias, blk.conv2_offset.bias)
    bound = 1.0 / (16 * 9) ** 0.5
    assert blk.conv2.weight.abs().max() <= bound and blk.conv2.weight.abs().max() > 0.9 * bound
