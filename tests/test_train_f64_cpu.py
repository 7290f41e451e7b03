"""Host-only checks of the float64 reference gradients (alphapose/models/hip_train_f64.py): the host statements of the feature's host
logic (tests/train_f64_cases.py: packed data-gradient filter + phase launches, split count) against torch float64 autograd, the
library's host-side size queries, the refusals that need no device, and that the product path never mentions the reference."""
import itertools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_f64_cases as FC
from tests import train_h16_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESET = {"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]}
HRNET = {"TYPE": "PoseHighResolutionNet", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50, "FINAL_CONV_KERNEL": 1, "PRETRAINED_LAYERS": ["*"],
         "STAGE2": {"NUM_MODULES": 1, "NUM_BRANCHES": 2, "NUM_BLOCKS": [4, 4], "NUM_CHANNELS": [32, 64], "BLOCK": "BASIC", "FUSE_METHOD": "SUM"},
         "STAGE3": {"NUM_MODULES": 4, "NUM_BRANCHES": 3, "NUM_BLOCKS": [4, 4, 4], "NUM_CHANNELS": [32, 64, 128], "BLOCK": "BASIC", "FUSE_METHOD": "SUM"},
         "STAGE4": {"NUM_MODULES": 3, "NUM_BRANCHES": 4, "NUM_BLOCKS": [4, 4, 4, 4], "NUM_CHANNELS": [32, 64, 128, 256], "BLOCK": "BASIC", "FUSE_METHOD": "SUM"}}


def _rand(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape))


def _build(cfg):
    from alphapose.models import builder
    from alphapose.utils.config import edict
    return builder.build_sppe(edict(cfg), preset_cfg=edict(PRESET))


@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("name", list(TC.DGRAD_CASES))
def test_packed_filter_and_phase_launches_equal_autograd(name, with_residual):
    """The flat filter layout the device packer writes and the per-phase stride-1 convs the launcher issues, stated on the host,
    reproduce the data gradient of the conv (float64 autograd), with the skip gradient riding along."""
    n, cin, cout, h, w, r, stride, pad = TC.DGRAD_CASES[name]
    rs = np.random.RandomState(3)
    x, wt = _rand(rs, n, cin, h, w).requires_grad_(True), _rand(rs, cout, cin, r, r)
    y = F.conv2d(x, wt, None, stride, pad)
    dz = _rand(rs, *y.shape)
    y.backward(dz)
    res = _rand(rs, n, cin, h, w) if with_residual else None
    packed = FC.pack_dgrad_filter(wt, stride, pad)
    assert packed.numel() == cin * r * r * cout                          # every tap in exactly one phase
    got = FC.dgrad_from_packed(dz, packed, cin, h, w, r, r, stride, pad, residual=res)
    want = x.grad if res is None else x.grad + res
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


def test_phase_tables_of_the_cases():
    """Stride 1: one phase with every tap, flipped.  3x3 / 2 / pad 1: phases of 1x1, 1x2, 2x1 and 2x2 taps.  1x1 / 2: three phases no tap
    reaches.  Odd extents: four different phase grids."""
    assert FC.dgrad_phases(3, 3, 1, 1) == [(0, 0, [2, 1, 0], [2, 1, 0], 1, 1)]
    assert [(len(ty), len(tx)) for _, _, ty, tx, _, _ in FC.dgrad_phases(3, 3, 2, 1)] == [(1, 1), (1, 2), (2, 1), (2, 2)]
    assert [(bool(ty), bool(tx)) for _, _, ty, tx, _, _ in FC.dgrad_phases(1, 1, 2, 0)] == [(True, True), (True, False), (False, True), (False, False)]
    h, w = TC.DGRAD_CASES["3x3s2_8to24_7x5"][3:5]
    grids = {(len(range(py, h, 2)), len(range(px, w, 2))) for py in (0, 1) for px in (0, 1)}
    assert len(grids) == 4


def test_deconv_data_gradient_is_the_plain_strided_conv():
    """dx of ConvTranspose2d(4,2,1) = conv2d(dz, W as OIHW, stride 2, pad 1): what the trainer launches on the forward kernel."""
    n, cin, cout, h, w = TC.DGRAD_DECONV_CASE
    rs = np.random.RandomState(4)
    x, wt = _rand(rs, n, cin, h, w).requires_grad_(True), _rand(rs, cin, cout, 4, 4)
    y = F.conv_transpose2d(x, wt, None, 2, 1)
    dz = _rand(rs, *y.shape)
    y.backward(dz)
    torch.testing.assert_close(F.conv2d(dz, wt, None, 2, 1), x.grad, rtol=1e-12, atol=1e-12)


def test_split_count_is_a_function_of_m_only():
    """The host statement, the header constant and the library's host-side queries agree (no device call is made)."""
    import vatl_hip as vh
    header = open(os.path.join(ROOT, "include", "vatl_hip.h")).read()
    assert int(re.search(r"#define VATL_WGRAD_F64_CHUNK (\d+)", header).group(1)) == FC.WGRAD_CHUNK
    for m in (0, 1, 45, FC.WGRAD_CHUNK - 1, FC.WGRAD_CHUNK, FC.WGRAD_CHUNK + 1, 4158, 120 * 128 * 96):
        assert vh.wgrad_f64_splits(m) == FC.wgrad_splits(m), m
        assert int(vh.lib().vatl_conv2d_wgrad_f64_workspace_doubles(17, 3, 7, 5, m)) == FC.wgrad_splits(m) * 17 * 3 * 7 * 5
    assert [FC.wgrad_splits(m) for m in (1, 2048, 2049, 4158)] == [1, 1, 2, 3]
    assert int(vh.lib().vatl_bn_f64_workspace_doubles(513, 17)) == 2 * 2 * 17 and int(vh.lib().vatl_bn_f64_workspace_doubles(0, 17)) == 0


def test_split_case_straddles_this_kernels_chunks():
    n, _, _, h, w = TC.WGRAD_SPLIT_CASE[:5]
    m = n * h * w
    assert m // FC.WGRAD_CHUNK == 2 and m % FC.WGRAD_CHUNK != 0 and m % FC.K_TILE != 0 and (m % FC.WGRAD_CHUNK) % FC.K_TILE != 0
    assert all(edge % (h * w) for edge in (FC.WGRAD_CHUNK, 2 * FC.WGRAD_CHUNK))          # an image straddles each chunk boundary


@pytest.mark.parametrize("model", ["FastPose", "HRNet"])
def test_trainer_refuses_other_networks_by_name_without_a_device(model):
    from alphapose.models import hip_train_f64
    m = _build({"TYPE": "FastPose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50} if model == "FastPose" else HRNET)
    with pytest.raises(NotImplementedError, match=model):
        hip_train_f64.trainer_for_f64(m)


def test_trainer_refuses_basic_block_resnets_and_cpu_tensors():
    from alphapose.models import hip_train_f64
    import vatl_hip as vh
    cfg = {"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256]}
    basic = _build(dict(cfg, NUM_LAYERS=50))
    basic.preact.layer4[2] = torch.nn.Identity()                           # a block without conv3 stands for a BasicBlock trunk (the package builds none)
    with pytest.raises(NotImplementedError, match="BasicBlock"):
        hip_train_f64.trainer_for_f64(basic)
    m = _build(dict(cfg, NUM_LAYERS=50))
    tr = hip_train_f64.trainer_for_f64(m)
    assert "_vatl_trainer_f64" not in m.__dict__ and not any("f64" in k for k in m.__dict__)      # nothing is cached on the module
    assert hip_train_f64.trainer_for_f64(m) is not tr
    with pytest.raises(vh.VatlError):
        tr.forward(torch.zeros(1, 3, 64, 48))
    with pytest.raises(vh.VatlError):
        tr.backward(torch.zeros(1, 17, 16, 12, dtype=torch.float64))
    assert not hasattr(hip_train_f64, "forward_train_f64")                                       # no autograd bridge: fp32 .grad would round the reference away


def test_the_product_path_never_mentions_the_reference():
    """model(x), the trainers, ActiveLearning and bench.py do not import hip_train_f64 nor call its entry points."""
    pkg = os.path.join(ROOT, "vatl4pose-wacv2024_amd")
    words = re.compile(r"hip_train_f64|_wgrad_f64|_dgrad_f64|bn_train_\w+_f64|bn_apply_f64|maxpool3x3s2_bwd_f64|col_sum_f64")
    allowed = {os.path.join(pkg, "alphapose", "models", "hip_train_f64.py"), os.path.join(pkg, "vatl_hip", "__init__.py")}
    seen = 0
    for base, dirs, files in itertools.chain(os.walk(pkg), [(ROOT, [], ["bench.py", "__graft_entry__.py"])]):
        dirs[:] = [d for d in dirs if d not in ("build", "build_ablation", "__pycache__", "csrc")]
        for f in files:
            path = os.path.join(base, f)
            if f.endswith(".py") and path not in allowed:
                seen += 1
                assert not words.search(open(path).read()), path
    assert seen > 20
