"""Deformable convolution (DCN v1 / v2) on MI355X against the float64 oracle of tests/dcn_cases.py: the fused forward, the column
route, the gradients, one SE bottleneck in the engine and the trainer, whole FastPose-50-DCN and one active-learning round.

Bar: normwise rel_err (tests/gpu_util.py) <= 2e-5 against float64 — what tests/test_gpu_winograd.py holds the convolutions to.  Every
case also records the distance of the oracle itself evaluated in fp32 on the CPU."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dcn_cases as D
from tests.gpu_util import dev, record, rel_err, to_dev

pytestmark = pytest.mark.gpu

BAR = 2e-5
IDS = [c[0] for c in D.ALL_CASES]


def _nhwc(t):
    return None if t is None else to_dev(t.permute(0, 2, 3, 1).contiguous().numpy())


def _nchw64(t):
    return t.permute(0, 3, 1, 2).double().cpu()


def _check(name, what, got, ref, bar=BAR, **kw):
    e = rel_err(got.numpy(), ref.numpy())
    record("dcn", case=name, what=what, rel_err=e, **kw)
    print(f"{name} {what}: {e:.3e}", kw)
    assert e <= bar, (name, what, e)


@pytest.mark.parametrize("spec", D.ALL_CASES, ids=IDS)
def test_forward_fused_and_columns_vs_oracle(spec):
    """(a)-(d): the fused launch, the column matrix, columns + GEMM, each against float64, and fused against columns; the mask arrives
    as logits (sigmoid in the kernels)."""
    import vatl_hip as vh
    c = D.case(spec)
    x, off, ml, w = _nhwc(c["x"]), _nhwc(c["offset"]), _nhwc(c["mask_logits"]), to_dev(c["w"].numpy())
    s, dg, co, cin = c["stride"], c["dg"], c["w"].shape[0], c["w"].shape[1]
    fused = vh.deform_conv2d_fwd(x, vh.pack_deform_weight(w), off, ml, None, None, s, dg, False, mask_logits=True)
    col = vh.deform_columns(x, off, ml, s, dg, mask_logits=True)
    cols = vh.conv2d_fwd(col, vh.pack_conv_weight(vh.deform_gemm_weight(w)), None, None, co, 1, 1, 1, 0, False)
    torch.cuda.synchronize()
    m = None if c["mask_logits"] is None else torch.sigmoid(c["mask_logits"])
    col_ref = D.deform_columns_ref(c["x"], c["offset"], m, s, dg)                       # (B, C, 9, Ho, Wo)
    b, ho, wo = col.shape[:3]
    got_col = col.cpu().double()
    if got_col.shape[3] > 9 * cin:                                                      # the padding up to the GEMM's K step is zeroed
        assert got_col[..., 9 * cin:].abs().max().item() == 0
    _check(c["name"], "columns", got_col[..., :9 * cin].reshape(b, ho, wo, 9, cin).permute(0, 4, 3, 1, 2), col_ref)
    oracle32 = c["fp32_oracle_err"]
    _check(c["name"], "fused", _nchw64(fused), c["ref"], fp32_oracle=oracle32)
    _check(c["name"], "columns+gemm", _nchw64(cols), c["ref"], fp32_oracle=oracle32)
    _check(c["name"], "fused vs columns", _nchw64(fused), _nchw64(cols))


@pytest.mark.parametrize("spec", [c for c in D.ALL_CASES if c[4] % 32 == 0], ids=[c[0] for c in D.ALL_CASES if c[4] % 32 == 0])
def test_zero_offsets_agree_with_the_plain_conv(spec):
    """(e): zero offsets and mask logits of +30 (sigmoid exactly 1 in fp32), both read from one [offsets | logits] tensor as
    conv2_offset writes it: the fused launch against vh.conv2d_fwd on the same tensors, with a folded scale / bias and ReLU."""
    import vatl_hip as vh
    c = D.case(spec)
    x, w = _nhwc(c["x"]), to_dev(c["w"].numpy())
    s, dg, co = c["stride"], c["dg"], c["w"].shape[0]
    ho, wo = D.out_hw(*c["x"].shape[2:], s)
    om = torch.zeros((x.shape[0], ho, wo, 27 * dg), device=dev())
    om[..., 18 * dg:] = 30.0
    g = torch.Generator().manual_seed(7)
    scale, bias = to_dev(1 + 0.1 * torch.randn(co, generator=g).numpy()), to_dev(0.1 * torch.randn(co, generator=g).numpy())
    got = vh.deform_conv2d_fwd(x, vh.pack_deform_weight(w), om, True, scale, bias, s, dg, True)
    want = vh.conv2d_fwd(x, vh.pack_conv_weight(w), scale, bias, co, 3, 3, s, 1, True)
    v1 = vh.deform_conv2d_fwd(x, vh.pack_deform_weight(w), om, None, scale, bias, s, dg, True)
    assert torch.equal(got, v1)                                                        # a mask of exactly 1 changes no bit
    _check(c["name"], "zero offsets vs conv2d_fwd", _nchw64(got), _nchw64(want))


@pytest.mark.parametrize("spec", D.ALL_CASES, ids=IDS)
def test_gradients_vs_oracle_autograd(spec):
    """(f): dx, d_offset, d_mask and dw of the modules' autograd Function (the column route, NCHW tensors) against autograd of the
    float64 oracle, on offsets redrawn so that every fractional part lies in [0.1, 0.9]."""
    from alphapose.models.layers.dcn import deform_conv, modulated_deform_conv
    c = D.smooth_offsets(D.make_case(*spec), 900 + D.ALL_CASES.index(spec))
    assert D.fractional_parts_ok(c)
    s, dg = c["stride"], c["dg"]
    m = None if c["mask_logits"] is None else torch.sigmoid(c["mask_logits"]).float().double()      # the modules take the modulation itself
    leaves = [c["x"].clone().requires_grad_(), c["offset"].clone().requires_grad_(), c["w"].clone().requires_grad_()]
    if m is not None:
        leaves.append(m.clone().requires_grad_())
    ref = D.deform_conv_ref(leaves[0], leaves[2], leaves[1], leaves[3] if m is not None else None, s, dg)
    gy = torch.randn(ref.shape, generator=torch.Generator().manual_seed(5)).double()
    want = torch.autograd.grad(ref, leaves, gy)
    d = [t.detach().float().to(dev()).requires_grad_() for t in leaves]
    if m is None:
        y = deform_conv(d[0], d[1], d[2], s, 1, 1, 1, dg)
    else:
        y = modulated_deform_conv(d[0], d[1], d[3], d[2], None, s, 1, 1, 1, dg)
    got = torch.autograd.grad(y, d, gy.float().to(dev()))
    _check(c["name"], "module forward", y.detach().double().cpu(), ref.detach())
    for name, a, b in zip(("dx", "d_offset", "dw", "d_mask"), got, want):
        _check(c["name"], name, a.double().cpu(), b)


@pytest.mark.parametrize("spec", [c for c in D.ALL_CASES if c[8]][:4] + [D.PRODUCT_CASES[0]], ids=lambda c: c[0])
def test_columns_bwd_with_logits_behind_the_offsets(spec):
    """deform_columns_bwd as the trainer calls it: offsets and mask logits in ONE tensor, the gradients written in the same layout into a
    zero-padded tensor, the sigmoid's derivative applied in the kernel."""
    import vatl_hip as vh
    c = D.smooth_offsets(D.make_case(*spec), 950)
    s, dg, cin = c["stride"], c["dg"], c["x"].shape[1]
    om64 = torch.cat([c["offset"], c["mask_logits"]], 1).clone().requires_grad_()
    x64 = c["x"].clone().requires_grad_()
    ref = D.deform_columns_ref(x64, om64[:, :18 * dg], torch.sigmoid(om64[:, 18 * dg:]), s, dg)        # (B, C, 9, Ho, Wo)
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(6)).double()
    wx, wom = torch.autograd.grad(ref, [x64, om64], g)
    x, om = _nhwc(c["x"]), _nhwc(om64.detach())
    b, _, _, ho, wo = ref.shape
    k = vh.deform_col_stride(cin)
    dcol = torch.zeros((b, ho, wo, k), device=dev())
    dcol[..., :9 * cin] = to_dev(g.permute(0, 3, 4, 2, 1).reshape(b, ho, wo, 9 * cin).numpy())
    dx, d_om, d_mask = vh.deform_columns_bwd(dcol, x, om, True, s, dg, grad_channels=32 * ((27 * dg + 31) // 32))
    assert d_mask is None and d_om[..., 27 * dg:].abs().max().item() == 0
    _check(c["name"], "dx (logits)", _nchw64(dx), wx)
    _check(c["name"], "d_offset | d_logit", _nchw64(d_om[..., :27 * dg]), wom)


# ---- (g) one SE bottleneck of the layer2.0 shape -----------------------------------------------------------------------------------

def _se_block(modulated, dg, seed):
    from alphapose.models.layers.SE_Resnet import Bottleneck
    import torch.nn as nn
    torch.manual_seed(seed)
    proj = nn.Sequential(nn.Conv2d(256, 512, kernel_size=1, stride=2, bias=False), nn.BatchNorm2d(512, momentum=0.1))
    blk = Bottleneck(256, 128, 2, proj, reduction=True, dcn={"MODULATED": modulated, "DEFORM_GROUP": dg})
    with torch.no_grad():
        for mod in blk.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.weight.uniform_(0.5, 1.5); mod.bias.normal_(0, 0.2); mod.running_mean.normal_(0, 0.2); mod.running_var.uniform_(0.5, 1.5)
        blk.conv2_offset.weight.mul_(0.7)                       # offsets of about a pixel
    return blk


def _ref_block(p, buf, x, modulated, dg, train, masks=None):
    """The block as a float64 torch graph: F.conv2d, F.batch_norm, the SE arithmetic and the oracle.  ``masks``: the ReLU decisions of the
    fp32 forward, replayed (train); None: F.relu (eval)."""
    it = iter(masks) if masks is not None else None

    def relu(t):
        return F.relu(t) if it is None else t * next(it)

    def bn(t, n):
        return F.batch_norm(t, buf[n + ".running_mean"], buf[n + ".running_var"], p[n + ".weight"], p[n + ".bias"], train, 0.1, 1e-5)
    a = relu(bn(F.conv2d(x, p["conv1.weight"]), "bn1"))
    om = F.conv2d(a, p["conv2_offset.weight"], p["conv2_offset.bias"], stride=2, padding=1)
    mask = torch.sigmoid(om[:, 18 * dg:]) if modulated else None
    b = relu(bn(D.deform_conv_ref(a, p["conv2.weight"], om[:, :18 * dg], mask, 2, dg), "bn2"))
    u = bn(F.conv2d(b, p["conv3.weight"]), "bn3")
    h = relu(F.linear(u.mean((2, 3)), p["se.fc.0.weight"], p["se.fc.0.bias"]))
    gate = torch.sigmoid(F.linear(h, p["se.fc.2.weight"], p["se.fc.2.bias"]))
    skip = bn(F.conv2d(x, p["downsample.0.weight"], stride=2), "downsample.1")
    return relu(u * gate[:, :, None, None] + skip)


@pytest.mark.parametrize("modulated,dg", [(True, 1), (False, 2)])
def test_se_bottleneck_engine_and_trainer(modulated, dg, monkeypatch):
    from alphapose.models import hip_engine, hip_train
    blk = _se_block(modulated, dg, 11).to(dev())
    x64 = torch.randn(2, 256, 16, 12, generator=torch.Generator().manual_seed(12)).float().double()
    p64 = {k: v.detach().double().cpu().clone().requires_grad_() for k, v in blk.named_parameters()}
    buf64 = {k: v.detach().double().cpu().clone() for k, v in blk.named_buffers() if v.dtype.is_floating_point}
    xh = _nhwc(x64)
    # engine, eval mode
    blk.eval()
    with torch.no_grad():
        want = _ref_block(p64, buf64, x64, modulated, dg, False)
        for fused in (False, True):                                       # the engine's route (columns + GEMM) and the fused launch
            monkeypatch.setattr(hip_engine, "DEFORM_FUSED", fused)
            plan = hip_engine._SEBottleneckPlan(blk)
            assert (plan.c2.w is not None) == fused
            _check(f"se_block_mod{int(modulated)}_dg{dg}", f"engine eval fused={fused}", _nchw64(plan(xh)), want.detach())
    # trainer, train mode: forward, running statistics, every gradient
    blk.train()
    unit = hip_train._SEBottleneckT(blk)
    dy64 = torch.randn(want.shape, generator=torch.Generator().manual_seed(13)).float().double()
    hip_train._relu_tap = []
    try:
        with torch.no_grad():
            y = unit.forward(xh)
    finally:
        taps, hip_train._relu_tap = hip_train._relu_tap, None
    masks = [(_nchw64(t) if t.dim() == 4 else t.double().cpu()) for t in taps]
    assert len(masks) == 4
    grads = hip_train._Grads()
    with torch.no_grad():
        dx = unit.backward(_nhwc(dy64), grads)
    hip_train._side.join()
    hip_train._flush_batch_counters()
    x_leaf = x64.clone().requires_grad_()
    y64 = _ref_block(p64, buf64, x_leaf, modulated, dg, True, masks)
    names = list(p64)
    g64 = torch.autograd.grad(y64, [x_leaf] + [p64[k] for k in names], dy64)
    tag = f"se_block_mod{int(modulated)}_dg{dg}"
    _check(tag, "trainer forward", _nchw64(y), y64.detach())
    for k, v in blk.named_buffers():
        if v.dtype.is_floating_point:
            _check(tag, "running " + k, v.detach().double().cpu(), buf64[k])
    assert int(blk.bn2.num_batches_tracked) == 1
    _check(tag, "trainer dx", _nchw64(dx), g64[0])
    by_param = dict(blk.named_parameters())
    assert set(grads) == set(by_param.values())
    for k, g in zip(names, g64[1:]):
        _check(tag, "grad " + k, grads[by_param[k]].detach().double().cpu().reshape(g.shape), g)


# ---- (h) whole FastPose-50-DCN -----------------------------------------------------------------------------------------------------

def _fastpose(dcn=None):
    from alphapose.models import builder
    from alphapose.utils.config import edict
    cfg = {"TYPE": "FastPose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50}
    if dcn is not None:
        cfg.update(DCN=dcn, STAGE_WITH_DCN=[False, True, True, True])
    preset = edict({"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]})
    return builder.build_sppe(edict(cfg), preset_cfg=preset)


def _heatmaps(m, x):
    """The evaluation stream's route (hip_engine.forward_into, what ActiveLearning.eval_and_query runs)."""
    from alphapose.models import hip_engine
    hm = torch.empty((x.shape[0], 17, 64, 48), device=dev())
    with torch.no_grad():
        hip_engine.forward_into(m, x, hm)
    return hm


@pytest.fixture(scope="module")
def plain_fastpose():
    from oracle import synth
    m = _fastpose()
    sd = synth.state_dict_for(m)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev()).eval()
    x = torch.from_numpy(synth.crops(2)).to(dev())
    return sd, x, _heatmaps(m, x)


@pytest.mark.parametrize("modulated", [False, True])
def test_fastpose_dcn_whole_network(modulated, plain_fastpose):
    """With conv2_offset zeroed (bias 0 for the offsets, +30 for the mask logits) the DCN network computes the plain network's function:
    its heat-maps agree with the plain FastPose plan on the same weights.  Both plans are held to 1e-4 of the exact heat-maps (the
    project's parity contract, __graft_entry__.smoke), so that is the bar between them; small random offset weights then change them."""
    sd, x, hm_plain = plain_fastpose
    m = _fastpose({"MODULATED": modulated, "DEFORM_GROUP": 1, "FALLBACK_ON_STRIDE": False})
    missing = m.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and all("conv2_offset" in k for k in missing.missing_keys) and len(missing.missing_keys) == 26
    offs = [mod.conv2_offset for mod in m.modules() if hasattr(mod, "conv2_offset")]
    assert len(offs) == 13
    with torch.no_grad():
        for o in offs:
            o.weight.zero_(); o.bias.zero_()
            if modulated:
                o.bias[18:] = 30.0
    m = m.to(dev()).eval()
    hm = _heatmaps(m, x)
    _check(f"fastpose_dcn_mod{int(modulated)}", "zeroed offsets vs plain plan", hm.double().cpu(), hm_plain.double().cpu(), bar=1e-4)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for o in offs:
            o.weight.copy_((0.02 * torch.randn(o.weight.shape, generator=g)).to(dev()))
    hm2 = _heatmaps(m, x)
    with torch.no_grad():
        _check(f"fastpose_dcn_mod{int(modulated)}", "module call vs stream route", m(x).double().cpu(), hm2.double().cpu(), bar=1e-4)
    assert torch.isfinite(hm2).all() and rel_err(hm2.cpu().numpy(), hm.cpu().numpy()) > 1e-3


# ---- (i) one active-learning round -------------------------------------------------------------------------------------------------

def test_active_learning_round_with_dcn(tmp_path):
    from active_learning import ActiveLearning
    from alphapose.models import hip_engine
    from tests.test_gpu_al import _cfg
    cfg = _cfg()
    cfg["MODEL"] = type(cfg["MODEL"])({"TYPE": "FastPose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50,
                                       "DCN": {"MODULATED": True, "DEFORM_GROUP": 1, "FALLBACK_ON_STRIDE": False}, "STAGE_WITH_DCN": [False, True, True, True]})
    opt = types.SimpleNamespace(work_dir=str(tmp_path), uncertainty="THC_L1", representativeness="None", filter="None", strategy="THC_L1", video_id="syn",
                                get_prenext=True, from_scratch=True, continual=True, num_gpu=1, onebyone=False, retrain_thresh=1, THCvsWPU="const")
    torch.manual_seed(0)
    al = ActiveLearning(cfg, opt)
    al.eval_and_query()
    watched = {k: v.detach().clone() for k, v in al.model.named_parameters()
               if "conv2_offset" in k or (k.endswith("conv2.weight") and k.split(".")[1] in ("layer2", "layer3", "layer4"))}
    assert len(watched) == 39
    al.retrain_epoch = 1
    al.retrain_model()
    assert np.isfinite(al.last_train_loss)
    now = dict(al.model.named_parameters())
    still = [k for k, v in watched.items() if torch.equal(v, now[k].detach())]
    assert not still, still
    # a write torch does not track into a conv2_offset weight: the parameter guard notices, the next call runs the new values
    al.model.eval()
    x = torch.stack([al.eval_dataset[i][1][0] for i in range(2)]).to(dev())
    with torch.no_grad():
        hm0 = al.model(x).clone()
        w = al.model.preact.layer2[0].conv2_offset.weight
        w.data.copy_(w.data * 2 + 0.05)
        with pytest.raises(hip_engine.StalePlanError):
            hip_engine.verify(al.model)
        hm1 = al.model(x)
    assert torch.isfinite(hm1).all() and not torch.equal(hm0, hm1)
    al.close()
