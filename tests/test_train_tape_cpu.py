"""Host-only checks of the tape the float64 reference step and the bf16 step share (alphapose/models/hip_train_tape.py): both trainers are
built for an R50 on the CPU (constructors touch no device), their layers are the shared module's, the bf16 filter list keeps its order, the
float64 module imports neither the fp32 nor the bf16 trainer nor loads the library, and every refusal keeps the words it had when each
precision carried its own copy of the tape (the strings below are copied from that version)."""
import contextlib
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vatl4pose-wacv2024_amd")
PRESET = {"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]}
SIMPLE = {"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50}
LAYERS = ("_ConvBN", "_DeconvBN", "_BottleneckT", "_HeadT")


def _build(cfg):
    from alphapose.models import builder
    from alphapose.utils.config import edict
    return builder.build_sppe(edict(cfg), preset_cfg=edict(PRESET))


@pytest.fixture(scope="module")
def model():
    return _build(SIMPLE)


@pytest.fixture(scope="module")
def makers():
    from alphapose.models import hip_train_f64, hip_train_h16
    return {"float64": hip_train_f64.SimplePoseTrainerF64, "bf16": hip_train_h16.SimplePoseTrainerH16}


@contextlib.contextmanager
def _swapped(owner, name, new):
    """``owner.name`` (or ``owner[name]`` of a Sequential) replaced by ``new`` for the duration."""
    if isinstance(name, int):
        old, owner[name] = owner[name], new
    else:
        old = getattr(owner, name)
        setattr(owner, name, new)
    try:
        yield new
    finally:
        if isinstance(name, int):
            owner[name] = old
        else:
            setattr(owner, name, old)


def _convs(tr):
    return [tr.stem] + [c for b in tr.blocks for c in (b.c1, b.c2, b.c3, b.proj) if c is not None] + tr.deconvs + [tr.head]


def test_layers_of_both_trainers_are_the_shared_modules(model, makers):
    from alphapose.models import hip_train_f64, hip_train_h16, hip_train_tape as T
    for name, make in makers.items():
        tr = make(model)
        assert isinstance(tr, T.SimplePoseTape)
        assert type(tr.stem) is T._ConvBN and type(tr.head) is T._HeadT and len(tr.blocks) == 16 and len(tr.deconvs) == 3
        assert all(type(b) is T._BottleneckT for b in tr.blocks) and all(type(d) is T._DeconvBN for d in tr.deconvs)
        assert all(type(c) is T._ConvBN for b in tr.blocks for c in (b.c1, b.c2, b.c3, b.proj) if c is not None)
        assert len(_convs(tr)) == 57 and tr.stem.need_dx is False and sum(b.proj is not None for b in tr.blocks) == 4
    for mod in (hip_train_f64, hip_train_h16):
        assert not any(hasattr(mod, n) for n in LAYERS), mod.__name__
        assert not hasattr(mod, "_check_model")
    assert all(hasattr(T, n) for n in LAYERS)


def test_bf16_filter_list_keeps_its_order(model, makers):
    """57 forward layouts and 56 data-gradient layouts (the stem's input gradient is never read): stem, then per block c1, c2, c3, proj, then the
    deconvs, then the head, ``w`` before ``wd``; the float64 trainer keeps no filter between steps."""
    import vatl_hip as vh
    from alphapose.models import hip_train_h16
    tr = makers["bf16"](model)
    want = [q for c in _convs(tr) for q in (c.w, c.wd) if q is not None]
    assert len(tr.packed) == 57 + 56 and all(a is b for a, b in zip(tr.packed, want)) and all(isinstance(q, hip_train_h16._Packed) for q in want)
    assert tr.packed[0] is tr.stem.w and tr.stem.wd is None and tr.packed[1] is tr.blocks[0].c1.w and tr.packed[2] is tr.blocks[0].c1.wd
    assert tr.packed[7] is tr.blocks[0].proj.w and tr.packed[-2] is tr.head.w and tr.packed[-1] is tr.head.wd
    weights = [p for k, p in model.named_parameters() if p.dim() == 4]
    order = [q.p for q in tr.packed if q is not tr.stem.w][::2]                   # each parameter after the stem's appears twice, w then wd
    assert tr.stem.w.p is weights[0] and len(order) == 56 and {id(p) for p in order} == {id(p) for p in weights[1:]}
    assert [q.job[0] for q in tr.packed[-8:]] == [vh.PACK_H16_DECONV, vh.PACK_H16_CONV] * 3 + [vh.PACK_H16_CONV, vh.PACK_H16_DGRAD]
    assert tr.blocks[3].c2.wd.job == (vh.PACK_H16_DGRAD, 2, 1)                    # layer2's first 3x3 runs at stride 2
    assert all(q.buf is None for q in tr.packed) and "_pack_plan" not in tr.__dict__          # nothing was packed, no plan was made
    f64 = makers["float64"](model)
    assert all(c.w is None and c.wd is None for c in _convs(f64)) and f64.stats == {}


def test_float64_module_imports_neither_trainer_nor_loads_the_library():
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from alphapose.models import hip_train_f64\n"
            "import vatl_hip\n"
            "assert 'alphapose.models.hip_train_tape' in sys.modules\n"
            "assert 'alphapose.models.hip_train' not in sys.modules and 'alphapose.models.hip_train_h16' not in sys.modules\n"
            "assert vatl_hip._lib is None\n" % (PKG, ROOT))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_shared_module_imports_torch_and_nothing_of_the_trainers():
    src = open(os.path.join(PKG, "alphapose", "models", "hip_train_tape.py")).read()
    imports = [ln.strip() for ln in src.splitlines() if ln.strip().startswith(("import ", "from "))]
    assert imports == ["import torch.nn as nn", "from .simplepose import SimplePose"], imports
    assert "vh." not in src and "hip_train." not in src and "_f64" not in src and "_h16" not in src


F64 = "the float64 reference step "
H16 = "RETRAIN.PRECISION bf16 "


@pytest.mark.parametrize("prec,fast,hrnet", [
    ("float64", F64 + "serves SimplePose only, not FastPose", F64 + "serves SimplePose only, not HRNet (PoseHighResolutionNet)"),
    ("bf16", H16 + "serves SimplePose only, not FastPose: it trains in fp32", H16 + "serves SimplePose only, not PoseHighResolutionNet: it trains in fp32")])
def test_other_networks_are_refused_in_each_precisions_words(makers, prec, fast, hrnet):
    from tests.test_train_f64_cpu import HRNET
    for cfg, want in (({"TYPE": "FastPose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50}, fast), (HRNET, hrnet)):
        with pytest.raises(NotImplementedError) as e:
            makers[prec](_build(cfg))
        assert str(e.value) == want


@pytest.mark.parametrize("prec,dcn,basic", [
    ("float64", F64 + "does not serve deformable bottlenecks (DCN)", F64 + "serves the bottleneck ResNets (50 / 101 / 152) only, not BasicBlock ResNets (18 / 34)"),
    ("bf16", H16 + "does not serve deformable bottlenecks (DCN): they train in fp32", H16 + "serves the bottleneck ResNets (50 / 101 / 152) only")])
def test_trunk_refusals_keep_their_words(model, makers, prec, dcn, basic):
    blk = model.preact.layer3[1]
    blk.with_dcn = True
    try:
        with pytest.raises(NotImplementedError) as e:
            makers[prec](model)
    finally:
        del blk.with_dcn
    assert str(e.value) == dcn
    with _swapped(model.preact.layer4, 2, nn.Identity()), pytest.raises(NotImplementedError) as e:         # a block without conv3 stands for a BasicBlock trunk
        makers[prec](model)
    assert str(e.value) == basic


@pytest.mark.parametrize("prec", ["float64", "bf16"])
def test_geometry_refusals_keep_their_words(model, makers, prec):
    cases = [(model.preact, "conv1", nn.Conv2d(3, 64, 7, 2, 3, bias=True), ""),
             (model.preact.layer1[0], "conv2", nn.Conv2d(64, 64, 3, 1, 1, groups=2, bias=False), ""),
             (model.preact.layer2[0], "conv2", nn.Conv2d(128, 128, 3, (2, 1), 1, bias=False), ""),
             (model.preact.layer3[0], "conv2", nn.Conv2d(256, 256, 3, 1, 2, dilation=2, bias=False), ""),
             (model.deconv_layers, 0, nn.ConvTranspose2d(2048, 256, 3, 2, 1, bias=False), ""),
             (model.deconv_layers, 3, nn.ConvTranspose2d(256, 256, 4, 2, 1, bias=True), ""),
             (model.deconv_layers, 6, nn.ConvTranspose2d(256, 256, 4, 2, 1, output_padding=1, bias=False), ""),
             (model, "final_layer", nn.Conv2d(256, 17, 3, 1, 1), "the head ")]
    for owner, name, new, head in cases:
        with _swapped(owner, name, new), pytest.raises(NotImplementedError) as e:
            makers[prec](model)
        assert str(e.value) == f"no {prec} training path for {head}{new}"


def test_what_only_the_float64_reference_refuses(model, makers):
    """A head without bias and a BatchNorm without affine parameters / running statistics / momentum: refused by the reference in its words;
    the bf16 trainer's constructor never looked at either."""
    for owner, name, new, head in [(model, "final_layer", nn.Conv2d(256, 17, 1, bias=False), "the head "),
                                   (model.preact, "bn1", nn.BatchNorm2d(64, affine=False), ""),
                                   (model.preact.layer2[1], "bn3", nn.BatchNorm2d(512, track_running_stats=False), ""),
                                   (model.deconv_layers, 4, nn.BatchNorm2d(256, momentum=None), ""),
                                   (model.preact.layer1[0].downsample, 1, nn.GroupNorm(4, 256), "")]:
        with _swapped(owner, name, new):
            with pytest.raises(NotImplementedError) as e:
                makers["float64"](model)
            assert str(e.value) == f"no float64 training path for {head}{new}"
            makers["bf16"](model)


def test_float64_input_and_cotangent_refusals_keep_their_words(model, makers):
    import vatl_hip as vh
    tr = makers["float64"](model)
    no_cpu = F64 + "runs on MI355X only (there is deliberately no CPU fallback)"
    for x, want in ((torch.zeros(3, 64, 48), F64 + "expects an (N,C,H,W) tensor"), ([1.0], F64 + "expects an (N,C,H,W) tensor"), (torch.zeros(1, 3, 64, 48), no_cpu)):
        with pytest.raises(vh.VatlError) as e:
            tr.forward(x)
        assert str(e.value) == want
        with pytest.raises(vh.VatlError) as e:
            tr.trunk_forward(x, 2)
        assert str(e.value) == want
    with pytest.raises(vh.VatlError) as e:
        tr.backward(torch.zeros(1, 17, 16, 12, dtype=torch.float64))
    assert str(e.value) == no_cpu
    assert torch.is_grad_enabled()                                         # the passes run under no_grad and give the caller's mode back


def test_bf16_autograd_entry_refuses_cpu_tensors_in_its_words(model):
    import vatl_hip as vh
    from alphapose.models import hip_train_h16
    with pytest.raises(vh.VatlError) as e:
        hip_train_h16.forward_train_h16(model, torch.zeros(1, 3, 64, 48))
    assert str(e.value) == "the pose network trains on MI355X only (there is deliberately no CPU fallback)"
    assert "_vatl_trainer_h16" not in model.__dict__
