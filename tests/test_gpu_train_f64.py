"""The float64 reference step of SimplePose on the device (alphapose/models/hip_train_f64.py) against float64 autograd on the host.

SimplePose-R50, seeded default initialisation with randomised BatchNorm affine parameters, B = 3 on 96x64 crops, a seeded cotangent,
the same state loaded into oracle.nets.SimplePoseRef(50) in train mode.  The host computes the float64 autograd gradients g64 and the
fp32 autograd gradients g32 of the same step.  For EVERY tensor t (170 parameter gradients, the heat-maps, the batch mean / variance
and the would-be running statistics of all 56 BatchNorm layers):

    e = max |t_dev - t_64| / max |t_64|,   e32 = max |t_32 - t_64| / max |t_64|,   required: e <= 2^-20 * e32.

The margin is derived, not tuned.  The ratio of the unit roundoffs is 2^-29.  Two host float64 evaluations of this very step (16 threads
against one thread, channels-last, batch reversed) differ by e' = 7.7e-15 .. 1.2e-12 per tensor against e32 = 9.6e-7 .. 0.11, i.e.
e' / e32 <= 8.0e-9, about 4 * 2^-29: 2^-20 leaves two orders of magnitude over that for another accumulation order, and stays four
orders of magnitude below what a single fp32 rounding anywhere on the path produces (ratio 1e-2 .. 1) and below any mis-wired,
missing or sign-flipped term.  A tensor whose g64 is identically zero must be exactly zero on the device.  The same rule is applied to a
shallow prefix (stem, max-pool, four bottlenecks; B = 4 on 64x48; a fixed cotangent).

MEASURED on an MI355X (tests.gpu_util.record, copied to profiles/train_f64_step.jsonl; profiles/train_f64_notes.md §4), worst e / e32:
gradients 3.5e-9, heat-maps 4.0e-9, statistics 1.8e-7 (5.4x under the gate, not the 16x one would like), shallow prefix 5.0e-9.
"""
import numpy as np
import pytest
import torch

from oracle import nets, synth
from tests import train_h16_cases as TC
from tests.gpu_util import dev, record, to_dev

pytestmark = pytest.mark.gpu

GATE = 2.0 ** -20
HW = (96, 64)
SHALLOW_BLOCKS = 4


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def _model(seed):
    from alphapose.models import builder
    from alphapose.utils.config import edict
    cfg = edict({"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50})
    preset = edict({"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]})
    torch.manual_seed(seed)
    m = builder.build_sppe(cfg, preset_cfg=preset)                         # default initialisation under the seed
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=gen) + 0.5)
                mod.bias.copy_(0.2 * torch.randn(mod.bias.shape, generator=gen))
    return m


def _bn_names(mod):
    return [k for k, b in mod.named_modules() if isinstance(b, torch.nn.BatchNorm2d)]


def _host_run(sd, x, cot, dtype, blocks=None):
    """The step on the host in ``dtype`` -> gradients, heat-maps (or trunk output), batch statistics and updated running statistics."""
    ref = nets.SimplePoseRef(50)
    ref.load_state_dict(sd, strict=True)
    ref = ref.to(dtype).train()
    batch, hooks = {}, []
    for k, b in ref.named_modules():
        if isinstance(b, torch.nn.BatchNorm2d):
            hooks.append(b.register_forward_hook(
                lambda mod, inp, out, k=k: batch.__setitem__(k, (inp[0].detach().mean((0, 2, 3)).double(), inp[0].detach().var((0, 2, 3), unbiased=False).double()))))   # in the run's own precision
    xin = torch.from_numpy(x).to(dtype)
    out = ref(xin) if blocks is None else TC.simulate_trunk(ref, xin, None, blocks)
    (out * cot.to(dtype)).sum().backward()
    for h in hooks:
        h.remove()
    mods = dict(ref.named_modules())
    return dict(grads={k: p.grad.double().clone() for k, p in ref.named_parameters() if p.grad is not None}, out=out.detach().double(),
                mean={k: v[0] for k, v in batch.items()}, var={k: v[1] for k, v in batch.items()},
                running_mean={k: mods[k].running_mean.double().clone() for k in batch}, running_var={k: mods[k].running_var.double().clone() for k in batch})


def _err(a, ref):
    return float((a - ref).abs().max() / ref.abs().max())


def _judge(tag, items):
    """items: [(name, device tensor, float64 host tensor, fp32 host tensor)] -> asserts the gate on every one of them and records the figures."""
    bad, es, e32s, ratios = [], [], [], []
    for name, got, t64, t32 in items:
        got = got.reshape(t64.shape)
        if float(t64.abs().max()) == 0.0:
            if float(got.abs().max()) != 0.0:
                bad.append((name, "nonzero where float64 is identically zero"))
            continue
        e, e32 = _err(got, t64), _err(t32, t64)
        es.append(e), e32s.append(e32), ratios.append(e / e32 if e32 > 0 else np.inf)
        if not (np.isfinite(e) and e <= GATE * e32):
            bad.append((name, e, e32))
    q = lambda v: (float(np.min(v)), float(np.median(v)), float(np.max(v)))
    record(f"train_f64_{tag}", tensors=len(items), e_min_med_max=q(es), e32_min_med_max=q(e32s), ratio_min_med_max=q(ratios), gate=GATE)
    print(f"{tag}: {len(items)} tensors, e {q(es)}, e32 {q(e32s)}, e/e32 {q(ratios)} (gate {GATE:.3e})")
    assert not bad, (tag, len(bad), bad[:10])


@pytest.fixture(scope="module")
def step(vh):
    """The device step (twice, from one state) and the two host runs, computed once; the model's state before and after."""
    from alphapose.models import hip_train_f64
    m = _model(5)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = synth.crops(3, seed=61, hw=HW)
    cot = torch.randn((3, 17, HW[0] // 4, HW[1] // 4), generator=torch.Generator().manual_seed(62)).double() * 2.0 ** -14    # fp32 values scaled by a power of two: every run gets the same cotangent
    host = {name: _host_run(sd, x, cot, dt) for name, dt in (("f64", torch.float64), ("f32", torch.float32))}
    m = m.to(dev()).train()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    passes = []
    for _ in range(2):
        tr = hip_train_f64.trainer_for_f64(m)
        out = tr.forward(to_dev(x))
        grads = tr.backward(cot.to(dev()))
        stats = tr.batch_statistics()
        torch.cuda.synchronize()
        passes.append((out, grads, stats))
    return dict(m=m, x=x, cot=cot, sd=sd, host=host, before=before, passes=passes)


def test_every_parameter_gradient_against_float64_autograd(step):
    m, (out, grads, _), f64, f32 = step["m"], step["passes"][0], step["host"]["f64"], step["host"]["f32"]
    named = dict(m.named_parameters())
    assert len(named) == 170 and set(named) == set(f64["grads"]) and all(p in grads for p in named.values()) and len(grads) == 170
    for k, p in named.items():
        assert grads[p].dtype == torch.float64 and grads[p].shape == p.shape, k
    _judge("step_gradients", [(k, grads[p].cpu(), f64["grads"][k], f32["grads"][k]) for k, p in named.items()])


def test_heat_maps_and_batch_statistics(step):
    m, (out, _, stats), f64, f32 = step["m"], step["passes"][0], step["host"]["f64"], step["host"]["f32"]
    assert out.dtype == torch.float64 and tuple(out.shape) == (3, 17, HW[0] // 4, HW[1] // 4)
    _judge("step_heatmaps", [("heatmaps", out.cpu(), f64["out"], f32["out"])])
    mods = dict(m.named_modules())
    names = _bn_names(m)
    assert len(names) == 56 and set(names) == set(f64["mean"]) and {mods[k] for k in names} == set(stats)
    items = [(f"{k}.{what}", stats[mods[k]][what].cpu(), f64[what][k], f32[what][k]) for k in names for what in ("mean", "var", "running_mean", "running_var")]
    _judge("step_statistics", items)


def test_the_model_is_not_touched(step):
    m = step["m"]
    after = m.state_dict()
    assert set(after) == set(step["before"]) and any(k.endswith("num_batches_tracked") for k in after)
    for k, v in step["before"].items():
        assert torch.equal(after[k], v), k
    assert all(p.grad is None for p in m.parameters())
    assert not any("f64" in k for k in m.__dict__)


def test_two_passes_from_one_state_are_bit_equal(step):
    (o1, g1, s1), (o2, g2, s2) = step["passes"]
    assert torch.equal(o1, o2) and float(o1.abs().sum()) > 0
    assert set(g1) == set(g2) and all(torch.equal(g1[p], g2[p]) for p in g1)
    assert all(torch.equal(s1[b][w], s2[b][w]) for b in s1 for w in s1[b])


def test_shallow_prefix(vh):
    """Stem, max-pool and four bottlenecks (the projection block, the stride-2 block with its per-phase data gradients, the skip gradient
    riding in conv1's write-out) at B = 4 on 64x48 with a fixed cotangent: the same gate on its 45 parameter tensors and its output."""
    from alphapose.models import hip_train_f64
    m = _model(11)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = synth.crops(4, seed=101, hw=(64, 48))
    cot = torch.randn((4, 512, 8, 6), generator=torch.Generator().manual_seed(13)).double()
    f64, f32 = (_host_run(sd, x, cot, dt, SHALLOW_BLOCKS) for dt in (torch.float64, torch.float32))
    m = m.to(dev()).train()
    tr = hip_train_f64.trainer_for_f64(m)
    y = tr.trunk_forward(to_dev(x), SHALLOW_BLOCKS)
    assert y.dtype == torch.float64 and tuple(y.shape) == (4, 8, 6, 512)
    grads = {}
    tr.trunk_backward(cot.permute(0, 2, 3, 1).contiguous().to(dev()), grads)
    torch.cuda.synchronize()
    named = dict(m.named_parameters())
    assert {k for k, p in named.items() if p in grads} == set(f64["grads"]) and len(f64["grads"]) == 45
    _judge("shallow_gradients", [(k, grads[named[k]].cpu(), g, f32["grads"][k]) for k, g in f64["grads"].items()])
    _judge("shallow_output", [("trunk_output", y.cpu().permute(0, 3, 1, 2), f64["out"], f32["out"])])


def test_fp32_trainer_is_as_far_from_the_device_reference_as_from_the_host_reference(step):
    """The yardstick in use: the fp32 trainer's per-tensor distance from the DEVICE float64 gradients and from the HOST float64 gradients
    agree to 1e-6 relative of the distance itself on every tensor."""
    import copy
    from alphapose.models import hip_train
    m2 = copy.deepcopy(step["m"]).train()                                  # hip_train updates the running statistics of the model it trains
    tr = hip_train.trainer_for(m2)
    with torch.no_grad():
        tr.forward(to_dev(step["x"]))
        g32 = tr.backward(step["cot"].float().to(dev()))
    torch.cuda.synchronize()
    g32 = {k: g32[p].detach().cpu().double() for k, p in m2.named_parameters()}
    gdev = {k: step["passes"][0][1][p].cpu() for k, p in step["m"].named_parameters()}
    bad, worst = [], 0.0
    for k, g64 in step["host"]["f64"]["grads"].items():
        d_dev, d_host = _err(g32[k].reshape(g64.shape), gdev[k]), _err(g32[k].reshape(g64.shape), g64)
        rel = abs(d_dev - d_host) / d_host
        worst = max(worst, rel)
        if not rel <= 1e-6:
            bad.append((k, d_dev, d_host))
    record("train_f64_yardstick_agreement", worst_relative_difference=worst, tensors=len(g32))
    print(f"fp32 trainer: distance from the device / host float64 gradients differ by at most {worst:.3e} of the distance")
    assert len(g32) == 170 and not bad, (len(bad), bad[:10])


def test_refusals_hold_on_the_device(vh):
    from alphapose.models import builder, hip_train_f64
    from alphapose.utils.config import edict
    preset = edict({"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]})
    fp = builder.build_sppe(edict({"TYPE": "FastPose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50}), preset_cfg=preset).to(dev())
    with pytest.raises(NotImplementedError, match="FastPose"):
        hip_train_f64.trainer_for_f64(fp)
    from tests.test_train_f64_cpu import HRNET
    hr = builder.build_sppe(edict(HRNET), preset_cfg=preset).to(dev())
    with pytest.raises(NotImplementedError, match="HRNet"):
        hip_train_f64.trainer_for_f64(hr)
    sp = _model(2)
    sp.preact.layer4[2] = torch.nn.Identity()                              # a block without conv3 stands for a BasicBlock trunk (the package builds none)
    with pytest.raises(NotImplementedError, match="BasicBlock"):
        hip_train_f64.trainer_for_f64(sp.to(dev()))
    tr = hip_train_f64.trainer_for_f64(_model(3).to(dev()).train())
    with pytest.raises(vh.VatlError):
        tr.forward(torch.zeros(1, 3, 64, 48))                              # a CPU tensor
    with pytest.raises(vh.VatlError):
        tr.forward(torch.zeros(1, 3, 64, 48, device=dev(), dtype=torch.float16))
