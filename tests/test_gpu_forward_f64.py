"""The float64 reference forward on the device (alphapose/models/hip_engine_f64.py) against the oracle graphs run in float64 with torch
on the host: single blocks first (they localise a failure), then the three 256x192 networks on 8 seeded crops.

The bar on the normwise distance, `tests.gpu_util.rel_err <= 1e-11`, is reasoned, not tuned: the fp32 routes measure 1.2e-6 to 6.3e-6
against float64 on these networks (profiles/r06_widepin_parity.jsonl); scaled by the ratio of the unit round-offs, 2^-53 / 2^-24 =
1.9e-9, that predicts about 1e-14 for two float64 evaluations that differ in summation order only.  The bar stands three orders above
that prediction and five below anything a single fp32 layer could reach, so it fails if any layer silently runs in fp32.  The measured
values are recorded (`tests.gpu_util.record`) and quoted in profiles/f64_reference_notes.md.

Last, the device reference as the yardstick of the existing claim: on the same crops it must single out exactly the planes of the timed
fp32 route that the host float64 oracle singles out, and measure the same distance to it.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import nets, synth
from tests.gpu_util import dev, record, rel_err, to_dev
from tests.test_gpu_widepin import CASES, _build

pytestmark = pytest.mark.gpu

BAR = 1e-11
NETS = ["simplepose_r50", "fastpose_r50", "hrnet_w32"]
N_CROPS = 8


@pytest.fixture(scope="module")
def f64():
    import vatl_hip
    vatl_hip.lib()
    from alphapose.models import hip_engine_f64
    return hip_engine_f64


def _pair(prod, ref):
    """Seeded weights into the product module (device, eval) and the oracle graph (host, float64, eval)."""
    sd = synth.state_dict_for(prod)
    prod.load_state_dict(sd, strict=True)
    ref.load_state_dict(sd, strict=True)
    return prod.to(dev()).eval(), ref.double().eval()


def _x(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape))             # float64 values fp32 cannot hold


# ----------------------------------------------------------------------------------------------------------------------- blocks
def test_se_bottleneck_with_projection(f64):
    """64 -> 32 -> 128, stride 2, on 8x6 planes: three convs, the projection, the pooled gate through two Linear layers, scale + skip + ReLU."""
    from alphapose.models.layers.SE_Resnet import Bottleneck
    proj = nn.Sequential(nn.Conv2d(64, 128, kernel_size=1, stride=2, bias=False), nn.BatchNorm2d(128))
    blk, ref = _pair(Bottleneck(64, 32, 2, proj, reduction=True), nets._SEBneck(64, 32, 2, True))
    x = _x(41, 3, 64, 8, 6)
    with torch.no_grad():
        want = ref(x)
    got = f64.features_f64(blk, x.to(dev()))
    assert got.dtype == torch.float64 and got.shape == want.shape == (3, 128, 4, 3)
    e = rel_err(got.cpu(), want)
    record("f64_block_se_bottleneck", rel=e)
    assert e <= BAR, e
    got32 = f64.features_f64(blk, x.float().to(dev()))                                      # fp32 input: converted exactly
    with torch.no_grad():
        assert rel_err(got32.cpu(), ref(x.float().double())) <= BAR


def test_two_branch_high_resolution_module(f64):
    """32 / 64 channels on 8x8 and 4x4 planes: BasicBlocks, the strided fuse path through the residual input, 1x1 + nearest up-sampling + add."""
    from alphapose.models.hrnet import BasicBlock, HighResolutionModule
    mod, ref = _pair(HighResolutionModule(2, BasicBlock, [2, 2], [32, 64], [32, 64], "SUM"), nets._HRModule((32, 64), [2, 2]))
    xs = [_x(42, 2, 32, 8, 8), _x(43, 2, 64, 4, 4)]
    with torch.no_grad():
        want = ref(xs)
    got = f64.features_f64(mod, [t.to(dev()) for t in xs])
    assert len(got) == len(want) == 2
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == torch.float64
        e = rel_err(g.cpu(), w)
        record(f"f64_block_hr_module_branch{i}", rel=e)
        assert e <= BAR, (i, e)


def test_duc(f64):
    """conv 3x3 + BatchNorm + ReLU + PixelShuffle(2), 16 -> 32 channels on 4x3 planes."""
    from alphapose.models.layers.DUC import DUC
    duc, ref = _pair(DUC(16, 32), nets._DUC(16, 32))
    x = _x(44, 3, 16, 4, 3)
    with torch.no_grad():
        want = ref(x)
    got = f64.features_f64(duc, x.to(dev()))
    assert got.shape == want.shape == (3, 8, 8, 6)
    e = rel_err(got.cpu(), want)
    record("f64_block_duc", rel=e)
    assert e <= BAR, e


# --------------------------------------------------------------------------------------------------------------- whole networks
@functools.lru_cache(maxsize=None)
def _case(name):
    """Per network, computed once and shared: the model, the crops, the host float64 heat-maps and pooled trunk output."""
    m = _build(name)
    x = synth.crops(N_CROPS, seed=4242, hw=CASES[name][1])
    ref = {"simplepose_r50": lambda: nets.SimplePoseRef(50), "fastpose_r50": lambda: nets.FastPoseRef(50), "hrnet_w32": lambda: nets.HRNetRef()}[name]()
    ref.load_state_dict(synth.state_dict_for(m), strict=True)
    ref = ref.double().eval()
    kept = {}
    if hasattr(ref, "preact"):                                                              # get_embedding's input, from the SAME trunk pass
        ref.preact.register_forward_hook(lambda mod, inp, out: kept.__setitem__("trunk", out))
    with torch.no_grad():
        h64 = ref(torch.from_numpy(x).double())
        emb = torch.flatten(F.adaptive_avg_pool2d(kept["trunk"], 1), 1).numpy() if kept else None
    return m, x, h64.numpy(), emb


@functools.lru_cache(maxsize=None)
def _device_f64(name):
    from alphapose.models import hip_engine_f64
    m, x, _, _ = _case(name)
    got = hip_engine_f64.forward_f64(m, to_dev(x))
    torch.cuda.synchronize()
    return got


def _argmax(h):
    return np.asarray(h).reshape(h.shape[0], h.shape[1], -1).argmax(2)


@pytest.mark.parametrize("name", NETS)
def test_forward_f64_matches_the_host_float64_oracle(f64, name):
    m, x, h64, _ = _case(name)
    got = _device_f64(name)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == h64.shape == (N_CROPS, 17) + CASES[name][2]
    g = got.cpu().numpy()
    e = rel_err(g, h64)
    moved = int((_argmax(g) != _argmax(h64)).sum())
    record(f"f64_forward_{name}", rel=e, planes=N_CROPS * 17, moved=moved)
    print(f"{name}: rel_err(device float64, host float64) = {e:.3e}, arg-max moved on {moved} of {N_CROPS * 17} planes")
    assert e <= BAR, e
    assert moved == 0
    # float64 crops, a preallocated output, another batching: the same bits
    out = torch.empty_like(got)
    assert f64.forward_f64(m, to_dev(x).double(), out=out) is out and torch.equal(out, got)
    assert torch.equal(f64.forward_f64(m, to_dev(x[5:7])), got[5:7])


@pytest.mark.parametrize("name", ["simplepose_r50", "fastpose_r50"])
def test_embedding_f64_matches_the_host_float64_oracle(f64, name):
    m, x, _, emb = _case(name)
    got = f64.embedding_f64(m, to_dev(x))
    assert got.dtype == torch.float64 and tuple(got.shape) == emb.shape == (N_CROPS, 2048)
    e = rel_err(got.cpu().numpy(), emb)
    record(f"f64_embedding_{name}", rel=e)
    assert e <= BAR, e


@pytest.mark.parametrize("name", NETS)
def test_device_reference_judges_the_timed_route_like_the_host_oracle(f64, name):
    """Same flipped planes, same distance: the device reference can stand in for the host's wherever the fp32 routes are judged."""
    from alphapose.models import hip_engine
    m, x, h64, _ = _case(name)
    d64 = _device_f64(name).cpu().numpy()
    hm = torch.empty((N_CROPS, 17) + CASES[name][2], device=dev())
    with torch.no_grad():
        hip_engine.forward_into(m, to_dev(x), hm)
    torch.cuda.synchronize()
    hm = hm.cpu().numpy()
    i32 = _argmax(hm)
    assert np.array_equal(i32 != _argmax(d64), i32 != _argmax(h64))
    e_dev, e_host = rel_err(hm, d64), rel_err(hm, h64)
    record(f"f64_yardstick_{name}", route_vs_device_f64=e_dev, route_vs_host_f64=e_host, flipped=int((i32 != _argmax(d64)).sum()))
    assert e_dev < 1e-4
    assert abs(e_dev - e_host) <= 1e-9 * e_host, (e_dev, e_host)
