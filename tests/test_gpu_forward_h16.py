"""The opt-in 16-bit forward on the device (alphapose/models/hip_engine_h16.py), float16 and bfloat16, judged by the ROUNDING
SIMULATION of tests/h16_cases.py: the oracle graph in float64 on the host with the input, every conv / deconv / linear weight and every
BatchNorm2d / ReLU / MaxPool2d / PixelShuffle output rounded to the storage type T.

    q = rel_err(simulation, float64 oracle)        what storing in T costs, with exact arithmetic in between
    e = rel_err(route,      float64 oracle)

Gate: e <= 3 q — the margin tests/test_gpu_pose_pretrain.py gives its trajectory.  The route and the simulation are two realisations of
the same per-layer roundings, not the same one (the route rounds a block's output once after the skip is added, the simulation rounds
the BatchNorm before it), so e / q near 1 is what a correct route gives; a missing fp32 accumulation, a wrong fold or a dropped residual
lands orders above 3.  An arg-max may move in either (the simulation itself moves one on these crops): `moved` is recorded, not asserted.

Blocks first (they localise a failure), at the float64 test's block shapes, then the three 256x192 networks on two seeded crops.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import nets, synth
from tests import h16_cases as HC
from tests.gpu_util import dev, record, rel_err, to_dev
from tests.test_gpu_widepin import CASES, _build

pytestmark = pytest.mark.gpu

NETS = ["simplepose_r50", "fastpose_r50", "hrnet_w32"]
TYPES = list(HC.DTYPES)
N_CROPS = 2
MARGIN = 3.0


@pytest.fixture(scope="module")
def h16():
    import vatl_hip
    vatl_hip.lib()
    from alphapose.models import hip_engine_h16
    return hip_engine_h16


def _pair(prod, ref):
    """Seeded weights into the product module (device, eval) and the oracle graph (host, float64, eval)."""
    sd = synth.state_dict_for(prod)
    prod.load_state_dict(sd, strict=True)
    ref.load_state_dict(sd, strict=True)
    return prod.to(dev()).eval(), ref.double().eval()


def _x(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def _gate(tag, got, want, sim):
    e, q = rel_err(got, want), rel_err(sim, want)
    record(tag, e=e, q=q, e_over_q=e / q)
    print(f"{tag}: e = {e:.3e}, q = {q:.3e}, e / q = {e / q:.2f}")
    assert np.isfinite(np.asarray(got)).all()
    assert q > 0 and e <= MARGIN * q, (tag, e, q)


# ----------------------------------------------------------------------------------------------------------------------- blocks
@pytest.mark.parametrize("tname", TYPES)
def test_se_bottleneck_with_projection(h16, tname):
    """64 -> 32 -> 128, stride 2, on 8x6 planes: three convs, the projection, the pooled gate through two Linear layers, scale + skip + ReLU."""
    from alphapose.models.layers.SE_Resnet import Bottleneck
    dt = HC.DTYPES[tname][0]
    proj = nn.Sequential(nn.Conv2d(64, 128, kernel_size=1, stride=2, bias=False), nn.BatchNorm2d(128))
    blk, ref = _pair(Bottleneck(64, 32, 2, proj, reduction=True), nets._SEBneck(64, 32, 2, True))
    x = _x(41, 3, 64, 8, 6)
    with torch.no_grad():
        want = ref(x.double())
    got = h16.features_h16(blk, x.to(dev()), dtype=dt)
    assert got.dtype == torch.float32 and got.shape == want.shape == (3, 128, 4, 3)
    _gate(f"h16_block_se_bottleneck_{tname}", got.cpu().numpy(), want.numpy(), HC.simulate(ref, x, dt).numpy())


@pytest.mark.parametrize("tname", TYPES)
def test_two_branch_high_resolution_module(h16, tname):
    """32 / 64 channels on 8x8 and 4x4 planes: BasicBlocks, the strided fuse path through the residual input, 1x1 + nearest up-sampling + add."""
    from alphapose.models.hrnet import BasicBlock, HighResolutionModule
    dt = HC.DTYPES[tname][0]
    mod, ref = _pair(HighResolutionModule(2, BasicBlock, [2, 2], [32, 64], [32, 64], "SUM"), nets._HRModule((32, 64), [2, 2]))
    xs = [_x(42, 2, 32, 8, 8), _x(43, 2, 64, 4, 4)]
    with torch.no_grad():
        want = ref([t.double() for t in xs])
    sim = HC.simulate(ref, xs, dt)
    got = h16.features_h16(mod, [t.to(dev()) for t in xs], dtype=dt)
    assert len(got) == len(want) == 2
    for i, (g, w, s) in enumerate(zip(got, want, sim)):
        assert g.shape == w.shape and g.dtype == torch.float32
        _gate(f"h16_block_hr_module_branch{i}_{tname}", g.cpu().numpy(), w.numpy(), s.numpy())


@pytest.mark.parametrize("tname", TYPES)
def test_duc(h16, tname):
    """conv 3x3 + BatchNorm + ReLU + PixelShuffle(2), 16 -> 32 channels on 4x3 planes."""
    from alphapose.models.layers.DUC import DUC
    dt = HC.DTYPES[tname][0]
    duc, ref = _pair(DUC(16, 32), nets._DUC(16, 32))
    x = _x(44, 3, 16, 4, 3)
    with torch.no_grad():
        want = ref(x.double())
    got = h16.features_h16(duc, x.to(dev()), dtype=dt)
    assert got.shape == want.shape == (3, 8, 8, 6)
    _gate(f"h16_block_duc_{tname}", got.cpu().numpy(), want.numpy(), HC.simulate(ref, x, dt).numpy())


# --------------------------------------------------------------------------------------------------------------- whole networks
def _oracle(name):
    return {"simplepose_r50": lambda: nets.SimplePoseRef(50), "fastpose_r50": lambda: nets.FastPoseRef(50), "hrnet_w32": lambda: nets.HRNetRef()}[name]()


@functools.lru_cache(maxsize=None)
def _case(name):
    """Per network, computed once and shared: the model, the crops, the oracle graph, its float64 heat-maps and pooled trunk output."""
    m = _build(name)
    x = synth.crops(N_CROPS, seed=4242, hw=CASES[name][1])
    ref = _oracle(name)
    ref.load_state_dict(synth.state_dict_for(m), strict=True)
    ref = ref.double().eval()
    kept = {}
    handle = ref.preact.register_forward_hook(lambda mod, inp, out: kept.__setitem__("trunk", out)) if hasattr(ref, "preact") else None
    with torch.no_grad():
        h64 = ref(torch.from_numpy(x).double())
        emb = torch.flatten(F.adaptive_avg_pool2d(kept["trunk"], 1), 1).numpy() if kept else None
    if handle is not None:
        handle.remove()
    return m, x, ref, h64.numpy(), emb


@functools.lru_cache(maxsize=None)
def _simulated(name, tname):
    """Heat-maps and pooled trunk output of the rounding simulation, once per network and type."""
    m, x, ref, _, emb = _case(name)
    dt = HC.DTYPES[tname][0]
    if emb is None:
        return HC.simulate(ref, torch.from_numpy(x), dt).numpy(), None
    hm, trunk = HC.simulate(ref, torch.from_numpy(x), dt, keep="preact")
    return hm.numpy(), torch.flatten(F.adaptive_avg_pool2d(trunk, 1), 1).numpy()


@functools.lru_cache(maxsize=None)
def _device(name, tname):
    from alphapose.models import hip_engine_h16
    m, x, _, _, _ = _case(name)
    got = hip_engine_h16.forward_h16(m, to_dev(x), dtype=HC.DTYPES[tname][0])
    torch.cuda.synchronize()
    return got


def _argmax(h):
    return np.asarray(h).reshape(h.shape[0], h.shape[1], -1).argmax(2)


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("name", NETS)
def test_forward_h16_within_the_rounding_simulations_margin(h16, name, tname):
    m, x, _, h64, _ = _case(name)
    dt = HC.DTYPES[tname][0]
    got = _device(name, tname)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == h64.shape == (N_CROPS, 17) + CASES[name][2]
    g, sim = got.cpu().numpy(), _simulated(name, tname)[0]
    e, q = rel_err(g, h64), rel_err(sim, h64)
    moved, moved_sim = int((_argmax(g) != _argmax(h64)).sum()), int((_argmax(sim) != _argmax(h64)).sum())
    record(f"h16_forward_{name}_{tname}", e=e, q=q, e_over_q=e / q, planes=N_CROPS * 17, moved=moved, moved_simulation=moved_sim)
    print(f"{name} {tname}: e = {e:.3e}, q = {q:.3e}, e / q = {e / q:.2f}; arg-max moved on {moved} (route) / {moved_sim} (simulation) of {N_CROPS * 17} planes")
    assert np.isfinite(g).all()
    assert q > 0 and e <= MARGIN * q, (e, q)
    # another batching, a preallocated output: the same bits
    assert torch.equal(h16.forward_h16(m, to_dev(x[1:2]), dtype=dt), got[1:2])
    out = torch.empty_like(got)
    assert h16.forward_h16(m, to_dev(x), out=out, dtype=dt) is out and torch.equal(out, got)


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("name", ["simplepose_r50", "fastpose_r50"])
def test_heatmaps_and_embedding_from_one_trunk_pass(h16, name, tname):
    m, x, _, _, emb64 = _case(name)
    dt = HC.DTYPES[tname][0]
    got = _device(name, tname)
    out, emb = torch.empty_like(got), torch.empty((N_CROPS, 2048), device=dev())
    assert h16.forward_with_embedding_h16(m, to_dev(x), out, emb, dtype=dt) is None
    assert torch.equal(out, got)
    assert emb.dtype == torch.float32 and torch.equal(emb, h16.embedding_h16(m, to_dev(x), dtype=dt))
    _gate(f"h16_embedding_{name}_{tname}", emb.cpu().numpy(), emb64, _simulated(name, tname)[1])


# --------------------------------------------------------------------------------------------------------------------- refusals
def test_what_the_route_does_not_serve_is_refused_loudly(h16):
    import vatl_hip as vh
    from alphapose.models import builder
    from alphapose.utils.config import edict
    m, x, _, _, _ = _case("simplepose_r50")
    xd = to_dev(x)
    with pytest.raises(vh.VatlError, match="float16"):
        h16.forward_h16(m, xd, dtype=torch.float32)
    with pytest.raises(vh.VatlError, match="MI355X"):
        h16.forward_h16(m, torch.from_numpy(x))
    with pytest.raises(vh.VatlError, match="MI355X"):
        h16.embedding_h16(m, torch.from_numpy(x))
    m.train()
    try:
        with pytest.raises(vh.VatlError, match="eval"):
            h16.forward_h16(m, xd)
    finally:
        m.eval()
    preset = edict({"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]})
    dcn = builder.build_sppe(edict({"TYPE": "FastPose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50,
                                    "DCN": {"MODULATED": False, "DEFORM_GROUP": 1, "FALLBACK_ON_STRIDE": False}, "STAGE_WITH_DCN": [False, True, True, True]}),
                             preset_cfg=preset).to(dev()).eval()
    for fn in (h16.forward_h16, h16.embedding_h16):
        with pytest.raises(NotImplementedError, match="DCN"):
            fn(dcn, xd)
