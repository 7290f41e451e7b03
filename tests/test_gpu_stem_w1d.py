"""The ResNet stem with a 1-D Winograd transform along the image rows (csrc/stem_pool_w1d.hip: F(2,4) on the odd pixels + F(2,3) on the even pixels): the packed
filter against a float64 restatement, the layer against float64 and against csrc/stem_pool.hip, borders that are zeros and not neighbours, bits independent of
batch position and band cut, the sizes it refuses, and the SimplePose-R50 plan with the route on and off.  (The network-level accuracy probe that preceded the
kernel: tests/probes/stem_w1d_accuracy.py.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import dev, record, rel_err, to_dev

pytestmark = pytest.mark.gpu

TOL = 2e-5      # max|err| / max|ref| per layer: the project's layer bar (tests/test_gpu_conv.py)

G4 = np.array([[0.5, 0, 0, 0], [0.5, 0.5, 0.5, 0.5], [1 / 6, -1 / 6, 1 / 6, -1 / 6], [1 / 6, 1 / 3, 2 / 3, 4 / 3], [0, 0, 0, 1.0]])    # F(2,4), points 0 1 -1 2 inf
G3 = np.array([[1.0, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1.0]])                                                      # F(2,3), points 0 1 -1 inf


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


@pytest.fixture(scope="module")
def stem(vh):
    """Filter and folded BatchNorm of tests/test_gpu_conv.py's stem test (seed 41), both packings."""
    g = torch.Generator(device="cpu").manual_seed(41)
    w = (torch.randn((64, 3, 7, 7), generator=g) * (2.0 / 147) ** 0.5)
    sc = torch.rand(64, generator=g) + 0.5
    bi = torch.randn(64, generator=g) * 0.5
    wd = w.to(dev())
    return {"w": w, "sc": sc, "bi": bi, "scd": sc.to(dev()), "bid": bi.to(dev()), "pw": vh.pack_stem_pool_weight(wd), "u1d": vh.pack_stem_pool_w1d_weight(wd), "g": g}


def _ref64(s, x):
    ref = F.conv2d(x.double(), s["w"].double(), None, 2, 3) * s["sc"].double().view(1, -1, 1, 1) + s["bi"].double().view(1, -1, 1, 1)
    return F.max_pool2d(ref.clamp_min(0), 3, 2, 1).permute(0, 2, 3, 1).numpy()


def _new(vh, s, x):
    return vh.stem_pool_fwd(x, s["pw"], s["scd"], s["bid"], u1d=s["u1d"])


def _old(vh, s, x):
    return vh.stem_pool_fwd(x, s["pw"], s["scd"], s["bid"])


def test_packed_filter_matches_a_float64_restatement(vh):
    r = np.random.RandomState(7)
    w = r.standard_normal((64, 3, 7, 7)).astype(np.float32)
    u = vh.pack_stem_pool_w1d_weight(to_dev(w)).cpu().numpy()
    assert u.size == int(vh.lib().vatl_stem_pool_w1d_weight_floats()) == 4 * 9 * 6 * 64
    w64 = w.astype(np.float64)
    U = np.concatenate([np.einsum("pi,ncki->pnkc", G4, w64[..., 0::2]), np.einsum("pi,ncki->pnkc", G3, w64[..., 1::2])], 0)       # position, n, ky, c
    U = np.concatenate([U.reshape(9, 64, 21), np.zeros((9, 64, 3))], 2)                                                        # kk = 3 ky + c, padded to 24
    # [n / 16][position][k-step = kk / 4][lane = 16 (kk % 4) + n % 16]
    ref = np.transpose(U.reshape(9, 4, 16, 6, 4), (1, 0, 3, 4, 2)).reshape(-1)
    # both sides round a float64 value once; the float64 values differ by summation order only, so the float32 results differ by at most one unit in the last place
    d = np.abs(u.astype(np.float64) - ref)
    assert (d <= 2.0 ** -23 * np.abs(ref) + 1e-12).all(), float(d.max())
    assert (u == ref.astype(np.float32)).mean() > 0.99
    pad = u.reshape(4, 9, 6, 4, 16)[:, :, 5, 1:, :]              # entries 21, 22, 23 (the 22nd entry and the two that fill the last k-step)
    assert np.abs(pad).max() == 0.0
    assert np.abs(u.reshape(4, 9, 6, 4, 16)[:, :, 5, 0, :]).min() > 0.0     # entry 20 = (ky 6, c 2) is a real one


SHAPES = [
    (1, 8, 192),        # two pooled rows, top and bottom borders in one step
    (3, 32, 192),       # two bands: the recomputed row above a band
    (2, 64, 192),       # four bands
    (600, 16, 192),     # one band, more blocks than slots
    (3, 256, 192),      # the flagship's crops
    (5, 32, 64),        # the further widths the rule admits: one unit of 16 tiles per row ...
    (3, 64, 128),       # ... and two, with a padded channel stride
]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_layer_matches_float64_and_the_direct_stem(vh, stem, shape):
    n, h, wdt = shape
    assert vh.stem_pool_w1d_supported(h, wdt) and vh.stem_pool_supported(h, wdt)
    x = torch.rand((n, 3, h, wdt), generator=torch.Generator(device="cpu").manual_seed(n * 1000 + h + wdt)) - 0.45
    xd = x.to(dev())
    with vh.flop_meter() as fm:
        got = _new(vh, stem, xd)
    assert fm.routes["stem_pool_w1d"] == 1 and fm.routes["stem_pool"] == 0 and sum(fm.routes.values()) == 1, fm.routes
    ph = h // 4
    bands = 1
    while n * bands < 512 and bands * 2 <= ph // 4:
        bands *= 2
    assert fm.direct == 2.0 * n * (ph + bands - 1) * 2 * (wdt // 4) * 9 * 24 * 64 and fm.direct_launches == 1 and fm.winograd_launches == 0
    assert got.shape == (n, h // 4, wdt // 4, 64)
    k = min(n, 3)
    ref = _ref64(stem, torch.cat([x[:k], x[n - 1:]]))
    e = rel_err(torch.cat([got[:k], got[n - 1:]]).cpu().numpy(), ref)
    with vh.flop_meter() as fo:
        old = _old(vh, stem, xd)
    assert fo.routes["stem_pool"] == 1 and fo.routes["stem_pool_w1d"] == 0, fo.routes
    eo = rel_err(got.cpu().numpy(), old.cpu().numpy())
    print(f"stem_w1d {shape}: vs float64 {e:.3e}  direct stem vs float64 {rel_err(old[:k].cpu().numpy(), ref[:k]):.3e}  vs direct stem {eo:.3e}")
    record("stem_w1d_" + "x".join(map(str, shape)), rel=e, vs_direct=eo)
    assert e < TOL, (shape, e)
    assert eo < TOL and not torch.equal(got, old), (shape, eo)
    # bits: an image alone (another band cut) and at another batch position
    solo = _new(vh, stem, xd[n - 1:n].contiguous())
    assert torch.equal(solo[0], got[n - 1])
    if n > 1:
        swapped = _new(vh, stem, torch.flip(xd, (0,)).contiguous())
        assert torch.equal(swapped[0], got[n - 1]) and torch.equal(swapped[n - 1], got[0])


def test_borders_are_zeros_not_neighbours(vh, stem):
    ones = torch.ones((2, 3, 32, 192))
    edge = (torch.rand((2, 3, 32, 192), generator=torch.Generator(device="cpu").manual_seed(3)) - 0.5) * 0.1
    big = torch.where(torch.rand((2, 3, 32, 192), generator=torch.Generator(device="cpu").manual_seed(4)) < 0.5, -100.0, 100.0)
    frame = torch.zeros((32, 192), dtype=torch.bool)
    frame[:2] = frame[-2:] = True
    frame[:, :2] = frame[:, -2:] = True
    edge = torch.where(frame, big, edge)
    for name, x in (("ones", ones), ("edge", edge)):
        got = _new(vh, stem, x.to(dev()))
        e = rel_err(got.cpu().numpy(), _ref64(stem, x))
        print(f"stem_w1d borders {name}: vs float64 {e:.3e}")
        assert e < TOL, (name, e)
    # a border test that is wrong reads a neighbouring image; NaN does not hide behind a zero product
    x = (torch.rand((3, 3, 32, 192), generator=torch.Generator(device="cpu").manual_seed(5)) - 0.45).to(dev())
    full = _new(vh, stem, x)
    xn = x.clone()
    xn[0] = float("nan")
    xn[2] = float("nan")
    poisoned = _new(vh, stem, xn)
    assert torch.isfinite(full).all() and torch.equal(poisoned[1], full[1])
    out = torch.full((3, 8, 48, 64), -7.0, device=dev())
    y = vh.stem_pool_fwd(x, stem["pw"], stem["scd"], stem["bid"], out=out, u1d=stem["u1d"])
    assert y.data_ptr() == out.data_ptr() and torch.equal(out, full)


def test_refused_sizes_fall_back_to_the_direct_stem(vh, stem):
    assert not vh.stem_pool_w1d_supported(384, 288) and not vh.stem_pool_w1d_supported(256, 200) and not vh.stem_pool_w1d_supported(258, 192)
    for h, wdt in ((384, 288), (256, 200), (258, 192)):
        with pytest.raises(vh.VatlError):
            vh.stem_pool_w1d_fwd(torch.zeros((1, 3, h, wdt), device=dev()), stem["u1d"], stem["scd"], stem["bid"])
    # stem_pool_fwd with the keyword goes to the direct stem on a refused size.  Both kernels serve the same sizes (W in {64, 128, 192}, H % 4 == 0), so what
    # comes back there is the direct stem's own refusal, word for word, and the new kernel is not launched
    for h, wdt in ((384, 288), (256, 200), (258, 192)):
        with pytest.raises(vh.VatlError, match="stem7x7s2_pool_fwd") as plain:
            _old(vh, stem, torch.zeros((1, 3, h, wdt), device=dev()))
        with vh.flop_meter() as fm, pytest.raises(vh.VatlError, match="stem7x7s2_pool_fwd") as keyed:
            _new(vh, stem, torch.zeros((1, 3, h, wdt), device=dev()))
        assert str(plain.value) == str(keyed.value) and fm.routes["stem_pool_w1d"] == 0


def test_simplepose_plan_takes_the_route(vh, monkeypatch):
    """SimplePose-R50 on 20 synthetic crops with STEM_W1D on against off: the bars of the fused-stem plan test, the route counter, and the flop meter lower by
    the stem's difference."""
    from alphapose.models import hip_engine
    from oracle import synth
    from tests.test_gpu_conv import _build_simplepose
    m = _build_simplepose()
    x = to_dev(synth.crops(20))
    on, off = torch.empty((20, 17, 64, 48), device=dev()), torch.empty((20, 17, 64, 48), device=dev())
    assert hip_engine.STEM_W1D is True
    m.__dict__.pop("_vatl_plan", None)
    with torch.no_grad(), vh.flop_meter() as fm:
        hip_engine.forward_into(m, x, on)
    with torch.no_grad(), vh.flop_meter() as fm2:
        hip_engine.forward_into(m, x, on)
    assert fm.routes["stem_pool_w1d"] == 1 and fm.routes["stem_pool"] == 0 and fm2.routes == fm.routes, (fm.routes, fm2.routes)
    monkeypatch.setattr(hip_engine, "STEM_W1D", False)
    m.__dict__.pop("_vatl_plan", None)
    with torch.no_grad(), vh.flop_meter() as fo:
        hip_engine.forward_into(m, x, off)
    m.__dict__.pop("_vatl_plan", None)
    assert fo.routes["stem_pool_w1d"] == 0 and fo.routes["stem_pool"] == 1, fo.routes
    assert all(fo.routes[k] == fm.routes[k] for k in fo.routes if k not in ("stem_pool", "stem_pool_w1d")), (fm.routes, fo.routes)
    steps = 20 * (64 + 16 - 1)                                   # 20 crops are cut into 16 bands: 15 recomputed steps per image, in both kernels
    assert fo.direct - fm.direct == 2.0 * steps * 2 * 64 * (96 * 168 - 48 * 9 * 24) and fo.winograd == fm.winograd
    e = rel_err(on.cpu().numpy(), off.cpu().numpy())
    record("stem_w1d_vs_direct_simplepose_r50", rel=e)
    print(f"stem_w1d plan: heat-maps on vs off {e:.3e}")
    assert not torch.equal(on, off)
    assert e < 1e-5 and torch.equal(on.flatten(2).argmax(-1), off.flatten(2).argmax(-1)), e
