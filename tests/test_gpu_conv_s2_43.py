"""Stride-2 3x3 convs as Winograd F(4x3, 2x2) summed over the four input phases (csrc/winograd_s2_43.hip): the filter transform against a float64
restatement, the layer against a float64 conv and against the implicit GEMM, out-of-image pieces that are zeros and not neighbours, the shapes it
refuses, and the SimplePose-R50 plan with the route on and off.  (The network-level accuracy probe that preceded the kernel: tests/probes/s2_43_accuracy.py.)"""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import dev, record, rel_err, to_dev

pytestmark = pytest.mark.gpu

TOL = 2e-5      # max|err| / max|ref| per layer: the bar of tests/test_gpu_winograd.py and tests/test_gpu_deconv43.py

G4 = np.array([[0.5, 0.0], [-0.5, -0.5], [-1.0 / 6, 1.0 / 6], [1.0 / 6, 1.0 / 3], [0.0, 1.0]])      # vertical, points (0, 1, -1, 2, inf)
G3 = np.array([[1.0, 0.0], [0.5, 0.5], [0.5, -0.5], [0.0, -1.0]])                                   # horizontal, the G of F(3x3,2x2)


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def _nhwc(x):
    return np.ascontiguousarray(np.transpose(x, (0, 2, 3, 1)))


def _packed_u_reference(w):
    """U = G4 g G3^T per input phase in float64, g[a][b] = w4[2a + by][2b + bx] of the filter padded to 4x4 with zeros, in the order
    [n / 64][by = 0: bx, c / 8, 20 positions | by = 1: bx, c / 8, 16 positions][n / 32 % 2][(c % 8 / 4) * 32 + n % 32][c % 4].
    Returns the flat array and, per by, the full 20-position transforms (to check what the by = 1 half leaves out)."""
    cout, cin = w.shape[:2]
    w4 = np.zeros((cout, cin, 4, 4))
    w4[:, :, :3, :3] = w.astype(np.float64)
    steps = cin // 8
    parts, full = [], []
    for by in range(2):
        npos = 20 if by == 0 else 16
        blk = np.zeros((cout // 64, 2, steps, npos, 2, 64, 4))
        for bx in range(2):
            u = np.einsum("xa,ncab,vb->xvcn", G4, w4[:, :, by::2, bx::2], G3).reshape(20, cin, cout)
            full.append((by, bx, u))
            u = u[:npos].reshape(npos, steps, 2, 4, cout // 64, 2, 32)                  # pos, step, c % 8 / 4, c % 4, n_tile, nh, n % 32
            blk[:, bx] = np.transpose(u, (4, 1, 0, 5, 2, 6, 3)).reshape(cout // 64, steps, npos, 2, 64, 4)
        parts.append(blk.reshape(cout // 64, -1))
    return np.concatenate(parts, axis=1).reshape(-1), full


@pytest.mark.parametrize("cin,cout", [(16, 64), (48, 192)])
def test_packed_filter_matches_a_float64_restatement(vh, cin, cout):
    r = np.random.RandomState(cin * 1000 + cout)
    w = r.standard_normal((cout, cin, 3, 3)).astype(np.float32)
    u = vh.pack_winograd_s2_43_weight(to_dev(w)).cpu().numpy()
    assert u.size == int(vh.lib().vatl_winograd_s2_43_weight_floats(cout, cin)) == (20 + 20 + 16 + 16) * cin * cout
    ref, full = _packed_u_reference(w)
    assert ref.size == u.size
    # both sides round a float64 value once; the two float64 values differ by summation order only (~1e-16), so the float32 results
    # differ by at most one unit in the last place (2^-23 relative), and only where that value sits on a rounding boundary
    d = np.abs(u.astype(np.float64) - ref)
    assert (d <= 2.0 ** -23 * np.abs(ref) + 1e-12).all(), float(d.max())
    assert (u == ref.astype(np.float32)).mean() > 0.99
    # the by = 1 phases store 16 positions: per 64 output channels 2 * (Cin / 8) * 20 * 512 floats of by = 0, then 2 * (Cin / 8) * 16 * 512 of by = 1 —
    # and the four positions left out (row position 4) are identically zero, as is column position 3 of the bx = 1 phases
    per_tile = u.reshape(cout // 64, -1)
    assert per_tile.shape[1] == (cin // 8) * 2 * (20 + 16) * 512
    for by, bx, t in full:
        if by:
            assert np.abs(t[16:]).max() == 0.0
        if bx:
            assert np.abs(t[3::4]).max() == 0.0
    by1 = per_tile[:, (cin // 8) * 2 * 20 * 512:].reshape(cout // 64, 2, cin // 8, 16, 2, 64, 4)
    want = np.einsum("xa,ncab,vb->xvcn", G4, np.pad(w.astype(np.float64), ((0, 0), (0, 0), (0, 1), (0, 1)))[:, :, 1::2, 0::2], G3).reshape(20, cin, cout)
    assert np.allclose(by1[0, 0, 0, :, 0, 0, 0], want[:16, 0, 0], rtol=2.0 ** -22, atol=1e-12)      # (phase (1, 0), channel pair (0, 0): all 16 positions in place)


CASES = [
    # n, H, W, Cin, Cout (H x W: the input grid)
    (1, 8, 6, 16, 64),            # one tile, one stage per phase; every border of every phase falls in the same tile
    (5, 16, 12, 32, 64),          # 20 tiles, images straddle a block
    (9, 16, 12, 48, 128),         # 36 tiles, a tail group, two filter tiles, an odd stage count per phase
    (2, 32, 24, 64, 192),         # interior tiles without any border
    (2, 16, 12, 512, 128),        # the long reduction: 128 stages, layer4.0.conv2's geometry
    (1, 64, 48, 128, 128),        # layer2.0.conv2's geometry
]


def _layer(vh, n, h, w, cin, cout):
    r = np.random.RandomState(zlib.crc32(repr((n, h, w, cin, cout)).encode()) % 2 ** 31)
    x = r.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (r.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
    gamma, beta = r.uniform(0.5, 1.5, cout).astype(np.float32), r.standard_normal(cout).astype(np.float32) * 0.1
    mean, var = r.standard_normal(cout).astype(np.float32) * 0.1, r.uniform(0.5, 1.5, cout).astype(np.float32)
    ref = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), None, 2, 1)
    ref = F.batch_norm(ref, torch.from_numpy(mean).double(), torch.from_numpy(var).double(), torch.from_numpy(gamma).double(),
                       torch.from_numpy(beta).double(), False, 0.0, 1e-5).relu().numpy()
    scale, bias = vh.bn_fold(to_dev(gamma), to_dev(beta), to_dev(mean), to_dev(var), 1e-5)
    return to_dev(_nhwc(x)), to_dev(wt), scale, bias, ref


def _s2(vh, x, wp, us2, scale, bias, cout, relu=True):
    return vh.conv2d_fwd(x, wp, scale, bias, cout, 3, 3, 2, 1, relu, u_s2=us2)


@pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c)) for c in CASES])
def test_s2_43_matches_float64_and_the_implicit_gemm(vh, case):
    n, h, w, cin, cout = case
    xd, wd, scale, bias, ref = _layer(vh, *case)
    assert vh.conv3x3s2_winograd43_supported(n, h, w, cin, cout)
    us2 = vh.pack_winograd_s2_43_weight(wd)
    with vh.flop_meter() as fm:
        y = _s2(vh, xd, None if cin % 32 else vh.pack_conv_weight(wd), us2, scale, bias, cout)
    assert fm.routes["winograd_s2_43"] == 1 and fm.routes["igemm"] == 0 and sum(fm.routes.values()) == 1, fm.routes
    tiles32 = (n * (h // 8) * (w // 6) + 31) // 32 * 32
    assert fm.direct == 2.0 * tiles32 * 72 * cin * cout and fm.direct_launches == 1 and fm.winograd_launches == 0 and fm.winograd == 0
    assert y.shape == (n, h // 2, w // 2, cout)
    e = rel_err(np.transpose(y.cpu().numpy(), (0, 3, 1, 2)), ref)
    print(f"s2_43 {case}: route vs float64 {e:.3e}")
    ed = None
    if cin % 32 == 0:                                           # the implicit GEMM needs whole 32-channel k-tiles
        wp = vh.pack_conv_weight(wd)
        with vh.flop_meter() as fo:
            yd = vh.conv2d_fwd(xd, wp, scale, bias, cout, 3, 3, 2, 1, True)
        assert fo.routes["winograd_s2_43"] == 0 and fo.routes["igemm"] == 1, fo.routes
        ed = rel_err(y.cpu().numpy(), yd.cpu().numpy())
        eg = rel_err(np.transpose(yd.cpu().numpy(), (0, 3, 1, 2)), ref)
        print(f"s2_43 {case}: route vs implicit GEMM {ed:.3e}, implicit GEMM vs float64 {eg:.3e}")
        record("s2_43_vs_igemm_" + "x".join(map(str, case)), rel=ed, igemm_vs_fp64=eg)
    record("s2_43_" + "x".join(map(str, case)), s2_43_vs_fp64=e)
    assert e < TOL, (case, e)
    assert ed is None or ed < TOL, (case, ed)


def test_out_of_image_pieces_are_zeros_not_neighbours(vh):
    case = (5, 16, 12, 32, 64)
    xd, wd, scale, bias, _ = _layer(vh, *case)
    wp, us2 = vh.pack_conv_weight(wd), vh.pack_winograd_s2_43_weight(wd)
    full = _s2(vh, xd, wp, us2, scale, bias, 64)
    for i in range(5):
        alone = _s2(vh, xd[i:i + 1].contiguous(), wp, us2, scale, bias, 64)
        assert torch.equal(alone[0], full[i]), i
    shifted = _s2(vh, xd[2:].contiguous(), wp, us2, scale, bias, 64)
    assert torch.equal(shifted, full[2:])
    # a phase whose border test is wrong reads a neighbouring row or image; a finite neighbour times a zero filter position would hide it, NaN does not
    xn = xd.clone()
    xn[1] = float("nan")
    xn[3] = float("nan")
    poisoned = _s2(vh, xn, wp, us2, scale, bias, 64)
    assert torch.equal(poisoned[2], full[2])
    assert torch.equal(poisoned[0], full[0]) and torch.equal(poisoned[4], full[4])
    out = torch.full((5, 8, 6, 64), -7.0, device=dev())
    y = vh.conv2d_fwd(xd, wp, scale, bias, 64, 3, 3, 2, 1, True, out=out, u_s2=us2)
    assert y.data_ptr() == out.data_ptr() and torch.equal(out, full)


@pytest.mark.parametrize("case", [(2, 15, 12, 64, 64), (2, 20, 12, 64, 64), (3, 16, 12, 256, 100), (1, 16, 12, 24, 64)], ids=lambda c: "x".join(map(str, c)))
def test_refused_shapes_keep_the_plain_bits(vh, case):
    """An odd H, an output grid of 10x6, Cout = 100, Cin = 24: unsupported, and conv2d_fwd with the keyword set gives the bits of the plain call
    (Cin = 24 is no shape of the implicit GEMM either: there both calls raise the plain call's error)."""
    n, h, w, cin, cout = case
    assert not vh.conv3x3s2_winograd43_supported(n, h, w, cin, cout)
    g = torch.Generator(device="cpu").manual_seed(cin + cout + h)
    x = torch.randn((n, h, w, cin), generator=g).to(dev())
    wt = (torch.randn((cout, cin, 3, 3), generator=g) * 0.05).to(dev())
    wp = vh.pack_conv_weight(wt)
    # the wrapper never looks into u_s2 on a refused shape (a filter with Cout % 64 != 0 or Cin % 16 != 0 cannot even be packed for the route)
    us2 = torch.empty(1, device=dev())
    if cout % 64 != 0 or cin % 16 != 0:
        with pytest.raises(vh.VatlError):
            vh.pack_winograd_s2_43_weight(wt)
    else:
        us2 = vh.pack_winograd_s2_43_weight(wt)
    if cin % 32 != 0:
        with pytest.raises(vh.VatlError, match="multiple of 32") as plain:
            vh.conv2d_fwd(x, wp, None, None, cout, 3, 3, 2, 1, False)
        with pytest.raises(vh.VatlError, match="multiple of 32") as keyed:
            vh.conv2d_fwd(x, wp, None, None, cout, 3, 3, 2, 1, False, u_s2=us2)
        assert str(plain.value) == str(keyed.value)
        return
    with vh.flop_meter() as fm:
        y = vh.conv2d_fwd(x, wp, None, None, cout, 3, 3, 2, 1, False, u_s2=us2)
    assert fm.routes["winograd_s2_43"] == 0 and fm.direct_launches == 1, fm.routes
    assert torch.equal(y, vh.conv2d_fwd(x, wp, None, None, cout, 3, 3, 2, 1, False))


def test_the_keyword_is_ignored_where_the_route_does_not_apply(vh):
    """A residual, NCHW output or another stride keep the implicit GEMM's bits with the keyword set."""
    xd, wd, scale, bias, _ = _layer(vh, 2, 16, 12, 32, 64)
    wp, us2 = vh.pack_conv_weight(wd), vh.pack_winograd_s2_43_weight(wd)
    res = torch.randn((2, 8, 6, 64), generator=torch.Generator(device="cpu").manual_seed(3)).to(dev())
    for kw in ({"residual": res}, {"out_nchw": True}):
        with vh.flop_meter() as fm:
            y = vh.conv2d_fwd(xd, wp, scale, bias, 64, 3, 3, 2, 1, True, u_s2=us2, **kw)
        assert fm.routes["winograd_s2_43"] == 0, (kw.keys(), fm.routes)
        assert torch.equal(y, vh.conv2d_fwd(xd, wp, scale, bias, 64, 3, 3, 2, 1, True, **kw))
    with vh.flop_meter() as fm:
        y = vh.conv2d_fwd(xd, wp, scale, bias, 64, 3, 3, 1, 1, True, u_s2=us2)
    assert fm.routes["winograd_s2_43"] == 0 and torch.equal(y, vh.conv2d_fwd(xd, wp, scale, bias, 64, 3, 3, 1, 1, True))


def test_simplepose_plan_routes_the_stride2_convs(vh, monkeypatch):
    """SimplePose-R50 on 3 crops: with S2_43 on, layer2/3/4.0.conv2 take the new kernel (the route counter says which); with it off none does and the
    same launches appear under igemm; the heat-maps agree to fp32 rounding with identical arg-max."""
    from alphapose.models import hip_engine
    from oracle import synth
    from tests.test_gpu_conv import _build_simplepose
    m = _build_simplepose()
    x = to_dev(synth.crops(3))
    routed = sum(vh.conv3x3s2_winograd43_supported(3, h, w, c, c) for h, w, c in ((64, 48, 128), (32, 24, 256), (16, 12, 512)))
    assert routed == 3
    on, off = torch.empty((3, 17, 64, 48), device=dev()), torch.empty((3, 17, 64, 48), device=dev())
    m.__dict__.pop("_vatl_plan", None)
    with torch.no_grad(), vh.flop_meter() as fm:
        hip_engine.forward_into(m, x, on)
    assert fm.routes["winograd_s2_43"] == routed, fm.routes
    monkeypatch.setattr(hip_engine, "S2_43", False)
    m.__dict__.pop("_vatl_plan", None)
    with torch.no_grad(), vh.flop_meter() as fo:
        hip_engine.forward_into(m, x, off)
    m.__dict__.pop("_vatl_plan", None)
    assert fo.routes["winograd_s2_43"] == 0 and fo.routes["igemm"] - fm.routes["igemm"] == routed, (fm.routes, fo.routes)
    assert sum(fo.routes.values()) == sum(fm.routes.values())
    assert all(fo.routes[k] == fm.routes[k] for k in fo.routes if k not in ("igemm", "winograd_s2_43")), (fm.routes, fo.routes)
    e = rel_err(on.cpu().numpy(), off.cpu().numpy())
    record("s2_43_vs_igemm_simplepose_r50", rel=e)
    print(f"s2_43 plan: heat-maps on vs off {e:.3e}")
    assert e < 2e-5 and torch.equal(on.flatten(2).argmax(-1), off.flatten(2).argmax(-1)), e
