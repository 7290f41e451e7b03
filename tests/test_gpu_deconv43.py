"""Winograd F(4x3, 2x2) route of ConvTranspose2d(4, 2, 1) (csrc/winograd_deconv43.hip): the filter transform against a float64 restatement,
the layer against a float64 transposed conv and against the implicit GEMM, bits independent of the batch position, the shapes it refuses,
and the SimplePose-R50 plan with the route on and off."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import dev, record, rel_err, to_dev

pytestmark = pytest.mark.gpu

TOL = 2e-5      # max|err| / max|ref| per layer: the file-level bar of tests/test_gpu_winograd.py

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
    """U = G4 g G3^T per phase in float64, in the fragment order [phase][n / 64][c / 8][xi * 4 + nu][n / 32 % 2][(c % 8 / 4) * 32 + n % 32][c % 4]."""
    cin, cout = w.shape[:2]
    w64 = w.astype(np.float64)
    out = np.zeros((4, cout // 64, cin // 8, 20, 2, 64, 4))
    for phase in range(4):
        py, px = phase >> 1, phase & 1
        g = w64[:, :, [3 - py, 1 - py]][:, :, :, [3 - px, 1 - px]]                  # g[c][n][a][b] = w[c][n][3 - py - 2a][3 - px - 2b]
        u = np.einsum("xa,cnab,vb->xvcn", G4, g, G3).reshape(20, cin, cout)
        u = u.reshape(20, cin // 8, 2, 4, cout // 64, 2, 32)                        # pos, step, c % 8 / 4, c % 4, n_tile, nh, n % 32
        out[phase] = np.transpose(u, (4, 1, 0, 5, 2, 6, 3)).reshape(cout // 64, cin // 8, 20, 2, 64, 4)
    return out.reshape(-1)


@pytest.mark.parametrize("cin,cout", [(16, 64), (48, 192)])
def test_packed_filter_matches_a_float64_restatement(vh, cin, cout):
    r = np.random.RandomState(cin * 1000 + cout)
    w = r.standard_normal((cin, cout, 4, 4)).astype(np.float32)
    u = vh.pack_winograd_deconv43_weight(to_dev(w)).cpu().numpy()
    assert u.size == int(vh.lib().vatl_winograd_deconv43_weight_floats(cout, cin)) == 80 * cin * cout
    ref = _packed_u_reference(w)
    # both sides round a float64 value once; the two float64 values differ by summation order only (~1e-16), so the float32 results
    # differ by at most one unit in the last place (2^-23 relative), and only where that value sits on a rounding boundary
    d = np.abs(u.astype(np.float64) - ref)
    assert (d <= 2.0 ** -23 * np.abs(ref) + 1e-12).all(), float(d.max())
    assert (u == ref.astype(np.float32)).mean() > 0.99


CASES = [
    # n, H, W, Cin, Cout
    (1, 4, 3, 16, 64),            # one tile, one stage
    (5, 8, 6, 32, 64),            # 20 tiles: images straddle a block, two stages
    (9, 8, 6, 48, 128),           # 36 tiles: a tail group, two channel units
    (2, 16, 12, 64, 192),         # odd half-count boundary
    (2, 8, 6, 2048, 256),         # the long reduction
    (1, 32, 24, 256, 256),        # the deconv3 geometry
]


def _layer(vh, n, h, w, cin, cout):
    r = np.random.RandomState(zlib.crc32(repr((n, h, w, cin, cout)).encode()) % 2 ** 31)
    x = r.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (r.standard_normal((cin, cout, 4, 4)) / np.sqrt(cin * 4)).astype(np.float32)
    gamma, beta = r.uniform(0.5, 1.5, cout).astype(np.float32), r.standard_normal(cout).astype(np.float32) * 0.1
    mean, var = r.standard_normal(cout).astype(np.float32) * 0.1, r.uniform(0.5, 1.5, cout).astype(np.float32)
    ref = F.conv_transpose2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), None, 2, 1)
    ref = F.batch_norm(ref, torch.from_numpy(mean).double(), torch.from_numpy(var).double(), torch.from_numpy(gamma).double(),
                       torch.from_numpy(beta).double(), False, 0.0, 1e-5).relu().numpy()
    scale, bias = vh.bn_fold(to_dev(gamma), to_dev(beta), to_dev(mean), to_dev(var), 1e-5)
    return to_dev(_nhwc(x)), to_dev(wt), scale, bias, ref


@pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c)) for c in CASES])
def test_deconv43_matches_float64_and_the_implicit_gemm(vh, case):
    n, h, w, cin, cout = case
    xd, wd, scale, bias, ref = _layer(vh, *case)
    assert vh.deconv4x4s2_winograd43_supported(n, h, w, cin, cout)
    u, u43 = vh.pack_winograd_deconv_weight(wd), vh.pack_winograd_deconv43_weight(wd)
    with vh.flop_meter() as fm:
        y = vh.deconv4x4s2_winograd_fwd(xd, u, scale, bias, cout, True, u43=u43)
    assert fm.routes["winograd_deconv43"] == 1 and fm.winograd_launches == 1 and fm.direct_launches == 0, fm.routes
    tiles32 = (n * (h // 4) * (w // 3) + 31) // 32 * 32
    assert fm.winograd == 2.0 * tiles32 * 20 * cin * cout * 4
    with vh.flop_meter() as fo:
        y33 = vh.deconv4x4s2_winograd_fwd(xd, u, scale, bias, cout, True)
    assert fo.routes["winograd_deconv43"] == 0 and fo.winograd_launches == 1, fo.routes
    e43 = rel_err(np.transpose(y.cpu().numpy(), (0, 3, 1, 2)), ref)
    e33 = rel_err(np.transpose(y33.cpu().numpy(), (0, 3, 1, 2)), ref)
    record("deconv43_" + "x".join(map(str, case)), f43_vs_fp64=e43, f33_vs_fp64=e33)
    print(f"deconv43 {case}: F(4x3,2x2) {e43:.3e}  F(3x3,2x2) {e33:.3e}")
    assert e43 < TOL and e33 < TOL, (case, e43, e33)
    if cin % 32 == 0:                                           # the implicit GEMM needs whole 32-channel k-tiles
        yd = vh.deconv4x4s2_fwd(xd, vh.pack_deconv_weight(wd), scale, bias, cout, True)
        ed = rel_err(y.cpu().numpy(), yd.cpu().numpy())
        record("deconv43_vs_igemm_" + "x".join(map(str, case)), rel=ed)
        assert ed < TOL, (case, ed)


def test_deconv43_bits_do_not_depend_on_the_batch_position_or_the_output_buffer(vh):
    case = (5, 8, 6, 32, 64)
    xd, wd, scale, bias, _ = _layer(vh, *case)
    u, u43 = vh.pack_winograd_deconv_weight(wd), vh.pack_winograd_deconv43_weight(wd)
    full = vh.deconv4x4s2_winograd_fwd(xd, u, scale, bias, 64, True, u43=u43)
    for i in range(5):
        alone = vh.deconv4x4s2_winograd_fwd(xd[i:i + 1].contiguous(), u, scale, bias, 64, True, u43=u43)
        assert torch.equal(alone[0], full[i]), i
    shifted = vh.deconv4x4s2_winograd_fwd(xd[2:].contiguous(), u, scale, bias, 64, True, u43=u43)
    assert torch.equal(shifted, full[2:])
    out = torch.full((5, 16, 12, 64), -7.0, device=dev())
    y = vh.deconv4x4s2_winograd_fwd(xd, u, scale, bias, 64, True, out=out, u43=u43)
    assert y.data_ptr() == out.data_ptr() and torch.equal(out, full)


@pytest.mark.parametrize("case", [(2, 5, 3, 64, 48), (3, 16, 12, 256, 100), (1, 7, 10, 48, 64)], ids=lambda c: "x".join(map(str, c)))
def test_refused_shapes_keep_the_f33_bits(vh, case):
    n, h, w, cin, cout = case
    assert not vh.deconv4x4s2_winograd43_supported(n, h, w, cin, cout)
    g = torch.Generator(device="cpu").manual_seed(cin + cout)
    x = torch.randn((n, h, w, cin), generator=g).to(dev())
    wt = (torch.randn((cin, cout, 4, 4), generator=g) * 0.05).to(dev())
    u = vh.pack_winograd_deconv_weight(wt)
    # the wrapper never looks into u43 on a refused shape (a filter with Cout % 64 != 0 cannot even be packed for the route)
    u43 = torch.empty(1, device=dev())
    if cout % 64 != 0:
        with pytest.raises(vh.VatlError):
            vh.pack_winograd_deconv43_weight(wt)
    else:
        u43 = vh.pack_winograd_deconv43_weight(wt)
    with vh.flop_meter() as fm:
        y = vh.deconv4x4s2_winograd_fwd(x, u, None, None, cout, False, u43=u43)
    assert fm.routes["winograd_deconv43"] == 0 and fm.winograd_launches == 1, fm.routes
    assert torch.equal(y, vh.deconv4x4s2_winograd_fwd(x, u, None, None, cout, False))


def test_simplepose_plan_routes_the_transposed_convs(vh, monkeypatch):
    """SimplePose-R50 on 3 crops: with DECONV_43 on, the transposed convs the plan routes take the F(4x3,2x2) kernel (the route counter says which);
    with it off none does; the heat-maps agree to fp32 rounding with identical arg-max."""
    from alphapose.models import hip_engine
    from oracle import synth
    from tests.test_gpu_conv import _build_simplepose
    m = _build_simplepose()
    x = to_dev(synth.crops(3))
    routed = sum(vh.deconv4x4s2_winograd43_supported(3, h, w, c, 256) for h, w, c in ((8, 6, 2048), (16, 12, 256), (32, 24, 256)))
    assert routed >= 1
    on, off = torch.empty((3, 17, 64, 48), device=dev()), torch.empty((3, 17, 64, 48), device=dev())
    m.__dict__.pop("_vatl_plan", None)
    with torch.no_grad(), vh.flop_meter() as fm:
        hip_engine.forward_into(m, x, on)
    assert fm.routes["winograd_deconv43"] == routed, fm.routes
    monkeypatch.setattr(hip_engine, "DECONV_43", False)
    m.__dict__.pop("_vatl_plan", None)
    with torch.no_grad(), vh.flop_meter() as fo:
        hip_engine.forward_into(m, x, off)
    m.__dict__.pop("_vatl_plan", None)
    f33 = lambda r: r["winograd"] + r["winograd_2h"]             # the F(3x3,2x2) launches share the general kernel's counters with the 3x3 layers at 8x6
    assert fo.routes["winograd_deconv43"] == 0 and f33(fo.routes) - f33(fm.routes) == routed, (fm.routes, fo.routes)
    assert sum(fo.routes.values()) == sum(fm.routes.values())
    e = rel_err(on.cpu().numpy(), off.cpu().numpy())
    record("deconv43_vs_f33_simplepose_r50", rel=e)
    assert e < 2e-5 and torch.equal(on.flatten(2).argmax(-1), off.flatten(2).argmax(-1)), e
