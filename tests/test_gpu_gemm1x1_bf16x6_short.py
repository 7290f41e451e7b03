"""The short-K form of the bf16x6 GEMM (csrc/gemm1x1_bf16x6.hip, gemm1x1_bf16x6_short_kernel: 128 <= K < 512, N >= 512 — conv3 of ResNet stages 2 and 3 — with
scale / bias loaded in front of the k-loop and the residual tile brought in by LDS-DMA under the last three stages), reached through
vatl_hip.conv1x1_rows_fwd(..., u_x6=): float64 parity inside the house bar of 2e-5 of the layer maximum (the fp32 kernel's error on the same inputs is
recorded beside it), exactness on data where the split must lose nothing, batch-position independence, the refusals of the C entry point and the
SimplePose-R50 plan with hip_engine.BF16X6_SHORT on and off."""
import ctypes

import numpy as np
import pytest
import torch

from tests.gpu_util import dev, record, rel_err, to_dev

pytestmark = pytest.mark.gpu

BAR = 2e-5         # of the layer maximum, against float64 (tests/test_gpu_gemm1x1_bf16x6.py)
ROUTE = "gemm1x1_bf16x6_short"


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def _short(vh, x, wp, ux6, sc, bi, cout, relu, res=None):
    with vh.flop_meter() as fm:
        y = vh.conv1x1_rows_fwd(x, wp, sc, bi, cout, relu, residual=res, u_x6=ux6)
    assert fm.routes[ROUTE] == 1 and sum(fm.routes.values()) == 1, fm.routes
    return y


def _fp32(vh, x, wp, sc, bi, cout, relu, res=None):
    """The same layer on the fp32 kernel that serves it without the keyword: the row-streaming GEMM (K = 128 / 256), else the implicit GEMM."""
    n, h, w_, k = x.shape
    if vh.conv1x1_rows_supported(k, 0, cout, n * h * w_):
        return vh.conv1x1_rows_fwd(x, wp, sc, bi, cout, relu, residual=res)
    return vh.conv2d_fwd(x, wp, sc, bi, cout, 1, 1, 1, 0, relu, residual=res)


def _layer(r, cin, cout):
    w = (r.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)
    return w, r.uniform(0.5, 1.5, cout).astype(np.float32), r.standard_normal(cout).astype(np.float32)


def _pack(vh, w):
    wp = vh.pack_conv_weight(to_dev(w.reshape(w.shape[0], w.shape[1], 1, 1)))
    return wp, vh.pack_gemm1x1_bf16x6_weight(wp)


# (n, H, W, K, N, residual, relu): one partial m-tile, eight n-tiles | two m-tiles with a tail | 8 stages, the shortest loop | the SE form, relu on and off |
# 12 stages | 28 stages
CASES = ((1, 8, 6, 256, 1024, True, True), (3, 8, 6, 256, 1024, True, True), (1, 16, 12, 128, 512, True, True), (3, 8, 6, 128, 512, False, True),
         (3, 8, 6, 128, 512, False, False), (2, 8, 6, 192, 512, True, True), (1, 8, 6, 448, 512, False, True))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c[:5]) + ("_res" if c[5] else "") + ("" if c[6] else "_norelu"))
def test_against_float64(vh, case):
    n, h, w_, k, cout, use_res, relu = case
    r = np.random.RandomState(k + cout + n)
    w, sc, bi = _layer(r, k, cout)
    x = r.standard_normal((n, h, w_, k)).astype(np.float32)
    rs = r.standard_normal((n, h, w_, cout)).astype(np.float32) if use_res else None
    want = (x.astype(np.float64).reshape(-1, k) @ w.T.astype(np.float64)) * sc + bi + (rs.reshape(-1, cout) if use_res else 0.0)
    want = (np.maximum(want, 0) if relu else want).reshape(n, h, w_, cout)
    xd, scd, bid, rsd = to_dev(x), to_dev(sc), to_dev(bi), to_dev(rs) if use_res else None
    wp, ux6 = _pack(vh, w)
    assert vh.gemm1x1_bf16x6_short_supported(n * h * w_, k, cout)
    got = _short(vh, xd, wp, ux6, scd, bid, cout, relu, rsd)
    plain = _fp32(vh, xd, wp, scd, bid, cout, relu, rsd)
    e, ep = rel_err(got.cpu().numpy(), want), rel_err(plain.cpu().numpy(), want)
    record(f"gemm1x1_bf16x6_short_{n}x{h}x{w_}x{k}_{cout}" + ("_res" if use_res else "") + ("" if relu else "_norelu"), vs_fp64=e, fp32_vs_fp64=ep)
    print(f"bf16x6 short {case}: route {e:.3e}  fp32 kernel {ep:.3e}")
    assert e < BAR, (e, ep)


EXACT = ((128, 512, False), (128, 512, True), (256, 1024, False), (256, 1024, True))
EXACT_IDS = [f"{k}_{n}" + ("_zero_res" if z else "") for k, n, z in EXACT]


def _zero_res(shape, on):
    return torch.zeros(shape, device=dev()) if on else None


@pytest.mark.parametrize("case", EXACT, ids=EXACT_IDS)
def test_permutation_filter_returns_the_input_bits(vh, case):
    """Row n of the filter is the unit vector perm[n mod K], full-mantissa inputs, no scale or bias (and a residual of zeros): the three pieces of an input
    add back to it exactly, so output column n IS input column perm[n mod K] — plane, lane and k order are right and the LDS residual path adds its zeros."""
    k, cout, zres = case
    r = np.random.RandomState(3 + k)
    x = to_dev(r.standard_normal((3, 8, 6, k)).astype(np.float32))
    perm = r.permutation(k)[np.arange(cout) % k]
    w = np.zeros((cout, k), np.float32)
    w[np.arange(cout), perm] = 1.0
    wp, ux6 = _pack(vh, w)
    y = _short(vh, x, wp, ux6, None, None, cout, False, _zero_res((3, 8, 6, cout), zres))
    assert torch.equal(y, x[..., torch.as_tensor(perm, device=dev())])


@pytest.mark.parametrize("case", EXACT, ids=EXACT_IDS)
def test_small_integers_are_exact(vh, case):
    k, cout, zres = case
    r = np.random.RandomState(4 + k)
    n, h, w_ = 2, 9, 11                                  # M = 198: a tail of 70 rows
    x = r.randint(-8, 9, (n, h, w_, k)).astype(np.float32)
    w = r.randint(-4, 5, (cout, k)).astype(np.float32)
    want = x.astype(np.int64).reshape(-1, k) @ w.T.astype(np.int64)                # |sum| <= 256 * 32: exact in fp32
    wp, ux6 = _pack(vh, w)
    y = _short(vh, to_dev(x), wp, ux6, None, None, cout, False, _zero_res((n, h, w_, cout), zres)).cpu().numpy().reshape(-1, cout)
    assert np.array_equal(y.astype(np.int64), want) and np.array_equal(y, want.astype(np.float32))


@pytest.mark.parametrize("case", EXACT, ids=EXACT_IDS)
def test_inputs_at_every_exponent_stay_inside_the_bar(vh, case):
    """Row m holds +-2^e (1 + 2^-23), e = m - 100 for m = 0 .. 200: every row, taken as a layer of its own, is inside the bar."""
    k, cout, zres = case
    r = np.random.RandomState(6 + k)
    m = 201
    w, _, _ = _layer(r, k, cout)
    e = np.arange(m) - 100
    x = (np.ldexp(1.0 + 2.0 ** -23, e)[:, None] * r.choice([-1.0, 1.0], (m, k))).astype(np.float32)
    want = x.astype(np.float64) @ w.T.astype(np.float64)
    wp, ux6 = _pack(vh, w)
    y = _short(vh, to_dev(x.reshape(1, 3, 67, k)), wp, ux6, None, None, cout, False, _zero_res((1, 3, 67, cout), zres)).cpu().numpy().reshape(m, cout)
    worst = max(rel_err(y[i], want[i]) for i in range(m))
    record(f"gemm1x1_bf16x6_short_exponents_{k}_{cout}" + ("_zero_res" if zres else ""), worst_row=worst)
    assert worst < BAR, worst


@pytest.mark.parametrize("k,cout", ((256, 1024), (128, 512)))
def test_rows_do_not_depend_on_their_neighbours(vh, k, cout):
    """Rows of the M = 144 case — the first, one of the tail tile, the last, and rows 60 and 125, whose residual travels in registers rather than through
    the ring — equal the same rows computed alone, and an image keeps its bits between neighbours whose inputs and residuals are NaN."""
    r = np.random.RandomState(8 + k)
    n, h, w_ = 3, 8, 6
    w, sc, bi = _layer(r, k, cout)
    x = to_dev(r.standard_normal((n, h, w_, k)).astype(np.float32))
    rs = to_dev(r.standard_normal((n, h, w_, cout)).astype(np.float32))
    scd, bid = to_dev(sc), to_dev(bi)
    wp, ux6 = _pack(vh, w)
    full = _short(vh, x, wp, ux6, scd, bid, cout, True, rs)
    for row in (0, 50, 60, 125, 143):
        solo = _short(vh, x.reshape(-1, k)[row].reshape(1, 1, 1, k).contiguous(), wp, ux6, scd, bid, cout, True, rs.reshape(-1, cout)[row].reshape(1, 1, 1, cout).contiguous())
        assert torch.equal(solo.reshape(-1), full.reshape(-1, cout)[row]), row
    xn, rn = torch.full_like(x, float("nan")), torch.full_like(rs, float("nan"))
    xn[1], rn[1] = x[1], rs[1]
    poisoned = _short(vh, xn, wp, ux6, scd, bid, cout, True, rn)
    assert torch.equal(poisoned[1], full[1])
    assert torch.equal(_short(vh, x[1:2].contiguous(), wp, ux6, scd, bid, cout, True, rs[1:2].contiguous())[0], full[1])      # the middle image alone


REFUSED = ((64, 512, 1), (512, 512, 1), (160, 512, 1), (256, 384, 1), (256, 640, 1), (256, 1024, 2))


def test_unsupported_shapes_are_refused_with_nothing_launched(vh):
    """K = 64, K = 512 (the long route's), K = 160, N = 384, N = 640 and stride 2: the shape query says no, the C entry point fails and names itself, nothing is
    launched or metered and y keeps its bytes; the Python keyword is ignored on such a shape and the call gives the plain kernel's bits."""
    lib = vh.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    buf = torch.zeros(1 << 22, device=dev())             # stands in for every operand: a refused call reads none of them
    y = torch.full((1 << 20,), 7.0, device=dev())
    for cin, cout, stride in REFUSED:
        assert stride != 1 or not vh.gemm1x1_bf16x6_short_supported(48, cin, cout), (cin, cout)
    assert vh.gemm1x1_bf16x6_short_supported(48, 128, 512) and vh.gemm1x1_bf16x6_short_supported(48, 448, 512)
    assert not vh.gemm1x1_bf16x6_supported(48, 448, 0, 512)                                                     # (the long route's rule has not moved)
    with vh.flop_meter() as fm:
        for cin, cout, stride in REFUSED:
            rc = lib.vatl_gemm1x1_bf16x6_short_fwd(p(buf), p(buf), None, None, p(buf), p(y), 1, 8, 6, cin, cout, stride, 0, None)
            assert rc != 0 and b"gemm1x1_bf16x6_short_fwd" in lib.vatl_last_error(), (cin, cout, stride)
        assert vh.flop_meter.launches_now() == 0
    assert sum(fm.routes.values()) == 0, fm.routes
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    r = np.random.RandomState(9)
    x = to_dev(r.standard_normal((1, 8, 6, 128)).astype(np.float32))
    wp = vh.pack_conv_weight(to_dev((r.standard_normal((384, 128, 1, 1)) / 11).astype(np.float32)))
    with vh.flop_meter() as fm:
        got = vh.conv1x1_rows_fwd(x, wp, None, None, 384, False, u_x6=buf)
    assert fm.routes[ROUTE] == 0 and fm.routes["rows_1x1"] == 1 and torch.equal(got, vh.conv1x1_rows_fwd(x, wp, None, None, 384, False))


def test_simplepose_plan_with_the_route_on_and_off(vh, monkeypatch):
    """SimplePose-R50 on 8 crops, plan rebuilds.  BF16X6_SHORT on with BF16X6_SHORT_MIN_K = 128: the eight conv3 + skip launches of stages 2 and 3 (l2.1-3,
    l3.1-5) take the short route and the 17 long-K launches stay where they were; with the shipped BF16X6_SHORT_MIN_K = 256 the five of stage 3 do; off: 0 and 17
    with the same launch total, heat-maps within 1e-5 of their maximum and the same arg-max as either switch-on run; BF16X6 off: neither route is taken."""
    from alphapose.models import hip_engine
    from oracle import synth
    from tests.test_gpu_conv import _build_simplepose
    m = _build_simplepose()
    x = to_dev(synth.crops(8))
    on, on5, off, none = (torch.empty((8, 17, 64, 48), device=dev()) for _ in range(4))

    def run(out):
        m.__dict__.pop("_vatl_plan", None)
        with torch.no_grad(), vh.flop_meter() as fm:
            hip_engine.forward_into(m, x, out)
        m.__dict__.pop("_vatl_plan", None)
        return fm.routes

    assert hip_engine.BF16X6 is True and hip_engine.BF16X6_SHORT is True and hip_engine.BF16X6_SHORT_MIN_K == 256
    r_on5 = run(on5)
    assert r_on5[ROUTE] == 5 and r_on5["gemm1x1_bf16x6"] == 17, r_on5
    monkeypatch.setattr(hip_engine, "BF16X6_SHORT_MIN_K", 128)
    r_on = run(on)
    assert r_on[ROUTE] == 8 and r_on["gemm1x1_bf16x6"] == 17 and sum(r_on.values()) == sum(r_on5.values()), (r_on, r_on5)
    monkeypatch.setattr(hip_engine, "BF16X6_SHORT", False)
    r_off = run(off)
    assert r_off[ROUTE] == 0 and r_off["gemm1x1_bf16x6"] == 17 and sum(r_off.values()) == sum(r_on.values()), (r_on, r_off)
    for name, got in (("8", on), ("5", on5)):
        e = rel_err(got.cpu().numpy(), off.cpu().numpy())
        record("bf16x6_short_vs_rows_simplepose_r50_" + name, rel=e)
        print(f"bf16x6 short plan, {name} launches on the route: heat-maps on vs off {e:.3e}")
        assert e < 1e-5 and torch.equal(got.flatten(2).argmax(-1), off.flatten(2).argmax(-1)), e
    monkeypatch.setattr(hip_engine, "BF16X6_SHORT", True)
    monkeypatch.setattr(hip_engine, "BF16X6", False)
    r_none = run(none)
    assert r_none[ROUTE] == 0 and r_none["gemm1x1_bf16x6"] == 0, r_none
