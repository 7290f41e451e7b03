"""The bf16x6 GEMM route for long-K 1x1 layers (csrc/gemm1x1_bf16x6.hip: every fp32 product as six bf16 MFMAs on exact three-way splits, csrc/split16.h),
reached through vatl_hip.conv2d_fwd(..., u_x6=) / conv1x1_dual_fwd(..., u_x6=): float64 parity inside the house bar of 2e-5 of the layer maximum (the
ring kernel's error on the same inputs is recorded beside it), exactness on data where the split must lose nothing, batch-position independence, the
refusals of the C entry points and the SimplePose-R50 plan with hip_engine.BF16X6 on against off."""
import ctypes

import numpy as np
import pytest
import torch

from tests.gpu_util import dev, record, rel_err, to_dev

pytestmark = pytest.mark.gpu

BAR = 2e-5         # of the layer maximum, against float64
BM = 5             # product knob: rows of the implicit-GEMM block tile (128 = whole 128-row tiles: the ring kernel serves the comparison launch)


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def _x6(vh, x, wp, ux6, sc, bi, cout, relu, res=None):
    with vh.flop_meter() as fm:
        y = vh.conv2d_fwd(x, wp, sc, bi, cout, 1, 1, 1, 0, relu, residual=res, u_x6=ux6)
    assert fm.routes["gemm1x1_bf16x6"] == 1 and sum(fm.routes.values()) == 1, fm.routes
    return y


def _ring(vh, fn):
    """fn() on the fp32 ring kernel (whole 128-row tiles forced, as tests/test_gpu_gemm1x1_ring.py does)."""
    try:
        vh.tune_set(BM, 128)
        with vh.flop_meter() as fm:
            y = fn()
    finally:
        vh.tune_set(BM, 0)
    assert fm.routes["gemm1x1_ring"] == 1, fm.routes
    return y


def _layer(r, cin, cout):
    w = (r.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)
    return w, r.uniform(0.5, 1.5, cout).astype(np.float32), r.standard_normal(cout).astype(np.float32)


# (n, H, W, K, N, residual): one partial tile (M = 48) | one full tile plus tail, two n-tiles | the longest K | residual epilogue, wide N
PLAIN = ((1, 8, 6, 512, 128, False), (3, 8, 6, 1024, 256, False), (2, 16, 12, 2048, 512, False), (3, 8, 6, 512, 2048, True))


@pytest.mark.parametrize("case", PLAIN, ids=lambda c: "x".join(str(v) for v in c[:5]) + ("_res" if c[5] else ""))
def test_plain_form_against_float64(vh, case):
    n, h, w_, k, cout, use_res = case
    r = np.random.RandomState(k + cout)
    w, sc, bi = _layer(r, k, cout)
    x = r.standard_normal((n, h, w_, k)).astype(np.float32)
    rs = r.standard_normal((n, h, w_, cout)).astype(np.float32) if use_res else None
    want = (x.astype(np.float64).reshape(-1, k) @ w.T.astype(np.float64)) * sc + bi
    want = np.maximum(want + (rs.reshape(-1, cout) if use_res else 0.0), 0).reshape(n, h, w_, cout)
    xd, scd, bid, rsd = to_dev(x), to_dev(sc), to_dev(bi), to_dev(rs) if use_res else None
    wp = vh.pack_conv_weight(to_dev(w.reshape(cout, k, 1, 1)))
    got = _x6(vh, xd, wp, vh.pack_gemm1x1_bf16x6_weight(wp), scd, bid, cout, True, rsd)
    ring = _ring(vh, lambda: vh.conv2d_fwd(xd, wp, scd, bid, cout, 1, 1, 1, 0, True, residual=rsd))
    e, er = rel_err(got.cpu().numpy(), want), rel_err(ring.cpu().numpy(), want)
    record(f"gemm1x1_bf16x6_{n}x{h}x{w_}x{k}_{cout}", vs_fp64=e, ring_vs_fp64=er)
    print(f"bf16x6 {case}: route {e:.3e}  ring {er:.3e}")
    assert e < BAR, (e, er)


# (n, Ho, Wo, C1, H2, W2, C2, stride, N): the widest dual launch | 12 k-tiles, the shortest admitted
DUAL = ((2, 8, 6, 512, 16, 12, 1024, 2, 2048), (1, 32, 24, 128, 64, 48, 256, 2, 512))


@pytest.mark.parametrize("case", DUAL, ids=lambda c: f"{c[3]}+{c[6]}_{c[8]}")
def test_dual_form_against_float64(vh, case):
    n, ho, wo, c1, h2, w2, c2, stride, cout = case
    r = np.random.RandomState(c1 + c2)
    w1, s1, b1 = _layer(r, c1, cout)
    w2_, s2, b2 = _layer(r, c2, cout)
    a = r.standard_normal((n, ho, wo, c1)).astype(np.float32)
    x = r.standard_normal((n, h2, w2, c2)).astype(np.float32)
    xs = x[:, ::stride, ::stride][:, :ho, :wo].astype(np.float64).reshape(-1, c2)
    want = (a.astype(np.float64).reshape(-1, c1) @ w1.T.astype(np.float64)) * s1 + b1 + (xs @ w2_.T.astype(np.float64)) * s2 + b2
    want = np.maximum(want, 0).reshape(n, ho, wo, cout)
    wp, bias = vh.pack_conv1x1_dual_weight(to_dev(w1.reshape(cout, c1, 1, 1)), to_dev(s1), to_dev(b1), to_dev(w2_.reshape(cout, c2, 1, 1)), to_dev(s2), to_dev(b2))
    ad, xd = to_dev(a), to_dev(x)
    with vh.flop_meter() as fm:
        got = vh.conv1x1_dual_fwd(ad, xd, wp, bias, cout, stride, True, u_x6=vh.pack_gemm1x1_bf16x6_weight(wp))
    assert fm.routes["gemm1x1_bf16x6"] == 1 and sum(fm.routes.values()) == 1, fm.routes
    ring = _ring(vh, lambda: vh.conv1x1_dual_fwd(ad, xd, wp, bias, cout, stride, True))
    e, er = rel_err(got.cpu().numpy(), want), rel_err(ring.cpu().numpy(), want)
    record(f"gemm1x1_bf16x6_dual_{c1}+{c2}_{cout}", vs_fp64=e, ring_vs_fp64=er)
    print(f"bf16x6 dual {case}: route {e:.3e}  ring {er:.3e}")
    assert e < BAR, (e, er)


def test_identity_and_permutation_filters_return_the_input_bits(vh):
    """W[n][k] = 1 at k == n (and at k == perm[n]: an asymmetric filter), full-mantissa inputs, scale 1, bias 0: the three pieces of every input add back
    to the input exactly, so the output IS the (permuted) input — the split loses nothing and plane, lane and k order are right."""
    r = np.random.RandomState(3)
    k = cout = 512
    x = to_dev(r.standard_normal((3, 8, 6, k)).astype(np.float32))
    for perm in (np.arange(k), r.permutation(k)):
        w = np.zeros((cout, k), np.float32)
        w[np.arange(cout), perm] = 1.0
        wp = vh.pack_conv_weight(to_dev(w.reshape(cout, k, 1, 1)))
        y = _x6(vh, x, wp, vh.pack_gemm1x1_bf16x6_weight(wp), None, None, cout, False)
        assert torch.equal(y, x[..., torch.as_tensor(perm, device=dev())])


def test_small_integers_are_exact(vh):
    r = np.random.RandomState(4)
    n, h, w_, k, cout = 2, 9, 11, 1024, 256             # M = 198: a tail of 70 rows
    x = r.randint(-8, 9, (n, h, w_, k)).astype(np.float32)
    w = r.randint(-4, 5, (cout, k)).astype(np.float32)
    want = x.astype(np.int64).reshape(-1, k) @ w.T.astype(np.int64)                # |sum| <= 1024 * 32: exact in fp32
    wp = vh.pack_conv_weight(to_dev(w.reshape(cout, k, 1, 1)))
    y = _x6(vh, to_dev(x), wp, vh.pack_gemm1x1_bf16x6_weight(wp), None, None, cout, False)
    assert np.array_equal(y.cpu().numpy().reshape(-1, cout).astype(np.int64), want) and np.array_equal(y.cpu().numpy().reshape(-1, cout), want.astype(np.float32))


def test_inputs_at_every_exponent_stay_inside_the_bar(vh):
    """Row m holds +-2^e (1 + 2^-23), e = m - 100 for m = 0 .. 200 (two non-zero pieces far apart, the middle one empty): every row, taken as a layer of
    its own, is inside the bar — the pieces of tiny and of large inputs are neither lost nor overflow."""
    r = np.random.RandomState(6)
    k, cout, m = 512, 128, 201
    w, sc, bi = _layer(r, k, cout)
    e = np.arange(m) - 100
    x = (np.ldexp(1.0 + 2.0 ** -23, e)[:, None] * r.choice([-1.0, 1.0], (m, k))).astype(np.float32)
    want = x.astype(np.float64) @ w.T.astype(np.float64)
    wp = vh.pack_conv_weight(to_dev(w.reshape(cout, k, 1, 1)))
    y = _x6(vh, to_dev(x.reshape(1, 3, 67, k)), wp, vh.pack_gemm1x1_bf16x6_weight(wp), None, None, cout, False).cpu().numpy().reshape(m, cout)
    worst = max(rel_err(y[i], want[i]) for i in range(m))
    record("gemm1x1_bf16x6_exponents", worst_row=worst)
    assert worst < BAR, worst


def test_rows_do_not_depend_on_their_neighbours(vh):
    """Rows 0, 50 and 143 of the M = 144 case equal the same rows computed alone, and an image keeps its bits between NaN-filled neighbours."""
    r = np.random.RandomState(8)
    n, h, w_, k, cout = 3, 8, 6, 1024, 256
    w, sc, bi = _layer(r, k, cout)
    x = to_dev(r.standard_normal((n, h, w_, k)).astype(np.float32))
    rs = to_dev(r.standard_normal((n, h, w_, cout)).astype(np.float32))
    scd, bid = to_dev(sc), to_dev(bi)
    wp = vh.pack_conv_weight(to_dev(w.reshape(cout, k, 1, 1)))
    ux6 = vh.pack_gemm1x1_bf16x6_weight(wp)
    full = _x6(vh, x, wp, ux6, scd, bid, cout, True, rs)
    for row in (0, 50, 143):
        solo = _x6(vh, x.reshape(-1, k)[row].reshape(1, 1, 1, k).contiguous(), wp, ux6, scd, bid, cout, True, rs.reshape(-1, cout)[row].reshape(1, 1, 1, cout).contiguous())
        assert torch.equal(solo.reshape(-1), full.reshape(-1, cout)[row]), row
    xn = torch.full_like(x, float("nan"))
    xn[1] = x[1]
    poisoned = _x6(vh, xn, wp, ux6, scd, bid, cout, True, rs)
    assert torch.equal(poisoned[1], full[1])          # (the NaN rows themselves come out as fmaxf(NaN, 0) = 0, as from every conv epilogue here)


def test_unsupported_shapes_are_refused_with_nothing_launched(vh):
    """K = 448, N = 192, stride 2 and a residual on the dual form: the shape query says no, the C entry points fail, nothing is launched and y keeps its bytes;
    the Python entry points ignore u_x6 on such shapes."""
    lib = vh.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    buf = torch.zeros(1 << 22, device=dev())             # stands in for every operand: a refused call reads none of them
    y = torch.full((1 << 20,), 7.0, device=dev())
    assert not vh.gemm1x1_bf16x6_supported(48, 448, 0, 128) and not vh.gemm1x1_bf16x6_supported(48, 512, 0, 192)
    assert not vh.gemm1x1_bf16x6_supported(48, 320, 128, 512) and not vh.gemm1x1_bf16x6_supported(48, 544, 32, 512) and vh.gemm1x1_bf16x6_supported(48, 384, 128, 512)
    with vh.flop_meter() as fm:
        for cin, cout, stride in ((448, 128, 1), (512, 192, 1), (512, 128, 2)):
            rc = lib.vatl_gemm1x1_bf16x6_fwd(p(buf), p(buf), None, None, None, p(y), 1, 8, 6, cin, cout, stride, 0, None)
            assert rc != 0 and b"gemm1x1_bf16x6_fwd" in lib.vatl_last_error(), (cin, cout, stride)
        rc = lib.vatl_gemm1x1_bf16x6_dual_fwd(p(buf), p(buf), p(buf), None, p(buf), p(y), 1, 8, 6, 512, 16, 12, 1024, 2, 2048, 0, None)
        assert rc != 0 and b"residual" in lib.vatl_last_error()
        rc = lib.vatl_gemm1x1_bf16x6_dual_fwd(p(buf), p(buf), p(buf), None, None, p(y), 1, 8, 6, 32, 16, 12, 480, 2, 512, 0, None)
        assert rc != 0
        assert vh.flop_meter.launches_now() == 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    # the keyword is ignored where the route does not apply: the plain kernels' bits
    r = np.random.RandomState(9)
    x = to_dev(r.standard_normal((1, 8, 6, 448)).astype(np.float32))
    wp = vh.pack_conv_weight(to_dev((r.standard_normal((128, 448, 1, 1)) / 21).astype(np.float32)))
    with vh.flop_meter() as fm:
        got = vh.conv2d_fwd(x, wp, None, None, 128, 1, 1, 1, 0, False, u_x6=buf)
    assert fm.routes["gemm1x1_bf16x6"] == 0 and torch.equal(got, vh.conv2d_fwd(x, wp, None, None, 128, 1, 1, 1, 0, False))


def test_simplepose_plan_with_the_route_on_and_off(vh, monkeypatch):
    """SimplePose-R50 on 8 crops: with BF16X6 on the 14 long-K 1x1 layers and the 3 conv3 + projection launches of stages 2 - 4 take the route (counted from the
    model by the shape rule), with it off none does and the launch count is the same; heat-maps within 1e-5 of their maximum, arg-max identical."""
    from alphapose.models import hip_engine
    from oracle import synth
    from tests.test_gpu_conv import _build_simplepose
    m = _build_simplepose()
    x = to_dev(synth.crops(8))
    routed = 0
    for stage in m.preact.stages():
        for blk in stage:
            fused = blk.downsample is not None
            for c in [blk.conv1] + ([] if fused else [blk.conv3]):
                routed += c.kernel_size == (1, 1) and c.stride == (1, 1) and vh.gemm1x1_bf16x6_supported(8 * 48, c.in_channels, 0, c.out_channels)
            if fused:
                c1, c2 = blk.conv3.in_channels, blk.downsample[0].in_channels
                routed += vh.gemm1x1_bf16x6_supported(8 * 48, c1 + c2, c1, blk.conv3.out_channels)
    assert routed == 17, routed
    on, off = torch.empty((8, 17, 64, 48), device=dev()), torch.empty((8, 17, 64, 48), device=dev())
    assert hip_engine.BF16X6 is True
    m.__dict__.pop("_vatl_plan", None)
    with torch.no_grad(), vh.flop_meter() as fm:
        hip_engine.forward_into(m, x, on)
    assert fm.routes["gemm1x1_bf16x6"] == routed, fm.routes
    monkeypatch.setattr(hip_engine, "BF16X6", False)
    m.__dict__.pop("_vatl_plan", None)
    with torch.no_grad(), vh.flop_meter() as fo:
        hip_engine.forward_into(m, x, off)
    m.__dict__.pop("_vatl_plan", None)
    assert fo.routes["gemm1x1_bf16x6"] == 0 and sum(fo.routes.values()) == sum(fm.routes.values()), (fm.routes, fo.routes)
    e = rel_err(on.cpu().numpy(), off.cpu().numpy())
    record("bf16x6_vs_fp32_simplepose_r50", rel=e)
    print(f"bf16x6 plan: heat-maps on vs off {e:.3e}")
    assert e < 1e-5 and torch.equal(on.flatten(2).argmax(-1), off.flatten(2).argmax(-1)), e
