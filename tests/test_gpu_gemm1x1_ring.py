"""The LDS-DMA ring kernel for long-K 1x1 layers (csrc/gemm1x1_ring.hip, gemm1x1_ring_kernel), which the default k-loop schedule
(vatl_tune_set(0, 4)) takes for them: bit-identical to the tiled implicit GEMM that the other schedules run (vatl_tune_set(0, 2) here;
the schedules' mutual bit-identity is pinned in tests/test_gpu_conv.py), float64 parity, batch-position independence and the routes."""
import numpy as np
import pytest
import torch

from tests.gpu_util import record, rel_err, to_dev

pytestmark = pytest.mark.gpu

VAR = 0            # product knob: k-loop schedule; 4 (default) = ring kernel for these layers, 2 = tiled kernel
BM = 5             # product knob: rows of the implicit-GEMM block tile (128 forces whole 128-row tiles on both paths)


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def _both(vh, fn):
    """fn() with the ring route on and off (128-row tiles on both), and the routes the 'on' call took."""
    try:
        vh.tune_set(BM, 128)
        vh.tune_set(VAR, 2)
        with vh.flop_meter() as fo:
            off = fn().clone()
        vh.tune_set(VAR, 4)
        with vh.flop_meter() as fm:
            on = fn().clone()
        torch.cuda.synchronize()
    finally:
        vh.tune_set(BM, 0)
        vh.tune_set(VAR, 4)
    assert fo.routes["gemm1x1_ring"] == 0 and fo.routes["igemm"] == 1, fo.routes
    return on, off, fm.routes


def _layer(r, cin, cout, sb):
    w = (r.standard_normal((cout, cin, 1, 1)) / np.sqrt(cin)).astype(np.float32)
    sc = r.uniform(0.5, 1.5, cout).astype(np.float32) if sb else None
    bi = r.standard_normal(cout).astype(np.float32) if sb else None
    return w, sc, bi


@pytest.mark.parametrize("K", [512, 1024, 2048])
def test_ring_is_bit_identical_to_the_tiled_kernel(vh, K):
    """torch.equal against conv2d_fwd with the route off: N in {128 .. 2048}, with / without scale-bias, residual and ReLU, pixel
    counts of one pixel, M = 127, 129 and a tail on the last tile."""
    r = np.random.RandomState(K)
    shapes = ((1, 1, 1), (1, 127, 1), (1, 129, 1), (3, 13, 11))          # (N, H, W): M = 1, 127, 129, 429 (tail of 45 rows)
    couts = (128, 256, 512, 1024, 2048)
    for cout in couts:
        w, sc, bi = _layer(r, K, cout, True)
        wp = vh.pack_conv_weight(to_dev(w))
        for n, h, wd in shapes:
            x = to_dev(r.standard_normal((n, h, wd, K)).astype(np.float32))
            rs = to_dev(r.standard_normal((n, h, wd, cout)).astype(np.float32))
            for relu, use_res, use_sb in ((True, True, True), (False, False, False), (True, False, True), (False, True, False)):
                s_, b_ = (to_dev(sc), to_dev(bi)) if use_sb else (None, None)
                on, off, routes = _both(vh, lambda: vh.conv2d_fwd(x, wp, s_, b_, cout, 1, 1, 1, 0, relu, residual=rs if use_res else None))
                assert routes["gemm1x1_ring"] == 1 and routes["igemm"] == 0, routes
                assert torch.equal(on, off), (K, cout, n, h, wd, relu, use_res, use_sb)


@pytest.mark.parametrize("stride", [1, 2])
def test_dual_ring_is_bit_identical_to_the_tiled_kernel(vh, stride):
    """The dual-source form (conv3 + projection shortcut) against conv1x1_dual_fwd with the route off, at the three headline
    channel splits and ragged pixel counts."""
    r = np.random.RandomState(40 + stride)
    for c1, c2, cout in ((128, 256, 512), (256, 512, 1024), (512, 1024, 2048)):
        w1, s1, b1 = _layer(r, c1, cout, True)
        w2, s2, b2 = _layer(r, c2, cout, True)
        wp, bias = vh.pack_conv1x1_dual_weight(to_dev(w1), to_dev(s1), to_dev(b1), to_dev(w2), to_dev(s2), to_dev(b2))
        for n, ho, wo in ((1, 1, 1), (2, 8, 6), (3, 9, 5)):
            h2, w2_ = (ho - 1) * stride + 1 + (stride - 1), (wo - 1) * stride + 1 + (stride - 1)
            a = to_dev(r.standard_normal((n, ho, wo, c1)).astype(np.float32))
            x = to_dev(r.standard_normal((n, h2, w2_, c2)).astype(np.float32))
            for relu in (True, False):
                on, off, routes = _both(vh, lambda: vh.conv1x1_dual_fwd(a, x, wp, bias, cout, stride, relu))
                assert routes["gemm1x1_ring"] == 1 and routes["igemm"] == 0, routes
                assert torch.equal(on, off), (c1, c2, cout, n, ho, wo, relu)


@pytest.mark.parametrize("K", [512, 1024, 2048])
def test_ring_vs_float64(vh, K):
    """One float64 check per K (scale / bias, residual, ReLU; a tail tile), the bound of the other 1x1 tests."""
    r = np.random.RandomState(7 + K)
    n, h, wd, cout = 2, 9, 13, 256
    w, sc, bi = _layer(r, K, cout, True)
    x = r.standard_normal((n, h, wd, K)).astype(np.float32)
    rs = r.standard_normal((n, h, wd, cout)).astype(np.float32)
    want = np.maximum((x.astype(np.float64) @ w[:, :, 0, 0].T.astype(np.float64)) * sc + bi + rs, 0)
    try:
        vh.tune_set(BM, 128)
        with vh.flop_meter() as fm:
            got = vh.conv2d_fwd(to_dev(x), vh.pack_conv_weight(to_dev(w)), to_dev(sc), to_dev(bi), cout, 1, 1, 1, 0, True, residual=to_dev(rs))
        got = got.cpu().numpy()
    finally:
        vh.tune_set(BM, 0)
    assert fm.routes["gemm1x1_ring"] == 1
    e = rel_err(got, want)
    record(f"gemm1x1_ring_K{K}", vs_fp64=e)
    assert e < 2e-6, e


def test_a_crop_has_the_same_bits_alone_and_in_a_batch(vh):
    """THC de-duplication compares crops across batches: a crop computed alone equals its slice of a batch (plain and dual form)."""
    r = np.random.RandomState(5)
    cin, cout = 1024, 256
    w, sc, bi = _layer(r, cin, cout, True)
    wp = vh.pack_conv_weight(to_dev(w))
    x = to_dev(r.standard_normal((7, 16, 12, cin)).astype(np.float32))
    rs = to_dev(r.standard_normal((7, 16, 12, cout)).astype(np.float32))
    w1, s1, b1 = _layer(r, 256, 1024, True)
    w2, s2, b2 = _layer(r, 512, 1024, True)
    dwp, dbias = vh.pack_conv1x1_dual_weight(to_dev(w1), to_dev(s1), to_dev(b1), to_dev(w2), to_dev(s2), to_dev(b2))
    a = to_dev(r.standard_normal((7, 8, 6, 256)).astype(np.float32))
    x2 = to_dev(r.standard_normal((7, 16, 12, 512)).astype(np.float32))
    try:
        vh.tune_set(BM, 128)
        with vh.flop_meter() as fm:
            full = vh.conv2d_fwd(x, wp, to_dev(sc), to_dev(bi), cout, 1, 1, 1, 0, True, residual=rs)
            dfull = vh.conv1x1_dual_fwd(a, x2, dwp, dbias, 1024, 2, True)
            for i in (0, 3, 6):
                solo = vh.conv2d_fwd(x[i:i + 1].contiguous(), wp, to_dev(sc), to_dev(bi), cout, 1, 1, 1, 0, True, residual=rs[i:i + 1].contiguous())
                assert torch.equal(solo, full[i:i + 1]), i
                dsolo = vh.conv1x1_dual_fwd(a[i:i + 1].contiguous(), x2[i:i + 1].contiguous(), dwp, dbias, 1024, 2, True)
                assert torch.equal(dsolo, dfull[i:i + 1]), i
    finally:
        vh.tune_set(BM, 0)
    assert fm.routes["gemm1x1_ring"] == 8 and fm.routes["igemm"] == 0, fm.routes


# long-K 1x1 layers of the headline step (SimplePose-R50, 256 x 192 crops, 1024 per launch): (H, W, K, N)
HEADLINE_1X1 = (("l2.n.c1", 32, 24, 512, 128), ("l3.0.c1", 32, 24, 512, 256), ("l3.n.c1", 16, 12, 1024, 256),
                ("l4.0.c1", 16, 12, 1024, 512), ("l4.n.c1", 8, 6, 2048, 512), ("l4.n.c3", 8, 6, 512, 2048))
HEADLINE_DUAL = (("l2.0.c3+p", 32, 24, 128, 64, 48, 256, 512), ("l3.0.c3+p", 16, 12, 256, 32, 24, 512, 1024),
                 ("l4.0.c3+p", 8, 6, 512, 16, 12, 1024, 2048))


def test_headline_shapes_take_the_ring_and_training_launches_do_not(vh):
    """At the headline batch the long-K 1x1 launches (default tile choice) run on the ring kernel; the fine-tune step's statistics
    launches of the same shapes stay on the tiled kernel, and another k-loop schedule sends the inference launches back to it."""
    n = 1024
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    for name, h, w, k, cout in HEADLINE_1X1:
        x = torch.randn((n, h, w, k), device="cuda", generator=g)
        wp = vh.pack_conv_weight(torch.randn((cout, k, 1, 1), device="cuda", generator=g) / k ** 0.5)
        sc, bi = torch.ones(cout, device="cuda"), torch.zeros(cout, device="cuda")
        with vh.flop_meter() as fm:
            vh.conv2d_fwd(x, wp, sc, bi, cout, 1, 1, 1, 0, True)
        assert fm.routes["gemm1x1_ring"] == 1, (name, fm.routes)
        gm, bt = torch.ones(cout, device="cuda"), torch.zeros(cout, device="cuda")
        rm, rv = torch.zeros(cout, device="cuda"), torch.ones(cout, device="cuda")
        with vh.flop_meter() as fm:
            vh.conv2d_fwd_bnstats(x, wp, cout, 1, 1, 1, 0, gm, bt, rm, rv, 0.1, 1e-5)
        assert fm.routes["gemm1x1_ring"] == 0 and fm.routes["igemm"] == 1, (name, fm.routes)
        try:
            vh.tune_set(VAR, 2)
            with vh.flop_meter() as fm:
                vh.conv2d_fwd(x, wp, sc, bi, cout, 1, 1, 1, 0, True)
        finally:
            vh.tune_set(VAR, 4)
        assert fm.routes["gemm1x1_ring"] == 0 and fm.routes["igemm"] == 1, (name, fm.routes)
        del x
    for name, ho, wo, c1, h2, w2, c2, cout in HEADLINE_DUAL:
        a = torch.randn((n, ho, wo, c1), device="cuda", generator=g)
        x = torch.randn((n, h2, w2, c2), device="cuda", generator=g)
        wp, bias = vh.pack_conv1x1_dual_weight(torch.randn((cout, c1, 1, 1), device="cuda", generator=g) / c1 ** 0.5, torch.ones(cout, device="cuda"),
                                               torch.zeros(cout, device="cuda"), torch.randn((cout, c2, 1, 1), device="cuda", generator=g) / c2 ** 0.5,
                                               torch.ones(cout, device="cuda"), torch.zeros(cout, device="cuda"))
        with vh.flop_meter() as fm:
            vh.conv1x1_dual_fwd(a, x, wp, bias, cout, 2, True)
        assert fm.routes["gemm1x1_ring"] == 1, (name, fm.routes)
        del a, x
    torch.cuda.synchronize()


def test_plain_data_gradient_launches_take_the_ring_with_the_same_bits(vh):
    """The fine-tune step's data-gradient launches of 1x1 / stride-1 layers without a BatchNorm-backward epilogue (vatl_conv2d_fwd_ex, skip
    gradient added as the residual) are plain GEMMs over K = the layer's output channels: they take the ring kernel where the shape
    qualifies, with the bits of the tiled kernel."""
    r = np.random.RandomState(77)
    n, h, w, k, cout = 5, 16, 12, 512, 128          # dL/dy of a 128 -> 512 conv3 (K = 512) -> dL/dx (128 channels)
    g = to_dev(r.standard_normal((n, h, w, k)).astype(np.float32))
    wt = vh.pack_conv_weight(to_dev((r.standard_normal((cout, k, 1, 1)) / np.sqrt(k)).astype(np.float32)))
    skip = to_dev(r.standard_normal((n, h, w, cout)).astype(np.float32))
    on, off, routes = _both(vh, lambda: vh.conv2d_fwd_ex(g, wt, cout, 1, 1, 1, 0, 0, h, w, h, w, 1, 1, 0, 0, residual=skip))
    assert routes["gemm1x1_ring"] == 1, routes
    assert torch.equal(on, off)
