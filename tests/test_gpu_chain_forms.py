"""The two chained launches of csrc/bottleneck_chain.hip's chain_form_kernel against the launches they replace and against float64:
  form P (vh.conv1x1_rows_fwd(..., x2=, next_conv1=)): conv3 + projection shortcut of a stage's first block (dual-source GEMM, K = 64 + 64) and the next block's 256 -> 64 conv1;
  form S (vh.bottleneck_chain_fwd(..., next_stage_conv1=)): conv3 + skip of a stage's last block and the 256 -> 128 conv1 of the next stage's first block.
T (the 256-channel block output) must have the bits of the launch replaced in both forms.  Y of form S walks K in the order of conv1x1_rows256_kernel: bit-equal too.
Y of form P sums K in another order than the tiled GEMM: within 1e-5 of the largest output (the bar of the existing chain test's plan check); everything within 2e-5 of float64."""
import numpy as np
import pytest
import torch

from tests.gpu_util import dev, record, rel_err, to_dev

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 5, 7), (3, 16, 12), (6, 64, 48)]      # less than a tile; a tail tile (M = 35); whole tiles; 576 tiles > the 512-block grid
Y_BAR, F64_BAR = 1e-5, 2e-5


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


class _Form:
    """Weights of one form and its three evaluations: the two launches replaced, the chained launch, float64."""

    def __init__(self, vh, name):
        self.vh, self.name, self.n2 = vh, name, 64 if name == "P" else 128
        r = np.random.RandomState(11 if name == "P" else 12)
        self.w3 = (r.standard_normal((256, 64, 1, 1)) / 8).astype(np.float32)
        self.s3, self.b3 = r.uniform(0.5, 1.5, 256).astype(np.float32), r.standard_normal(256).astype(np.float32)
        self.wp = (r.standard_normal((256, 64, 1, 1)) / 8).astype(np.float32)                  # P: projection shortcut
        self.sp, self.bp = r.uniform(0.5, 1.5, 256).astype(np.float32), r.standard_normal(256).astype(np.float32)
        self.w1 = (r.standard_normal((self.n2, 256, 1, 1)) / 16).astype(np.float32)
        self.s1, self.b1 = r.uniform(0.5, 1.5, self.n2).astype(np.float32), r.standard_normal(self.n2).astype(np.float32)
        self.s3d, self.b3d, self.s1d, self.b1d = to_dev(self.s3), to_dev(self.b3), to_dev(self.s1), to_dev(self.b1)
        self.w3p, self.w1p = vh.pack_conv_weight(to_dev(self.w3)), vh.pack_conv_weight(to_dev(self.w1))
        self.dual, self.dbias = vh.pack_conv1x1_dual_weight(to_dev(self.w3), self.s3d, self.b3d, to_dev(self.wp), to_dev(self.sp), to_dev(self.bp))
        self.rng = r

    def inputs(self, n, h, w):
        """(a, second): second = the block input (P) or the skip tensor (S)."""
        a = self.rng.standard_normal((n, h, w, 64)).astype(np.float32)
        second = self.rng.standard_normal((n, h, w, 64 if self.name == "P" else 256)).astype(np.float32)
        return a, second

    def conv1(self, plain=False):
        return (self.w1p, None, None) if plain else (self.w1p, self.s1d, self.b1d)

    def fused(self, a, second, plain=False, **kw):
        vh = self.vh
        if self.name == "P":
            return vh.conv1x1_rows_fwd(a, self.dual, None, None if plain else self.dbias, 256, True, x2=second, next_conv1=self.conv1(plain), **kw)
        s3, b3 = (None, None) if plain else (self.s3d, self.b3d)
        return vh.bottleneck_chain_fwd(a, self.w3p, s3, b3, second, next_stage_conv1=self.conv1(plain), **kw)

    def two(self, a, second, plain=False):
        vh = self.vh
        w1p, s1, b1 = self.conv1(plain)
        if self.name == "P":
            t = vh.conv1x1_rows_fwd(a, self.dual, None, None if plain else self.dbias, 256, True, x2=second)
            return t, vh.conv2d_fwd(t, w1p, s1, b1, 64, 1, 1, 1, 0, True)
        s3, b3 = (None, None) if plain else (self.s3d, self.b3d)
        t = vh.bottleneck_chain_fwd(a, self.w3p, s3, b3, second)[0]
        return t, vh.conv1x1_rows_fwd(t, w1p, s1, b1, 128, True)

    def float64(self, a, second):
        f = lambda w: w[:, :, 0, 0].T.astype(np.float64)
        t = (a.astype(np.float64) @ f(self.w3)) * self.s3 + self.b3
        t = t + ((second.astype(np.float64) @ f(self.wp)) * self.sp + self.bp if self.name == "P" else second)
        t = np.maximum(t, 0)
        return t, np.maximum((t @ f(self.w1)) * self.s1 + self.b1, 0)


@pytest.fixture(scope="module")
def forms(vh):
    return {k: _Form(vh, k) for k in ("P", "S")}


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("name", ["P", "S"])
def test_against_the_two_launches_and_float64(forms, name, shape):
    f = forms[name]
    a, second = f.inputs(*shape)
    ad, sd = to_dev(a), to_dev(second)
    t2, y2 = f.two(ad, sd)
    t, y = f.fused(ad, sd)
    assert t.shape == shape + (256,) and y.shape == shape + (f.n2,)
    t64, y64 = f.float64(a, second)
    e_y = rel_err(y.cpu().numpy(), y2.cpu().numpy())
    e_t64, e_y64 = rel_err(t.cpu().numpy(), t64), rel_err(y.cpu().numpy(), y64)
    record(f"chain_form_{name}_{'x'.join(map(str, shape))}", y_vs_two_launches=e_y, t_vs_fp64=e_t64, y_vs_fp64=e_y64,
           two_launches_t_vs_fp64=rel_err(t2.cpu().numpy(), t64), two_launches_y_vs_fp64=rel_err(y2.cpu().numpy(), y64))
    print(f"form {name} {shape}: y vs two launches {e_y:.3e}, t vs fp64 {e_t64:.3e}, y vs fp64 {e_y64:.3e}")
    assert torch.equal(t, t2)
    if name == "S":
        assert torch.equal(y, y2)
    assert e_y < Y_BAR and e_t64 < F64_BAR and e_y64 < F64_BAR


@pytest.mark.parametrize("name", ["P", "S"])
def test_optional_operands(vh, forms, name):
    """No folded BN on either GEMM; S without a skip tensor."""
    f = forms[name]
    a, second = f.inputs(3, 16, 12)
    ad, sd = to_dev(a), to_dev(second)
    t2, y2 = f.two(ad, sd, plain=True)
    t, y = f.fused(ad, sd, plain=True)
    assert torch.equal(t, t2) and rel_err(y.cpu().numpy(), y2.cpu().numpy()) < Y_BAR and (name == "P" or torch.equal(y, y2))
    if name == "S":
        t2 = vh.bottleneck_chain_fwd(ad, f.w3p, f.s3d, f.b3d, None)[0]
        t, y = vh.bottleneck_chain_fwd(ad, f.w3p, f.s3d, f.b3d, None, next_stage_conv1=f.conv1())
        assert torch.equal(t, t2) and torch.equal(y, vh.conv1x1_rows_fwd(t2, f.w1p, f.s1d, f.b1d, 128, True))


@pytest.mark.parametrize("name", ["P", "S"])
def test_out_buffers_are_overwritten_completely(forms, name):
    f = forms[name]
    a, second = f.inputs(2, 9, 5)                                  # M = 90: two whole tiles and a tail
    ad, sd = to_dev(a), to_dev(second)
    t_ref, y_ref = f.fused(ad, sd)
    t = torch.full((2, 9, 5, 256), -777.0, device=dev()); y = torch.full((2, 9, 5, f.n2), -777.0, device=dev())
    t_got, y_got = f.fused(ad, sd, out=t, y1_out=y)
    assert t_got.data_ptr() == t.data_ptr() and y_got.data_ptr() == y.data_ptr()
    assert torch.equal(t, t_ref) and torch.equal(y, y_ref) and not (t == -777.0).any() and not (y == -777.0).any()


@pytest.mark.parametrize("name", ["P", "S"])
def test_rows_past_m_are_neither_read_nor_written(forms, name):
    """M = 35 inside larger buffers: NaN rows behind A and behind the second source do not reach the output, the rows behind T and Y keep their fill."""
    f = forms[name]
    a, second = f.inputs(1, 5, 7)
    t_ref, y_ref = f.fused(to_dev(a), to_dev(second))

    def backed(x, fill):
        big = torch.full((96, x.shape[-1]), fill, device=dev())
        big[:35] = to_dev(x).reshape(35, -1)
        return big, big[:35].view(1, 5, 7, x.shape[-1])
    _, av = backed(a, float("nan"))
    _, sv = backed(second, float("nan"))
    tb, tv = backed(np.zeros((35, 256), np.float32), -777.0)
    yb, yv = backed(np.zeros((35, f.n2), np.float32), -777.0)
    f.fused(av, sv, out=tv, y1_out=yv)
    assert torch.equal(tv, t_ref) and torch.equal(yv, y_ref)
    assert (tb[35:] == -777.0).all() and (yb[35:] == -777.0).all()


@pytest.mark.parametrize("name", ["P", "S"])
def test_a_crops_bits_do_not_depend_on_its_batch(forms, name):
    f = forms[name]
    a, second = f.inputs(3, 7, 9)                                  # 63 pixels per crop: every tile straddles two crops
    ad, sd = to_dev(a), to_dev(second)
    t, y = f.fused(ad, sd)
    t_again, y_again = f.fused(ad, sd)
    assert torch.equal(t, t_again) and torch.equal(y, y_again)
    ts, ys = f.fused(ad[1:2].contiguous(), sd[1:2].contiguous())
    assert torch.equal(ts, t[1:2]) and torch.equal(ys, y[1:2])


def test_refusals(vh, forms):
    m = 1024 * 64 * 48
    assert vh.chain_proj_supported(64, 256, 64, m) and vh.chain_step_supported(64, 256, 128, m)
    assert vh.chain_proj_supported(64, 256, 64, 1) and vh.chain_step_supported(64, 256, 128, 1)
    for fn, n2 in ((vh.chain_proj_supported, 64), (vh.chain_step_supported, 128)):
        assert not fn(128, 256, n2, 100) and not fn(64, 512, n2, 100) and not fn(64, 256, 192 - n2, 100) and not fn(64, 256, 0, 100)
        assert not fn(64, 256, n2, 0) and not fn(64, 256, n2, (1 << 22) - 32) and fn(64, 256, n2, (1 << 22) - 33)
    p, s = forms["P"], forms["S"]
    a, x = (to_dev(v) for v in p.inputs(1, 2, 2))
    r = np.random.RandomState(5)
    with pytest.raises(vh.VatlError):                              # P with the 256 -> 128 conv1
        vh.conv1x1_rows_fwd(a, p.dual, None, p.dbias, 256, True, x2=x, next_conv1=s.conv1())
    with pytest.raises(vh.VatlError):                              # P without the second source
        vh.conv1x1_rows_fwd(to_dev(r.standard_normal((1, 2, 2, 128)).astype(np.float32)), p.dual, None, p.dbias, 256, True, next_conv1=p.conv1())
    a, skip = (to_dev(v) for v in s.inputs(1, 2, 2))
    with pytest.raises(vh.VatlError):                              # S with the 256 -> 64 conv1
        vh.bottleneck_chain_fwd(a, s.w3p, s.s3d, s.b3d, skip, next_stage_conv1=p.conv1())
    with pytest.raises(vh.VatlError):                              # S with 32 mid channels
        vh.bottleneck_chain_fwd(a[..., :32].contiguous(), s.w3p[:, :, :, :32].contiguous(), s.s3d, s.b3d, skip, next_stage_conv1=s.conv1())
    with pytest.raises(vh.VatlError):                              # both continuations at once
        vh.bottleneck_chain_fwd(a, s.w3p, s.s3d, s.b3d, skip, *p.conv1(), next_stage_conv1=s.conv1())


@pytest.mark.parametrize("net", ["SimplePose", "HRNet"])
def test_plans_take_the_forms(vh, monkeypatch, net):
    """SimplePose-R50: stage 1 is (projection block, block, block) and stage 2 starts with a 256 -> 128 conv1: one P, the existing link, one S.
    HRNet-W32: layer1 is (projection block, 3 blocks) followed by the transitions: one P, two links and the first-GEMM-only launch, no S.
    Each switch restores the launches it replaced; heat-maps on against off within 1e-5 with equal arg-max."""
    from alphapose.models import hip_engine
    from tests.test_gpu_conv import HRNET_CFG, _build, _build_simplepose
    torch.manual_seed(5)
    m = _build_simplepose() if net == "SimplePose" else _build(HRNET_CFG)
    want = {"chain_proj": 1, "chain_step": 1, "bottleneck_chain": 1} if net == "SimplePose" else {"chain_proj": 1, "chain_step": 0, "bottleneck_chain": 3}
    x = torch.randn((3, 3, 256, 192), device=dev())

    def run():
        out = torch.empty((3, 17, 64, 48), device=dev())
        with torch.no_grad(), vh.flop_meter() as fm:
            hip_engine.forward_into(m, x, out)
        return out, fm.routes
    assert hip_engine.FUSE_CHAIN_PROJ is True and hip_engine.FUSE_CHAIN_STEP is True
    on, r_on = run()
    assert {k: r_on[k] for k in want} == want, r_on
    monkeypatch.setattr(hip_engine, "FUSE_CHAIN_PROJ", False)
    off_p, r_p = run()
    assert r_p["chain_proj"] == 0 and r_p["rows_1x1"] == r_on["rows_1x1"] + 1 and r_p["chain_step"] == want["chain_step"], r_p
    assert sum(r_p.values()) == sum(r_on.values()) + 1
    monkeypatch.setattr(hip_engine, "FUSE_CHAIN_STEP", False)
    off, r_off = run()
    assert r_off["chain_proj"] == 0 and r_off["chain_step"] == 0 and r_off["bottleneck_chain"] == want["bottleneck_chain"] + want["chain_step"], r_off
    assert r_off["rows_1x1"] == r_p["rows_1x1"] + want["chain_step"] and sum(r_off.values()) == sum(r_p.values()) + want["chain_step"]
    for name, other in (("proj_off", off_p), ("both_off", off)):
        e = rel_err(on.cpu().numpy(), other.cpu().numpy())
        record(f"chain_forms_{net}_{name}", on_vs_off=e)
        assert e < 1e-5 and torch.equal(on.flatten(2).argmax(-1), other.flatten(2).argmax(-1)), (name, e)
