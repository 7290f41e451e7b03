"""The ordered (bit-reproducible) dx of the deformable convolution on MI355X: the kernel's bits against the numpy float32 model of
tests/dcn_ordered_cases.py (the documented key order and arithmetic of include/vatl_hip.h), against the atomic entry and the float64
oracle; the workspace contract; the switch through the modules, the trainer and a whole FastPose-50-DCN fine-tune step.

Bars: normwise rel_err (tests/gpu_util.py) <= 2e-5 against float64, the bar of tests/test_gpu_dcn.py, and 4e-5 between the two entries
(each within 2e-5 of the same float64 values)."""
import numpy as np
import pytest
import torch

from tests import dcn_cases as D
from tests import dcn_ordered_cases as O
from tests.gpu_util import dev, record, rel_err, to_dev

pytestmark = pytest.mark.gpu

BAR = 2e-5
CASES = [("drawn", s) for s in D.ALL_CASES] + [("new", n) for n in O.NEW_CASES]
IDS = [s[0] if kind == "drawn" else s for kind, s in CASES]


def _case(kind, spec):
    return (D.case(spec), "drawn/" + spec[0]) if kind == "drawn" else (O.new_case(spec), spec)


def _nhwc(t):
    return None if t is None else to_dev(t.permute(0, 2, 3, 1).contiguous().numpy())


def _nchw64(t):
    return t.permute(0, 3, 1, 2).double().cpu()


def _check(name, what, got, ref, bar=BAR):
    e = rel_err(got.numpy(), ref.numpy())
    record("dcn_ordered", case=name, what=what, rel_err=e)
    print(f"{name} {what}: {e:.3e}")
    assert e <= bar, (name, what, e)


def _dcol(g):
    """(B, C, 9, Ho, Wo) -> the device rows (B, Ho, Wo, deform_col_stride(C)), zero behind 9 C."""
    import vatl_hip as vh
    b, c, _, ho, wo = g.shape
    out = torch.zeros((b, ho, wo, vh.deform_col_stride(c)), device=dev())
    out[..., :9 * c] = to_dev(O.dcol_rows(g).reshape(b, ho, wo, 9 * c))
    return out


def _index_bytes(n, h, w, stride, dg):
    """The formula of include/vatl_hip.h."""
    ho, wo = D.out_hw(h, w, stride)
    return (12 * n * h * w * dg + 15) // 16 * 16 + 8 * 4 * n * ho * wo * 9 * dg


def _ordered_raw(dcol, x, off, mask, stride, dg, ws_bytes=None):
    """vatl_deform_columns_bwd_ordered itself, on a dx full of NaN, gradients full of a sentinel and a workspace full of 0xFF bytes
    -> (rc, dx, d_offset, d_mask)."""
    import vatl_hip as vh
    (n, h, w, c, ho, wo), oargs = vh._deform_args("test", x, off, mask, stride, dg, False)
    dx = torch.full_like(x, float("nan"))
    d_off = torch.full((n, ho, wo, 18 * dg), -77.0, device=dev())
    d_mask = None if mask is None else torch.full((n, ho, wo, 9 * dg), -77.0, device=dev())
    need = _index_bytes(n, h, w, stride, dg)
    ws = torch.full((need if ws_bytes is None else ws_bytes,), 0xFF, dtype=torch.uint8, device=dev())
    rc = vh.lib().vatl_deform_columns_bwd_ordered(vh._ptr(dcol), dcol.shape[3], vh._ptr(x), *oargs, vh._ptr(dx), vh._ptr(d_off), 18 * dg,
                                                  vh._ptr(d_mask), 9 * dg if mask is not None else 0, n, h, w, c, stride, dg, ws.data_ptr(), ws.numel(),
                                                  vh._stream())
    torch.cuda.synchronize()
    return rc, dx, d_off, d_mask


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("kind,spec", CASES, ids=IDS)
def test_ordered_dx_has_the_models_bits(kind, spec):
    """v1 and direct-mask calls of every case as drawn (borders included) and of the pile-up, empty and dg 4 / stride 2 cases: dx, written
    over NaN from an index built over 0xFF bytes, has the bits of the model (an element left unwritten is NaN, a stale index word is a
    count of -1 or a NaN weight); a second call repeats them; d_offset and d_mask have the atomic entry's bits; the two dx agree."""
    import vatl_hip as vh
    c, tag = _case(kind, spec)
    g = O.grad_columns(c)
    m = O.direct_mask(c)
    x, off, mh, dcol = _nhwc(c["x"]), _nhwc(c["offset"]), _nhwc(m), _dcol(g)
    s, dg = c["stride"], c["dg"]
    rc, dx, d_off, d_mask = _ordered_raw(dcol, x, off, mh, s, dg)
    assert rc == 0, vh.lib().vatl_last_error()
    want = O.model_dx(tag, c, g)
    got = dx.cpu().numpy()
    assert not np.isnan(got).any(), f"{int(np.isnan(got).sum())} elements of dx left unwritten (or NaN)"
    differ = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert differ.size == 0, (tag, differ.size, got.reshape(-1)[differ[:4]], want.reshape(-1)[differ[:4]])
    if kind == "new" and spec == "empty":
        assert not _bits(dx).any() and not d_off.any()                                   # +0.0 everywhere, no offset gradient
    rc2, dx2, d_off2, d_mask2 = _ordered_raw(dcol, x, off, mh, s, dg)
    assert rc2 == 0 and np.array_equal(_bits(dx), _bits(dx2)) and torch.equal(d_off, d_off2)
    # the wrapper with deterministic=True is the same call; the atomic entry differs in dx only
    dx_w, d_off_w, d_mask_w = vh.deform_columns_bwd(dcol, x, off, mh, s, dg, deterministic=True)
    dx_a, d_off_a, d_mask_a = vh.deform_columns_bwd(dcol, x, off, mh, s, dg, deterministic=False)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dx_w), _bits(dx))
    assert np.array_equal(_bits(d_off), _bits(d_off_a)) and np.array_equal(_bits(d_off_w), _bits(d_off_a))
    if m is not None:
        assert np.array_equal(_bits(d_mask), _bits(d_mask_a)) and np.array_equal(_bits(d_mask_w), _bits(d_mask_a))
    else:
        assert d_mask is None and d_mask_a is None
    ref = O.oracle_dx(c, g)
    _check(tag, "ordered dx vs atomic dx", _nchw64(dx), _nchw64(dx_a), bar=4e-5)
    _check(tag, "ordered dx vs float64", _nchw64(dx), ref)
    _check(tag, "atomic dx vs float64", _nchw64(dx_a), ref)


@pytest.mark.parametrize("spec", [c for c in D.ALL_CASES if c[8]][:4] + [D.PRODUCT_CASES[0]], ids=lambda c: c[0])
def test_ordered_with_logits_behind_the_offsets(spec):
    """The trainer's layout (offsets and mask logits in one tensor, mask=True): run to run identical, within the bar of float64, and the
    offset / logit gradients with the atomic entry's bits."""
    import vatl_hip as vh
    c = D.smooth_offsets(D.make_case(*spec), 950)
    s, dg, cin = c["stride"], c["dg"], c["x"].shape[1]
    om64 = torch.cat([c["offset"], c["mask_logits"]], 1).clone().requires_grad_()
    x64 = c["x"].clone().requires_grad_()
    ref = D.deform_columns_ref(x64, om64[:, :18 * dg], torch.sigmoid(om64[:, 18 * dg:]), s, dg)
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(6)).double()
    wx, wom = torch.autograd.grad(ref, [x64, om64], g)
    x, om, dcol = _nhwc(c["x"]), _nhwc(om64.detach()), _dcol(g)
    gc = 32 * ((27 * dg + 31) // 32)
    runs = [vh.deform_columns_bwd(dcol, x, om, True, s, dg, grad_channels=gc, deterministic=True) for _ in range(3)]
    dx_a, d_om_a, _ = vh.deform_columns_bwd(dcol, x, om, True, s, dg, grad_channels=gc, deterministic=False)
    torch.cuda.synchronize()
    dx, d_om, d_mask = runs[0]
    assert d_mask is None and d_om[..., 27 * dg:].abs().max().item() == 0
    for dx_r, d_om_r, _ in runs[1:]:
        assert np.array_equal(_bits(dx), _bits(dx_r)) and np.array_equal(_bits(d_om), _bits(d_om_r))
    assert np.array_equal(_bits(d_om), _bits(d_om_a))
    _check(c["name"], "ordered dx (logits)", _nchw64(dx), wx)
    _check(c["name"], "ordered d_offset | d_logit", _nchw64(d_om[..., :27 * dg]), wom)
    _check(c["name"], "ordered dx vs atomic dx (logits)", _nchw64(dx), _nchw64(dx_a), bar=4e-5)


@pytest.mark.parametrize("kind,spec", [("drawn", D.TILE_CASES[0]), ("new", "dg4_s2")], ids=["tile_162px", "dg4_s2"])
def test_an_image_has_the_bits_it_gets_alone(kind, spec):
    """Image 1 of a batch of 3: its lists live in its own region of the index, its keys count output pixels inside the image."""
    c, _ = _case(kind, spec)
    assert c["x"].shape[0] == 3
    g = O.grad_columns(c)
    m = O.direct_mask(c)
    x, off, mh, dcol = _nhwc(c["x"]), _nhwc(c["offset"]), _nhwc(m), _dcol(g)
    rc, dx, d_off, _ = _ordered_raw(dcol, x, off, mh, c["stride"], c["dg"])
    one = lambda t: None if t is None else t[1:2].contiguous()
    rc1, dx1, d_off1, _ = _ordered_raw(one(dcol), one(x), one(off), one(mh), c["stride"], c["dg"])
    assert rc == 0 and rc1 == 0
    assert np.array_equal(_bits(dx[1:2]), _bits(dx1)) and np.array_equal(_bits(d_off[1:2]), _bits(d_off1))
    assert dx1.abs().max().item() > 0


def test_workspace_size_and_refusal():
    import vatl_hip as vh
    for n, h, w, s, dg in ((1, 1, 1, 1, 1), (2, 7, 5, 1, 1), (3, 10, 8, 2, 4), (3, 9, 6, 1, 2), (120, 64, 48, 2, 1), (32, 96, 72, 1, 4)):
        assert vh.lib().vatl_deform_dx_index_bytes(n, h, w, s, dg) == _index_bytes(n, h, w, s, dg) == vh.deform_dx_index_bytes(n, h, w, s, dg)
    for bad in ((0, 7, 5, 1, 1), (1, 7, 5, 3, 1), (1, 7, 5, 1, 3), (1, 1 << 15, 1 << 15, 1, 1)):
        assert vh.lib().vatl_deform_dx_index_bytes(*bad) == -1
        with pytest.raises(vh.VatlError):
            vh.deform_dx_index_bytes(*bad)
    c = O.new_case("pileup_frac")
    g = O.grad_columns(c)
    x, off, dcol = _nhwc(c["x"]), _nhwc(c["offset"]), _dcol(g)
    need = _index_bytes(2, 7, 5, 1, 1)
    rc, dx, d_off, _ = _ordered_raw(dcol, x, off, None, 1, 1, ws_bytes=need - 1)
    assert rc == -1 and b"workspace" in vh.lib().vatl_last_error()                       # VATL_EINVAL
    assert torch.isnan(dx).all() and (d_off == -77.0).all()                              # nothing was launched
    rc, dx, d_off, _ = _ordered_raw(dcol, x, off, None, 1, 1, ws_bytes=need)
    assert rc == 0 and not torch.isnan(dx).any() and not (d_off == -77.0).any()
    # the refusals of the atomic entry are the ordered entry's too
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    args = (vh._ptr(dcol), dcol.shape[3], vh._ptr(x), vh._ptr(off), 18, None, 0, 0, vh._ptr(dx), vh._ptr(d_off), 18, None, 0, 2, 7, 5, 16)
    assert vh.lib().vatl_deform_columns_bwd_ordered(*args, 3, 1, ws.data_ptr(), need, vh._stream()) == -1 and b"stride 3" in vh.lib().vatl_last_error()
    assert vh.lib().vatl_deform_columns_bwd_ordered(*args, 1, 3, ws.data_ptr(), need, vh._stream()) == -1 and b"deformable groups" in vh.lib().vatl_last_error()
    assert vh.lib().vatl_deform_columns_bwd_ordered(*args, 1, 1, None, need, vh._stream()) == -1 and b"workspace" in vh.lib().vatl_last_error()


# ---- the switch through the modules --------------------------------------------------------------------------------------------------

@pytest.fixture
def clean_switch():
    from alphapose.models.layers import dcn
    before = (dcn.vh.deform_deterministic_mode(), torch.are_deterministic_algorithms_enabled(), torch.backends.cudnn.deterministic)
    dcn.set_deterministic(None)
    torch.use_deterministic_algorithms(False)
    torch.backends.cudnn.deterministic = False
    yield dcn
    dcn.set_deterministic(before[0])
    torch.use_deterministic_algorithms(before[1])
    torch.backends.cudnn.deterministic = before[2]


@pytest.mark.parametrize("spec", [D.PRODUCT_CASES[0], D.TILE_CASES[2]], ids=lambda c: c[0])
def test_module_gradients_under_the_context_manager(spec, clean_switch, monkeypatch):
    import vatl_hip as vh
    dcn = clean_switch
    c = D.smooth_offsets(D.make_case(*spec), 900 + D.ALL_CASES.index(spec))
    s, dg = c["stride"], c["dg"]
    m = torch.sigmoid(c["mask_logits"]).float().double()
    seen = []
    real = vh.deform_columns_bwd

    def spy(*a, **kw):
        seen.append(kw.get("deterministic"))
        return real(*a, **kw)
    monkeypatch.setattr(vh, "deform_columns_bwd", spy)
    for masked in (True, False):
        leaves = [c["x"].clone().requires_grad_(), c["offset"].clone().requires_grad_(), c["w"].clone().requires_grad_()]
        if masked:
            leaves.append(m.clone().requires_grad_())
        ref = D.deform_conv_ref(leaves[0], leaves[2], leaves[1], leaves[3] if masked else None, s, dg)
        gy = torch.randn(ref.shape, generator=torch.Generator().manual_seed(5)).double()
        want = torch.autograd.grad(ref, leaves, gy)

        def run():
            d = [t.detach().float().to(dev()).requires_grad_() for t in leaves]
            if masked:
                y = dcn.modulated_deform_conv(d[0], d[1], d[3], d[2], None, s, 1, 1, 1, dg)
            else:
                y = dcn.deform_conv(d[0], d[1], d[2], s, 1, 1, 1, dg)
            return torch.autograd.grad(y, d, gy.float().to(dev()))
        del seen[:]
        with dcn.deterministic():
            first, second = run(), run()
        assert seen == [True, True]
        run()
        assert seen == [True, True, False]
        for name, a, b, w64 in zip(("dx", "d_offset", "dw", "d_mask"), first, second, want):
            assert torch.equal(a, b), name
            _check(c["name"], f"{name} under deterministic(), masked={masked}", a.double().cpu(), w64)


# ---- the trainer: one SE bottleneck of the layer2.0 shape ---------------------------------------------------------------------------------

@pytest.mark.parametrize("modulated,dg", [(False, 1), (True, 2)], ids=["v1_dg1", "v2_dg2"])
def test_se_bottleneck_trainer_is_bit_reproducible_with_the_switch_on(modulated, dg, clean_switch):
    from alphapose.models import hip_train
    from tests.test_gpu_dcn import _se_block
    dcn = clean_switch
    xh = _nhwc(torch.randn(2, 256, 16, 12, generator=torch.Generator().manual_seed(12)))
    dyh = _nhwc(torch.randn(2, 512, 8, 6, generator=torch.Generator().manual_seed(13)))

    def run():
        blk = _se_block(modulated, dg, 11).to(dev()).train()
        unit = hip_train._SEBottleneckT(blk)
        grads = hip_train._Grads()
        with torch.no_grad():
            unit.forward(xh)
            dx = unit.backward(dyh, grads)
        hip_train._side.join()
        hip_train._flush_batch_counters()
        torch.cuda.synchronize()
        by_param = {p: k for k, p in blk.named_parameters()}
        out = {by_param[p]: g.detach().clone() for p, g in grads.items()}
        assert len(out) == 18
        out["dx"] = dx.clone()
        return out
    dcn.set_deterministic(True)
    a, b = run(), run()
    dcn.set_deterministic(False)
    off = run()
    tag = f"se_block_mod{int(modulated)}_dg{dg}"
    for k in a:
        assert torch.equal(a[k], b[k]), k
        _check(tag, f"{k}: switch on vs off", a[k].double().cpu(), off[k].double().cpu())
    assert set(a) == set(off)


# ---- whole FastPose-50-DCN, as the driver's --seedfix leaves torch --------------------------------------------------------------------

def test_fastpose_dcn_finetune_steps_are_bit_reproducible_under_cudnn_deterministic(clean_switch):
    import vatl_hip as vh
    from active_learning.optim import AdamW
    from alphapose.models import hip_train
    from tests.test_gpu_dcn import _fastpose
    dcn = clean_switch
    torch.backends.cudnn.deterministic = True                                            # nothing else: the switch stays None
    assert dcn.vh.deform_deterministic_mode() is None and dcn.is_deterministic()
    gen = torch.Generator().manual_seed(21)
    x = (torch.rand((2, 3, 256, 192), generator=gen) - 0.45).to(dev())
    labels = (torch.rand((2, 17, 64, 48), generator=gen) * 0.1).to(dev())
    masks = (torch.rand((2, 17, 1, 1), generator=gen) > 0.2).float().to(dev())
    finals = []
    for _ in range(2):
        torch.manual_seed(166)
        m = _fastpose({"MODULATED": True, "DEFORM_GROUP": 1, "FALLBACK_ON_STRIDE": False}).to(dev()).train()
        opt = AdamW(params=[{"params": m.parameters(), "lr": 2.5e-4}], weight_decay=0.7)
        tr, arena = hip_train.trainer_for(m), hip_train.arena_for(m)
        losses = []
        for _ in range(2):
            with torch.no_grad():
                out = tr.forward(x)
                loss, dout = vh.masked_mse_fwd_bwd(out, labels, masks)
                arena.begin()
                tr.backward(dout, arena=arena, overlap=True)
                arena.finish()
                arena.attach()
            opt.step()
            losses.append(float(loss))
        torch.cuda.synchronize()
        finals.append((losses, {k: v.detach().clone() for k, v in m.state_dict().items()}))
        del m, opt, tr, arena
    (la, sa), (lb, sb) = finals
    assert la == lb and np.isfinite(la).all()
    moved = [k for k in sa if "conv2_offset" in k]
    assert len(moved) == 26
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
