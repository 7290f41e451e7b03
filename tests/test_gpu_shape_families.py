"""The three inference kernels with a host shape rule (csrc/winograd_s2_43.hip, csrc/winograd_deconv43.hip, csrc/stem_pool_w1d.hip — and csrc/stem_pool.hip, whose
band cut the last one shares) away from the corner their own test files pin: tile grids that are no powers of two, a tile row of one tile, the remainder group of
the tile order, every epilogue the wrappers accept, stem heights whose band cut is uneven or leaves a band empty, and the S2_43 / STEM_W1D route switches in
HRNet-W32 and FastPose-R50.  Layers, references and filters are those of tests/test_gpu_conv_s2_43.py, tests/test_gpu_deconv43.py and tests/test_gpu_stem_w1d.py;
the bar is their TOL.  Measured errors next to the old cases': profiles/shape_family_notes.md."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import test_gpu_conv_s2_43 as s2t
from tests import test_gpu_deconv43 as d43t
from tests import test_gpu_stem_w1d as w1t
from tests.gpu_util import dev, record, rel_err, to_dev
from tests.test_gpu_stem_w1d import stem, vh  # noqa: F401  (fixtures: the seed-41 stem filter in both packings; the library)

pytestmark = pytest.mark.gpu

TOL = s2t.TOL       # 2e-5, max|err| / max|ref| per layer: the bar of the three files
assert TOL == d43t.TOL == w1t.TOL == 2e-5


def _id(c):
    return "x".join(map(str, c))


def _nchw(y):
    return np.transpose(y.cpu().numpy(), (0, 3, 1, 2))


# ---- 1. grids that are no powers of two, row ends, remainders of the tile order ------------------------------------------------------------------------
# Tiles per image column x row (TH x TW) are H / 8 x W / 6 for s2_43 and H / 4 x W / 3 for deconv43; a block takes 32 tiles x 64 output channels.  The tile order
# walks groups of rn filter slices: rn = max(2, 2048 / (18 Cin)) of Cout / 64 filter tiles for s2_43, rn = max(2, 2048 / (5 Cin)) of 4 Cout / 64 (phase, filter tile)
# slices for deconv43, each capped by the slice count; a slice count that is no multiple of rn ends in a shorter group (`last_grp`, divided by `d_rn_last`).

S2_CASES = [
    # n, H, W, Cin, Cout
    (1, 24, 18, 16, 64),      # 3x3 tiles (the 24x18 grid of the 384x288 nets): fdiv by TW = 3 and tpi = 9; rn = min(1 slice, 7) = 1, no remainder
    (3, 40, 30, 32, 256),     # 5x5 tiles, 75 tiles = 3 m-tiles with a tail of 11; rn = 2048 / 576 = 3 over 4 filter tiles -> last group of 1 (d_rn_last = 1); 12 blocks = 8 + 4 over the XCDs
    (2, 48, 36, 48, 64),      # 6x6 tiles, 72 tiles; Cin / 16 = 3 stages per phase (odd: the stage buffer parity flips at every phase change); rn = 1
    (1, 96, 72, 16, 64),      # 12x12 tiles = 144 = 4.5 blocks: images rows of 12 tiles straddle the 32-tile blocks at 8 / 4 / 0
    (7, 8, 42, 16, 512),      # TH = 1, TW = 7: every tile has the top and bottom border; rn = 2048 / 288 = 7 over 8 filter tiles -> last group of 1
    (5, 56, 6, 16, 64),       # TW = 1: every tile is the first AND the last of its row (set_goff's `tx == 0` rule at every entry), TH = 7
]

D43_CASES = [
    (1, 12, 9, 16, 64),       # 3x3 tiles; 4 slices, rn = min(4, 2048 / 80 = 25) = 4, no remainder
    (3, 20, 15, 128, 64),     # 5x5 tiles, 75 tiles with a tail; rn = 2048 / 640 = 3 over 4 slices -> last group of 1
    (2, 24, 18, 80, 128),     # 6x6 tiles; rn = 2048 / 400 = 5 over 8 slices -> last group of 3 (d_rn_last = 3); Cin / 16 = 5 stages
    (1, 48, 36, 16, 64),      # 12x12 tiles = 4.5 blocks
    (7, 4, 21, 16, 64),       # TH = 1, TW = 7
    (5, 28, 3, 16, 64),       # TW = 1: every tile at both row ends, TH = 7
]


def _s2_run(vh, xd, wd, scale, bias, cout, relu=True, out=None):
    us2 = vh.pack_winograd_s2_43_weight(wd)
    wp = None if xd.shape[-1] % 32 else vh.pack_conv_weight(wd)      # the wrapper touches w_packed only on the implicit-GEMM route
    return vh.conv2d_fwd(xd, wp, scale, bias, cout, 3, 3, 2, 1, relu, out=out, u_s2=us2)


def _d43_run(vh, xd, wd, scale, bias, cout, relu=True, out=None):
    return vh.deconv4x4s2_winograd_fwd(xd, vh.pack_winograd_deconv_weight(wd), scale, bias, cout, relu, out=out, u43=vh.pack_winograd_deconv43_weight(wd))


@pytest.mark.parametrize("case", S2_CASES, ids=_id)
def test_s2_43_odd_grids_match_float64_and_the_implicit_gemm(vh, case):
    n, h, w, cin, cout = case
    xd, wd, scale, bias, ref = s2t._layer(vh, *case)
    assert vh.conv3x3s2_winograd43_supported(n, h, w, cin, cout)
    with vh.flop_meter() as fm:
        y = _s2_run(vh, xd, wd, scale, bias, cout)
    assert fm.routes["winograd_s2_43"] == 1 and fm.routes["igemm"] == 0 and sum(fm.routes.values()) == 1, fm.routes
    tiles32 = (n * (h // 8) * (w // 6) + 31) // 32 * 32
    assert fm.direct == 2.0 * tiles32 * 72 * cin * cout and fm.direct_launches == 1 and fm.winograd_launches == 0 and fm.winograd == 0
    assert y.shape == (n, h // 2, w // 2, cout)
    e = rel_err(_nchw(y), ref)
    ed = eg = None
    if cin % 32 == 0:                                           # the implicit GEMM needs whole 32-channel k-tiles
        with vh.flop_meter() as fo:
            yd = vh.conv2d_fwd(xd, vh.pack_conv_weight(wd), scale, bias, cout, 3, 3, 2, 1, True)
        assert fo.routes["winograd_s2_43"] == 0 and fo.routes["igemm"] == 1, fo.routes
        ed, eg = rel_err(y.cpu().numpy(), yd.cpu().numpy()), rel_err(_nchw(yd), ref)
    print(f"family s2_43 {case}: vs float64 {e:.3e}  vs implicit GEMM {ed}  implicit GEMM vs float64 {eg}")
    record("family_s2_43_" + _id(case), s2_43_vs_fp64=e, vs_igemm=ed, igemm_vs_fp64=eg)
    assert e < TOL, (case, e)
    assert ed is None or ed < TOL, (case, ed)
    if n > 1:                                                   # other tile numbers, another block, another tail: the same bits
        alone = _s2_run(vh, xd[n - 1:].contiguous(), wd, scale, bias, cout)
        assert torch.equal(alone[0], y[n - 1])


@pytest.mark.parametrize("case", D43_CASES, ids=_id)
def test_deconv43_odd_grids_match_float64_the_f33_route_and_the_implicit_gemm(vh, case):
    n, h, w, cin, cout = case
    xd, wd, scale, bias, ref = d43t._layer(vh, *case)
    assert vh.deconv4x4s2_winograd43_supported(n, h, w, cin, cout)
    with vh.flop_meter() as fm:
        y = _d43_run(vh, xd, wd, scale, bias, cout)
    assert fm.routes["winograd_deconv43"] == 1 and sum(fm.routes.values()) == 1 and fm.winograd_launches == 1 and fm.direct_launches == 0, fm.routes
    tiles32 = (n * (h // 4) * (w // 3) + 31) // 32 * 32
    assert fm.winograd == 2.0 * tiles32 * 20 * cin * cout * 4 and fm.direct == 0
    assert y.shape == (n, 2 * h, 2 * w, cout)
    with vh.flop_meter() as fo:
        y33 = vh.deconv4x4s2_winograd_fwd(xd, vh.pack_winograd_deconv_weight(wd), scale, bias, cout, True)
    assert fo.routes["winograd_deconv43"] == 0 and fo.winograd_launches == 1, fo.routes
    e43, e33, e4333 = rel_err(_nchw(y), ref), rel_err(_nchw(y33), ref), rel_err(y.cpu().numpy(), y33.cpu().numpy())
    ed = eg = None
    if cin % 32 == 0:                                           # the implicit GEMM needs whole 32-channel k-tiles
        yd = vh.deconv4x4s2_fwd(xd, vh.pack_deconv_weight(wd), scale, bias, cout, True)
        ed, eg = rel_err(y.cpu().numpy(), yd.cpu().numpy()), rel_err(_nchw(yd), ref)
    print(f"family deconv43 {case}: F(4x3,2x2) {e43:.3e}  F(3x3,2x2) {e33:.3e}  between them {e4333:.3e}  vs implicit GEMM {ed}  implicit GEMM vs float64 {eg}")
    record("family_deconv43_" + _id(case), f43_vs_fp64=e43, f33_vs_fp64=e33, f43_vs_f33=e4333, vs_igemm=ed, igemm_vs_fp64=eg)
    assert e43 < TOL and e33 < TOL and e4333 < TOL, (case, e43, e33, e4333)
    assert ed is None or ed < TOL, (case, ed)
    if n > 1:
        alone = _d43_run(vh, xd[n - 1:].contiguous(), wd, scale, bias, cout)
        assert torch.equal(alone[0], y[n - 1])


def _poisoned_neighbours(run, xd, out_shape):
    """tests/test_gpu_conv_s2_43.py::test_out_of_image_pieces_are_zeros_not_neighbours on another shape: a piece outside the image that is read from a
    neighbouring row or image instead of the zero entry may hide behind a zero filter position while the neighbour is finite; behind NaN it cannot."""
    n = xd.shape[0]
    full = run(xd)
    assert torch.isfinite(full).all()
    shifted = run(xd[1:].contiguous())
    assert torch.equal(shifted, full[1:])
    xn = xd.clone()
    xn[0::2] = float("nan")                                     # every even image poisoned: the odd ones keep their bits ...
    poisoned = run(xn)
    for i in range(1, n, 2):
        assert torch.equal(poisoned[i], full[i]), i
    xn = xd.clone()
    xn[1::2] = float("nan")                                     # ... and the other way round
    poisoned = run(xn)
    for i in range(0, n, 2):
        assert torch.equal(poisoned[i], full[i]), i
    out = torch.full(out_shape, -7.0, device=dev())
    y = run(xd, out=out)
    assert y.data_ptr() == out.data_ptr() and torch.equal(out, full)


@pytest.mark.parametrize("case", [(5, 56, 6, 16, 64), (3, 40, 30, 32, 256)], ids=_id)     # TW = 1; 5x5 tiles
def test_s2_43_out_of_image_pieces_are_zeros_at_a_one_tile_row_and_an_odd_grid(vh, case):
    n, h, w, cin, cout = case
    xd, wd, scale, bias, _ = s2t._layer(vh, *case)
    _poisoned_neighbours(lambda x, out=None: _s2_run(vh, x, wd, scale, bias, cout, out=out), xd, (n, h // 2, w // 2, cout))


@pytest.mark.parametrize("case", [(5, 28, 3, 16, 64), (3, 20, 15, 128, 64)], ids=_id)     # TW = 1; 5x5 tiles
def test_deconv43_out_of_image_pieces_are_zeros_at_a_one_tile_row_and_an_odd_grid(vh, case):
    n, h, w, cin, cout = case
    xd, wd, scale, bias, _ = d43t._layer(vh, *case)
    _poisoned_neighbours(lambda x, out=None: _d43_run(vh, x, wd, scale, bias, cout, out=out), xd, (n, 2 * h, 2 * w, cout))


# ---- 2. every epilogue of the two F(4x3,2x2) kernels ---------------------------------------------------------------------------------------------------
# The wrappers pass scale and bias through one by one (a null pointer each), so the one-sided settings are calls a user can make and are covered as well.

EPILOGUES = [
    # name, scale, bias, relu
    ("scale_bias_relu", True, True, True),
    ("scale_bias", True, True, False),
    ("scale_bias_c", True, "c", False),       # bias[c] = c: a bias read from another channel is off by at least 1
    ("none", False, False, False),
    ("none_relu", False, False, True),
    ("scale_only", True, False, False),
    ("bias_only_relu", False, True, True),
]
KERNELS = {
    # the layer of the kernel's own test file, the route, the float64 operation, one small and one odd-grid shape of item 1 (the second: several filter tiles)
    "s2_43": (s2t._layer, _s2_run, lambda x, w: F.conv2d(x, w, None, 2, 1), [(1, 24, 18, 16, 64), (3, 40, 30, 32, 256)]),
    "deconv43": (d43t._layer, _d43_run, lambda x, w: F.conv_transpose2d(x, w, None, 2, 1), [(1, 12, 9, 16, 64), (2, 24, 18, 80, 128)]),
}
EPI_CASES = [(k, c) for k in KERNELS for c in KERNELS[k][3]]

_raw = {}


def _raw64(vh, kernel, case):
    """The layer's inputs on the device, its folded scale and bias, and the float64 convolution without any epilogue (computed once per shape)."""
    if (kernel, case) not in _raw:
        layer, _, op, _ = KERNELS[kernel]
        xd, wd, scale, bias, _ = layer(vh, *case)
        z = op(xd.permute(0, 3, 1, 2).cpu().double(), wd.cpu().double())
        _raw[kernel, case] = (xd, wd, scale, bias, z)
    return _raw[kernel, case]


@pytest.mark.parametrize("kernel,case", EPI_CASES, ids=[k + "_" + _id(c) for k, c in EPI_CASES])
def test_every_epilogue_matches_float64(vh, kernel, case):
    cout = case[4]
    xd, wd, scale, bias, z = _raw64(vh, kernel, case)
    run = KERNELS[kernel][1]
    for name, use_scale, use_bias, relu in EPILOGUES:
        sc = scale if use_scale else None
        bi = torch.arange(cout, dtype=torch.float32, device=dev()) if use_bias == "c" else (bias if use_bias else None)
        ref = z
        if sc is not None:
            ref = ref * sc.cpu().double().view(1, -1, 1, 1)     # the folded fp32 values as they are: the reference is the epilogue the kernel is asked for
        if bi is not None:
            ref = ref + bi.cpu().double().view(1, -1, 1, 1)
        if relu:
            ref = ref.clamp_min(0)
        y = run(vh, xd, wd, sc, bi, cout, relu=relu)
        e = rel_err(_nchw(y), ref.numpy())
        print(f"family epilogue {kernel} {case} {name}: vs float64 {e:.3e}")
        record(f"family_epilogue_{kernel}_{_id(case)}_{name}", rel=e)
        assert e < TOL, (kernel, case, name, e)
        if not relu:
            assert (y < 0).any(), "without ReLU the negative half of the outputs is part of the comparison"


@pytest.mark.parametrize("kernel,case", EPI_CASES, ids=[k + "_" + _id(c) for k, c in EPI_CASES])
def test_power_of_two_scales_commute_with_the_kernel_bit_for_bit(vh, kernel, case):
    """ReLU off, no bias, scale[c] = 2^k(c) with k spread over -10 .. 10 in a scrambled channel order (k differs between c and c + 4, c + 32, c + 64: channel
    quads, filter halves, filter tiles): fp32 rounding commutes with a power of two and the outputs (|y| ~ 1) are far from under- and overflow, so the output
    is bit-equal to the unit-scale output times that vector.  A scale from the wrong channel fails exactly, however small the channel."""
    cout = case[4]
    xd, wd, _, _, _ = _raw64(vh, kernel, case)
    run = KERNELS[kernel][1]
    k = (torch.arange(cout) * 37 + 11) % 21 - 10
    assert k.min() == -10 and k.max() == 10 and all((k[:-s] != k[s:]).all() for s in (4, 32, 64) if s < cout)
    pow2 = torch.pow(2.0, k.float()).to(dev())
    unit = run(vh, xd, wd, torch.ones(cout, device=dev()), None, cout, relu=False)
    assert torch.equal(unit, run(vh, xd, wd, None, None, cout, relu=False))             # a null scale is a scale of one
    scaled = run(vh, xd, wd, pow2, None, cout, relu=False)
    assert float(unit.abs().max()) < 2.0 ** 10 and float(unit[unit != 0].abs().min()) > 2.0 ** -100
    same = scaled == unit * pow2
    record(f"family_pow2_{kernel}_{_id(case)}", equal=float(same.float().mean()))
    assert same.all(), (kernel, case, torch.nonzero(~same)[:4].tolist())
    assert torch.equal(run(vh, xd, wd, pow2, torch.zeros(cout, device=dev()), cout, relu=False), scaled)      # a zero bias is no bias


# ---- 3. stem bands -------------------------------------------------------------------------------------------------------------------------------------
# Both stem files cut an image into `bands` (doubled while N * bands < 512 and 2 * bands <= PH / 4) of ceil(PH / bands) pooled rows, PH = H / 4.

STEM_SHAPES = [
    # n, H, W
    (3, 4, 64),         # PH = 1: one band, one step with the top and the bottom border in it
    (1, 12, 64),        # PH = 3: one band of an odd number of steps
    (1, 36, 192),       # PH = 9: 2 bands of 5 and 4
    (2, 100, 128),      # PH = 25: 4 bands of 7, 7, 7 and 4
    (1, 132, 192),      # PH = 33: 8 bands of 5 — band 6 has 3 rows, band 7 starts at row 35 and leaves through `if (i_first >= i_end) return;`
    (70, 132, 64),      # the same cut on many images (70 * 4 < 512, so still 8 bands with the empty one; the blocks of an image are (image, band), 560 of them)
    (130, 132, 64),     # 130 * 4 >= 512: 4 bands of 9, 9, 9 and 6, none empty — the batch and the image alone (8 bands) are cut differently
]


def _bands(n, h):
    """(bands, bands that hold at least one pooled row) from the host rule."""
    ph, bands = h // 4, 1
    while n * bands < 512 and bands * 2 <= ph // 4:
        bands *= 2
    per = (ph + bands - 1) // bands
    return bands, (ph + per - 1) // per


def test_the_band_cuts_the_cases_are_there_for():
    assert [_bands(n, h) for n, h, _ in STEM_SHAPES] == [(1, 1), (1, 1), (2, 2), (4, 4), (8, 7), (8, 7), (4, 4)]
    assert _bands(1, 132) != _bands(130, 132)
    assert all(_bands(n, h)[0] == _bands(n, h)[1] for n, h, _ in w1t.SHAPES)            # no old shape has an empty band: their meter assertions stand


@pytest.fixture(scope="module")
def stem3(vh):
    """HRNet's conv1: a seeded 3x3 filter with the folded BatchNorm of the `stem` fixture."""
    w = torch.randn((64, 3, 3, 3), generator=torch.Generator(device="cpu").manual_seed(43)) * (2.0 / 27) ** 0.5
    return {"w": w, "pw": vh.pack_stem3_weight(w.to(dev()))}


def _stem_x(shape):
    n, h, wdt = shape
    return torch.rand((n, 3, h, wdt), generator=torch.Generator(device="cpu").manual_seed(n * 1000 + h + wdt)) - 0.45


def _picked(n):
    return sorted(set(range(min(n, 3))) | {n - 1})              # the images compared with float64: the first three and the last


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=_id)
def test_pooling_stems_on_uneven_and_empty_bands(vh, stem, shape):
    n, h, wdt = shape
    assert vh.stem_pool_w1d_supported(h, wdt) and vh.stem_pool_supported(h, wdt)
    x = _stem_x(shape)
    xd = x.to(dev())
    ph, (bands, nonempty) = h // 4, _bands(n, h)
    steps = n * (ph + nonempty - 1)                             # the steps that run: a band below the first recomputes one, an empty band none
    with vh.flop_meter() as fm:
        new = w1t._new(vh, stem, xd)
    assert fm.routes["stem_pool_w1d"] == 1 and sum(fm.routes.values()) == 1, fm.routes
    assert fm.direct == 2.0 * steps * 2 * (wdt // 4) * 9 * 24 * 64 and fm.direct_launches == 1 and fm.winograd_launches == 0, (fm.direct, steps)
    with vh.flop_meter() as fo:
        old = w1t._old(vh, stem, xd)
    assert fo.routes["stem_pool"] == 1 and sum(fo.routes.values()) == 1, fo.routes
    assert fo.direct == 2.0 * steps * 2 * (wdt // 2) * 64 * 168 and fo.direct_launches == 1, (fo.direct, steps)
    assert new.shape == old.shape == (n, ph, wdt // 4, 64)
    pick = _picked(n)
    ref = w1t._ref64(stem, x[pick])
    en, eo, eno = rel_err(new[pick].cpu().numpy(), ref), rel_err(old[pick].cpu().numpy(), ref), rel_err(new.cpu().numpy(), old.cpu().numpy())
    print(f"family stem {shape} ({bands} bands, {nonempty} with rows): 1-D Winograd {en:.3e}  direct {eo:.3e}  between them {eno:.3e}")
    record("family_stem_" + _id(shape), w1d_vs_fp64=en, direct_vs_fp64=eo, w1d_vs_direct=eno)
    assert en < TOL and eo < TOL and eno < TOL, (shape, en, eo, eno)
    assert not torch.equal(new, old)                            # the keyword did select the other kernel
    last = xd[n - 1:].clone()
    for fn, full in ((w1t._new, new), (w1t._old, old)):
        assert torch.equal(fn(vh, stem, last)[0], full[n - 1])  # alone (at 130 images: another cut), the same bits
    for u1d, full in ((stem["u1d"], new), (None, old)):
        out = torch.full((n, ph, wdt // 4, 64), -7.0, device=dev())
        y = vh.stem_pool_fwd(xd, stem["pw"], stem["scd"], stem["bid"], out=out, u1d=u1d)
        assert y.data_ptr() == out.data_ptr() and torch.equal(out, full) and not (out == -7.0).any()     # a short or empty band leaves no row unwritten


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=_id)
def test_hrnet_stem_on_uneven_and_empty_bands(vh, stem, stem3, shape):
    n, h, wdt = shape
    x = _stem_x(shape)
    xd = x.to(dev())
    with vh.flop_meter() as fm:
        got = vh.stem3_fwd(xd, stem3["pw"], stem["scd"], stem["bid"])
    assert fm.routes["stem_pool"] == 1 and sum(fm.routes.values()) == 1, fm.routes
    assert fm.direct == 2.0 * n * (h // 4) * 2 * (wdt // 2) * 64 * 36 and fm.direct_launches == 1      # no pooling, so no band recomputes a step
    assert got.shape == (n, h // 2, wdt // 2, 64)
    pick = _picked(n)
    ref = (F.conv2d(x[pick].double(), stem3["w"].double(), None, 2, 1) * stem["sc"].double().view(1, -1, 1, 1) + stem["bi"].double().view(1, -1, 1, 1)).clamp_min(0)
    e = rel_err(got[pick].cpu().numpy(), ref.permute(0, 2, 3, 1).numpy())
    print(f"family stem3 {shape}: vs float64 {e:.3e}")
    record("family_stem3_" + _id(shape), rel=e)
    assert e < TOL, (shape, e)
    assert torch.equal(vh.stem3_fwd(xd[n - 1:].clone(), stem3["pw"], stem["scd"], stem["bid"])[0], got[n - 1])
    out = torch.full((n, h // 2, wdt // 2, 64), -7.0, device=dev())
    y = vh.stem3_fwd(xd, stem3["pw"], stem["scd"], stem["bid"], out=out)
    assert y.data_ptr() == out.data_ptr() and torch.equal(out, got) and not (out == -7.0).any()


# ---- 4. the route switches in the other two networks ---------------------------------------------------------------------------------------------------

def _forward(vh, hip_engine, m, x, monkeypatch, **switches):
    """One stream-route pass with the given hip_engine switches on a fresh plan: heat-maps, the meter, and every stride-2 3x3 _Conv call as
    (input shape, Cout, called without residual and with NHWC output)."""
    for k, v in switches.items():
        monkeypatch.setattr(hip_engine, k, v)
    calls = []
    inner = hip_engine._Conv.__call__

    def spy(self, x, relu, residual=None, out_nchw=False, out=None):
        if (self.r, self.s, self.stride, self.pad) == (3, 3, 2, 1):
            calls.append((tuple(x.shape), self.cout, residual is None and not out_nchw))
        return inner(self, x, relu, residual=residual, out_nchw=out_nchw, out=out)

    monkeypatch.setattr(hip_engine._Conv, "__call__", spy)
    hm = torch.empty((x.shape[0], 17, 64, 48), device=dev())
    m.__dict__.pop("_vatl_plan", None)
    try:
        with torch.no_grad(), vh.flop_meter() as fm:
            hip_engine.forward_into(m, x, hm)
    finally:
        m.__dict__.pop("_vatl_plan", None)
        monkeypatch.setattr(hip_engine._Conv, "__call__", inner)
    return hm, fm, calls


def _same_heatmaps(name, on, off):
    """On and off within 2e-5 (the bar of the SimplePose plan tests); a plane's arg-max may move only between two values that differ by less than that bar times
    the plane's maximum, in both passes (the s2_43 change itself moved two such planes of 17 408 on the benchmark step)."""
    e = rel_err(on.cpu().numpy(), off.cpu().numpy())
    a, b = on.flatten(2).cpu().double(), off.flatten(2).cpu().double()
    ia, ib = a.argmax(-1, keepdim=True), b.argmax(-1, keepdim=True)
    moved = int((ia != ib).sum())
    gap = 0.0
    for p in (a, b):
        gap = max(gap, float(((p.gather(-1, ia) - p.gather(-1, ib)).abs() / p.abs().amax(-1, keepdim=True))[ia != ib].max()) if moved else 0.0)
    print(f"family {name}: heat-maps on vs off {e:.3e}, {moved} arg-max planes moved (largest gap between the two candidates {gap:.3e} of the plane's maximum)")
    record("family_" + name, rel=e, argmax_moved=moved, argmax_gap=gap)
    assert e < 2e-5 and gap < 2e-5, (name, e, moved, gap)


def _routes_differ_only_in(fm, fo, moved):
    """`moved`: {route with the switch on: (route with it off, launches)}; every other counter is the same."""
    names = set(moved) | {v[0] for v in moved.values()}
    assert all(fo.routes[k] == fm.routes[k] for k in fo.routes if k not in names), (fm.routes, fo.routes)
    assert sum(fo.routes.values()) == sum(fm.routes.values())
    for k, (other, count) in moved.items():
        assert fm.routes[k] == count and fo.routes[k] == 0 and fo.routes[other] - fm.routes[other] == count, (k, fm.routes, fo.routes)


def test_hrnet_plan_routes_its_stride2_convs(vh, monkeypatch):
    """HRNet-W32 on 2 crops: the stem's conv2, the transitions and the fuse layers' down-sampling steps that run without a residual take the s2_43 kernel where the
    rule admits their grid (a chain's last step adds the branch it lands on and stays on the implicit GEMM); with S2_43 off the same launches are implicit GEMMs."""
    from alphapose.models import hip_engine
    from oracle import synth
    from tests.test_gpu_conv import HRNET_CFG, _build
    m = _build(HRNET_CFG)
    x = to_dev(synth.crops(2))
    on, fm, calls = _forward(vh, hip_engine, m, x, monkeypatch, S2_43=True)
    off, fo, calls_off = _forward(vh, hip_engine, m, x, monkeypatch, S2_43=False)
    assert calls == calls_off and len(calls) > 0
    routed = sum(free and vh.conv3x3s2_winograd43_supported(*shape, cout) for shape, cout, free in calls)
    print(f"family hrnet: {len(calls)} stride-2 3x3 calls, {sum(free for _, _, free in calls)} without residual, {routed} routed; shapes {sorted(set(c for c in calls if c[2]))}")
    assert 0 < routed < len(calls)
    _routes_differ_only_in(fm, fo, {"winograd_s2_43": ("igemm", routed)})
    _same_heatmaps("hrnet_w32_s2_43_on_off", on, off)


def test_fastpose_plan_routes_its_stride2_convs_and_the_stem(vh, monkeypatch):
    """FastPose-R50 on 2 crops: layer2 / 3 / 4.0.conv2 take the s2_43 kernel and the stem the 1-D Winograd kernel; each switch alone moves exactly its launches."""
    from alphapose.models import hip_engine
    from oracle import synth
    from tests.test_gpu_conv import _build
    m = _build({"TYPE": "FastPose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50})
    x = to_dev(synth.crops(2))
    assert vh.stem_pool_w1d_supported(256, 192)
    on, fm, calls = _forward(vh, hip_engine, m, x, monkeypatch, S2_43=True, STEM_W1D=True)
    routed = sum(free and vh.conv3x3s2_winograd43_supported(*shape, cout) for shape, cout, free in calls)
    assert routed == len(calls) == 3, calls
    assert fm.routes["stem_pool_w1d"] == 1 and fm.routes["stem_pool"] == 0, fm.routes
    off_s2, fo, _ = _forward(vh, hip_engine, m, x, monkeypatch, S2_43=False, STEM_W1D=True)
    _routes_differ_only_in(fm, fo, {"winograd_s2_43": ("igemm", routed)})
    _same_heatmaps("fastpose_r50_s2_43_on_off", on, off_s2)
    off_stem, fo, _ = _forward(vh, hip_engine, m, x, monkeypatch, S2_43=True, STEM_W1D=False)
    _routes_differ_only_in(fm, fo, {"stem_pool_w1d": ("stem_pool", 1)})
    assert not torch.equal(on, off_stem)
    _same_heatmaps("fastpose_r50_stem_w1d_on_off", on, off_stem)
    off_both, fo, _ = _forward(vh, hip_engine, m, x, monkeypatch, S2_43=False, STEM_W1D=False)
    _routes_differ_only_in(fm, fo, {"winograd_s2_43": ("igemm", routed), "stem_pool_w1d": ("stem_pool", 1)})
    _same_heatmaps("fastpose_r50_both_on_off", on, off_both)
