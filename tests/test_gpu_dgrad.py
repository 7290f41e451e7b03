"""fp32 data gradients (alphapose/models/hip_train.py: _ConvBN._dgrad on vatl_conv2d_fwd_ex and on the F(2x2,3x3) data-gradient filter), every
launch branch on its own at small size: the cases, the float64 reference, the host model and the impulses of tests/dgrad_cases.py (proved
in tests/test_dgrad_cpu.py).

    integer inputs   operands and residual in [-2, 2]: every partial sum is exact in fp32, so the device equals float64 autograd element for
                     element (a zero of either sign counts as zero), stream-K and Winograd included
    impulse inputs   dz one-hot: the direct routes give exactly 0 or exactly one filter element; Winograd to TOL * max|w|
    random inputs    normwise error against float64 below the bars of the neighbouring files (2e-5), two runs bit-identical, and for the direct
                     routes |got - ref| <= 2 gamma_n S element by element, n = K + 1
    branch           the route counters and the metered FLOPs are what the case's comment claims; knob settings give the same bits
    phases           one stride-2 phase alone writes its own pixels and no other; 1x1 / stride 2 leaves the odd pixels 0 or the residual's bits
    writes           the words around ``out`` keep their sentinel
    refusals         bad channel counts, a null output and an empty batch are refused before any launch

Measured figures per case: profiles/dgrad_notes.md."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import dgrad_cases as D
from tests.gpu_util import dev, record, rel_err, to_dev

pytestmark = pytest.mark.gpu

DIRECT_TOL = 2e-5     # tests/test_gpu_train.py::test_conv_dgrad_wgrad
TOL = 2e-5            # tests/test_gpu_winograd.py
IDS = [D.case_id(c) for c in D.CASES]
SENTINEL = 0x7FC12345                                            # a NaN no kernel writes: compared as bits
ids = lambda cases: [D.case_id(c) for c in cases]
S2_CASES = [c for c in D.CASES if (c.k, c.stride) == (3, 2)]
P2_CASES = [c for c in D.CASES if (c.k, c.stride) == (1, 2)]
KNOB_CASES = [c for c in D.CASES if c.knobs or c.route == D.WINO_PERSIST]
SK_CASES = [c for c in D.CASES if c.scope]
# one of each form and route: stride 1 nine taps, padded K, four phases, 1x1 / stride 2, 128x32 tile, persistent, ring, stream-K, Winograd with one and two halves and persistent
WRITE_CASES = [c for c in D.CASES if D.case_id(c) in (
    "igemm-2x5x3-64to64-k3s1p1-direct", "igemm-2x8x6-17in32to256-k1s1p0-direct", "igemm-3x6x4-96to48-k3s2p1", "igemm-2x10x6-128to64-k1s2p0",
    "igemm-3x7x7-64to32-k1s1p0", "persistent_1x1-2x13x9-256to96-k1s1p0-knob5=128", "gemm1x1_ring-1x5x3-512to128-k1s1p0-knob5=128",
    "streamk-1x32x32-1152to1024-k1s1p0-scope", "winograd-2x5x3-80to48-k3s1p1", "winograd_2h-2x13x9-48to80-k3s1p1-knob21=3",
    "winograd_persist-2767x8x8-16to16-k3s1p1")]
assert len(WRITE_CASES) == 11


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


@functools.lru_cache(maxsize=None)
def _data(case, regime):
    """dz, w, residual on the device, the float64 reference without the residual, the residual in float64, S without the residual: computed
    once, shared, left alone."""
    dz, w, res = D.inputs(case, regime)
    s = D.abs_sum(case, dz, w) if regime == "random" else None
    return to_dev(dz), to_dev(w), to_dev(res), D.reference(case, dz, w), res.astype(np.float64), s


@contextlib.contextmanager
def _setup(vh, case, knobs=None):
    """The case's product knobs (restored afterwards) and, for a stream-K case, the scope the trainers open."""
    knobs = dict(case.knobs) if knobs is None else knobs
    try:
        for k, v in knobs.items():
            vh.tune_set(k, v)
        with (vh.streamk_scope(dev(), force=True) if case.scope else contextlib.nullcontext()), torch.no_grad():
            yield
    finally:
        for k in knobs:
            vh.tune_set(k, D.KNOB_DEFAULTS.get(k, 8))                                          # (knob 22, persistent Winograd stages: default 8)


def _layer(case, w):
    from alphapose.models import hip_train
    c = case
    conv = torch.nn.Conv2d(c.cin, c.cout, c.k, c.stride, c.pad, bias=False, device=dev())
    conv.weight.data.copy_(w)
    layer = hip_train._ConvBN(conv, torch.nn.BatchNorm2d(c.cout), False)
    assert layer.wino == D.is_winograd(c)
    return layer


def _direct(vh, case, dz, w, res, only=None, out=None):
    """The launches of D.launches(case) on conv2d_fwd_ex with the case's cout_k, one by one: what lets a single phase and a caller's ``out``
    be tested (a Winograd case: its one launch with ``out``).  hip_train._igemm_dgrad, which _DeformConvBN.backward and the head call with
    their cout_k, must give the same bits (test_the_assembler_equals_the_direct_launches)."""
    c = case
    if D.is_winograd(c):
        return vh.conv3x3_winograd_fwd(dz, vh.pack_winograd_weight(w, data_gradient=True), None, None, c.cin, False, residual=res, out=out)
    if out is None:
        if (c.k, c.stride) == (1, 2):
            out = torch.zeros((c.n, c.h, c.w, c.cin), device=dev()) if res is None else res.clone()
        else:
            out = torch.empty((c.n, c.h, c.w, c.cin), device=dev())
    for i, L in enumerate(D.launches(c)):
        if only is None or i in only:
            wd = vh.pack_dgrad_weight(w, L.taps, cout_k=c.coutk if c.coutk != c.cout else None)
            vh.conv2d_fwd_ex(dz, wd, c.cin, L.r, L.s, 1, L.pad_y, L.pad_x, L.ho, L.wo, c.h, c.w, L.osy, L.osx, L.ooy, L.oox, out=out, residual=res)
    return out


def _run(vh, case, dz, w, res, knobs=None, only=None, out=None):
    with _setup(vh, case, knobs):
        if case.via == "layer" and only is None and out is None:
            return _layer(case, w)._dgrad(dz, (case.n, case.h, case.w, case.cin), res)
        return _direct(vh, case, dz, w, res, only, out)


DIRECT_CASES = [c for c in D.CASES if c.via != "layer"]


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("case", DIRECT_CASES, ids=ids(DIRECT_CASES))
def test_the_assembler_equals_the_direct_launches(vh, case, with_res):
    """hip_train._igemm_dgrad with the case's cout_k — the call of _DeformConvBN.backward (27 in 32 channels, stride 1 and 2) and of the
    head (17 in 32) — against the launches of D.launches(case) issued here one by one: the same bits."""
    from alphapose.models import hip_train
    c = case
    assert DIRECT_CASES and c.stride in (1, 2)
    dz, w, res, _, _, _ = _data(c, "random")
    r = res if with_res else None
    with _setup(vh, c):
        got = hip_train._igemm_dgrad(dz, w, (c.n, c.h, c.w, c.cin), c.k, c.k, c.stride, c.pad, residual=r, cout_k=c.coutk if c.coutk != c.cout else None)
        want = _direct(vh, c, dz, w, r)
    assert got.shape == want.shape and torch.equal(got, want)


def _first_wrong(got, want):
    bad = np.argwhere(~(got == want))                                                         # NaN counts as wrong
    return len(bad), [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:5]]


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_integer_inputs_equal_float64_exactly(vh, case, with_res):
    dz, w, res, ref, res64, _ = _data(case, "integer")
    got = _run(vh, case, dz, w, res if with_res else None).cpu().numpy()
    want64 = ref + res64 if with_res else ref
    want = want64.astype(np.float32)
    assert got.shape == want.shape and np.array_equal(want.astype(np.float64), want64)         # the cast is exact
    count, first = _first_wrong(got, want)
    record("dgrad_integer_" + D.case_id(case), residual=with_res, mismatches=count)
    assert count == 0, (count, "(image, row, column, channel), got, want:", first)


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_impulse_inputs_copy_single_filter_elements(vh, case):
    c, w_host = case, D.impulse_weights(case)
    w = to_dev(w_host)
    ho, wo = D.out_size(c)
    dz = torch.zeros((c.n, ho, wo, c.coutk), device=dev())
    worst = 0.0
    for b, ch, oy, ox in D.impulse_sites(c):
        dz[b, oy, ox, ch] = 1.0
        got = _run(vh, c, dz, w, None)
        dz[b, oy, ox, ch] = 0.0
        want = torch.zeros_like(got)
        for (iy, ix), (r, s) in D.impulse_footprint(c, oy, ox):
            want[b, iy, ix, :] = w[ch, :, r, s]
        if D.is_winograd(c):
            worst = max(worst, float((got - want).abs().max()))
            assert torch.isfinite(got).all() and worst <= TOL * float(np.abs(w_host).max()), ((b, ch, oy, ox), worst)
        elif not torch.equal(got, want):
            count, first = _first_wrong(got.cpu().numpy(), want.cpu().numpy())
            raise AssertionError(f"impulse at (image, channel, row, column) {(b, ch, oy, ox)}: {count} wrong, first (image, row, column, channel), got, want: {first}")
    if D.is_winograd(c):
        record("dgrad_impulse_" + D.case_id(c), err=worst)


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_random_inputs_against_float64(vh, case, with_res):
    dz, w, res, ref, res64, s = _data(case, "random")
    r = res if with_res else None
    out = _run(vh, case, dz, w, r)
    assert torch.equal(_run(vh, case, dz, w, r), out)                                          # fixed summation order
    got = out.cpu().numpy().astype(np.float64)
    want = ref + res64 if with_res else ref
    s = s + np.abs(res64) if with_res else s
    assert got.shape == want.shape
    err = np.abs(got - want)
    e = rel_err(got, want)
    ratio = float((err[s > 0] / (D.U * s[s > 0])).max())
    q = D.plan(case)
    record("dgrad_" + D.case_id(case), residual=with_res, rel=e, ratio=ratio, M=[m for m, _, _ in q["launches"]] if q["direct"] else case.n * case.h * case.w,
           K=case.k * case.k * case.cout, routes=q["routes"])
    print(f"{D.case_id(case)}: rel {e:.3e} max |err| / (u S) {ratio:.3f}")
    assert np.isfinite(got).all() and e < (TOL if D.is_winograd(case) else DIRECT_TOL), e
    if not D.is_winograd(case):
        bound = D.elementwise_bound(case, s)
        worst = np.unravel_index(np.argmax(err - bound), got.shape)
        assert (err <= bound).all(), (worst, got[worst], want[worst], bound[worst])


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_the_case_reaches_the_branch_its_comment_names(vh, case):
    dz, w, res, _, _, _ = _data(case, "integer")
    q = D.plan(case)
    with vh.flop_meter() as fm:
        _run(vh, case, dz, w, res)
    routes = {k: v for k, v in fm.routes.items() if v}
    assert routes == q["routes"] and case.route in routes, (routes, q["routes"])
    assert (fm.direct, fm.winograd) == ((q["flops"], 0.0) if q["direct"] else (0.0, q["flops"])), (fm.direct, fm.winograd, q)


@pytest.mark.parametrize("case", [c for c in D.CASES if not D.is_winograd(c)], ids=ids([c for c in D.CASES if not D.is_winograd(c)]))
def test_packed_filters_are_the_host_layout(vh, case):
    """pack_dgrad_weight against the host statement of its layout, for the taps of every launch of the case: [CinPad][taps][CoutK], zero
    behind Cin and behind Cout (the padded dz channels are zero as well: 0 * 0, never 0 * garbage)."""
    c = case
    _, w, _, _, _, _ = _data(c, "integer")
    w_host = w.cpu().numpy()
    assert vh.conv_cout_pad(c.cin) == D.cout_pad(c.cin)
    for L in D.launches(c):
        wd = vh.pack_dgrad_weight(w, L.taps, cout_k=c.coutk if c.coutk != c.cout else None).cpu().numpy()
        want = D.expect_dgrad_pack(w_host, L.taps, c.coutk)
        assert wd.shape == want.shape == (D.cout_pad(c.cin), L.r * L.s, c.coutk)
        assert np.array_equal(wd.view(np.int32), want.view(np.int32)), L.taps
        assert not wd[c.cin:].any() and not wd[:, :, c.cout:].any()


def _alternatives(case):
    """Other settings of the product knobs for a case that sets some: [(knobs, routes they must give)], all documented bit-identical."""
    n = len(D.launches(case)) if not D.is_winograd(case) else 1
    alt = [({}, None)]                                                                        # the defaults
    if case.route == D.WINO_PERSIST:
        alt.append(({22: 0}, {D.WINO: 1}))                                                    # knob 22: persistent Winograd route off
    if dict(case.knobs).get(D.BM) == 128:
        alt.append(({D.BM: 64}, {D.IGEMM: n}))
    if case.route == D.PERSISTENT:
        alt.append(({D.BM: 128, D.PERSIST_K: 0}, {D.IGEMM: 1}))                               # the tiled kernel on the same 128x128 tiles
    if case.route == D.RING:
        alt.append(({D.BM: 128, D.VAR: 2}, {D.IGEMM: 1}))
    if case.route == D.WINO_2H:
        alt.append(({D.WINO_HALVES: 1}, {D.WINO: 1}))
    return alt


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("case", KNOB_CASES, ids=ids(KNOB_CASES))
def test_knob_settings_give_the_same_bits(vh, case, with_res):
    dz, w, res, _, _, _ = _data(case, "random")
    r = res if with_res else None
    base = _run(vh, case, dz, w, r)
    for knobs, want_routes in _alternatives(case):
        with vh.flop_meter() as fm:
            other = _run(vh, case, dz, w, r, knobs=knobs)
        routes = {k: v for k, v in fm.routes.items() if v}
        assert want_routes is None or routes == want_routes, (knobs, routes)
        assert torch.equal(other, base), (knobs, routes)
    if case.knobs and not D.is_winograd(case):                                                # the defaults take another tile or kernel: the knob is needed
        assert D.plan(case._replace(knobs=()))["tile"] != D.plan(case)["tile"]


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=dev()).view(torch.float32)


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("phase", range(4), ids=["even_even", "even_odd", "odd_even", "odd_odd"])
@pytest.mark.parametrize("case", S2_CASES, ids=ids(S2_CASES))
def test_one_stride2_phase_writes_its_own_pixels_only(vh, case, phase):
    c = case
    dz, w, res, ref, res64, _ = _data(c, "integer")
    L = D.launches(c)[phase]
    assert (L.ooy, L.oox) == divmod(phase, 2) and len(L.taps) == (1, 2, 2, 4)[phase]
    buf = _sentinel(c.n, c.h, c.w, c.cin)
    with vh.flop_meter() as fm:
        _run(vh, c, dz, w, res, only=(phase,), out=buf)
    assert fm.routes[D.plan(c)["launches"][phase][2]] == 1 and sum(fm.routes.values()) == 1, fm.routes
    mine = torch.zeros((c.h, c.w), dtype=torch.bool, device=dev())
    mine[L.ooy::2, L.oox::2] = True
    assert (_bits(buf[:, ~mine]) == SENTINEL).all()                                           # the other three phases' pixels
    got, want = buf[:, mine].cpu().numpy(), (ref + res64).astype(np.float32)[:, mine.cpu().numpy()]
    count, first = _first_wrong(got, want)
    assert count == 0, (count, "(image, pixel of the phase, channel), got, want:", first)


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("case", P2_CASES, ids=ids(P2_CASES))
def test_1x1_stride2_leaves_the_odd_pixels_alone(vh, case, with_res):
    """Only the even pixels receive gradient: the others are +0.0, or the residual bit for bit (the launch writes into a clone of it)."""
    c = case
    dz, w, res, ref, res64, _ = _data(c, "random")
    res = -res.abs() - 1.0                                                                    # negative everywhere: a fill of zeros would show
    got = _run(vh, c, dz, w, res if with_res else None)
    odd = torch.ones((c.h, c.w), dtype=torch.bool, device=dev())
    odd[0::2, 0::2] = False
    if with_res:
        assert torch.equal(_bits(got[:, odd]), _bits(res[:, odd]))
        assert not (got[:, ~odd] == res[:, ~odd]).all(dim=-1).any()                           # every even pixel received something
    else:
        assert (_bits(got[:, odd]) == 0).all()
        assert (got[:, ~odd] != 0).any(dim=-1).all()
    want = ref[:, 0::2, 0::2] + (res.cpu().numpy().astype(np.float64)[:, 0::2, 0::2] if with_res else 0.0)
    assert rel_err(got[:, 0::2, 0::2].cpu().numpy(), want) < DIRECT_TOL


@pytest.mark.parametrize("case", SK_CASES, ids=ids(SK_CASES))
def test_streamk_scope_is_reproducible_and_leaves_nothing_behind(vh, case):
    """Inside the scope the launch that passes streamk_wanted finishes tiles from workspace slabs (the stride-2 phase then scatters them):
    the route counter says so, two runs agree bit for bit, and a run after the scope equals the run before it."""
    dz, w, res, ref, res64, _ = _data(case, "random")
    outside = case._replace(scope=False)
    n = len(D.launches(case))
    with vh.flop_meter() as fb:
        before = _run(vh, outside, dz, w, res)
    with vh.flop_meter() as fm:
        first = _run(vh, case, dz, w, res)
    second = _run(vh, case, dz, w, res)
    with vh.flop_meter() as fa:
        after = _run(vh, outside, dz, w, res)
    assert fb.routes[D.STREAMK] == fa.routes[D.STREAMK] == 0 and fb.routes[D.IGEMM] == fa.routes[D.IGEMM] == n
    assert fm.routes[D.STREAMK] == 1 and fm.routes[D.IGEMM] == n - 1, fm.routes
    assert torch.equal(first, second) and torch.equal(after, before)
    e = rel_err(first.cpu().numpy(), before.cpu().numpy())
    record("dgrad_streamk_vs_tiles_" + D.case_id(case), rel=e, same_bits=bool(torch.equal(first, before)))
    assert e < DIRECT_TOL, e


@pytest.mark.parametrize("case", WRITE_CASES, ids=ids(WRITE_CASES))
def test_writes_stay_inside_the_output(vh, case):
    c = case
    dz, w, res, ref, res64, _ = _data(c, "integer")
    numel, margin = c.n * c.h * c.w * c.cin, 256
    buf = _sentinel(numel + 2 * margin)
    out = buf[margin:margin + numel].view(c.n, c.h, c.w, c.cin)
    got = _run(vh, c, dz, w, res, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert (_bits(buf[:margin]) == SENTINEL).all() and (_bits(buf[margin + numel:]) == SENTINEL).all()
    want = (ref + res64).astype(np.float32)
    if (c.k, c.stride) == (1, 2):                                                              # the odd pixels are the caller's (zeros or a residual clone)
        odd = torch.ones((c.h, c.w), dtype=torch.bool, device=dev())
        odd[0::2, 0::2] = False
        assert (_bits(out[:, odd]) == SENTINEL).all() and not (_bits(out[:, ~odd]) == SENTINEL).any()
        assert np.array_equal(out[:, 0::2, 0::2].cpu().numpy(), want[:, 0::2, 0::2])
    else:
        assert not (_bits(out) == SENTINEL).any()                                              # every element written
        assert np.array_equal(out.cpu().numpy(), want)


def test_bad_arguments_are_refused_before_any_launch(vh):
    EINVAL = -1
    lib, st = vh.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    z = lambda *shape: torch.zeros(shape, device=dev())
    p = lambda t: None if t is None else t.data_ptr()
    x32, x48 = z(2, 4, 3, 32), z(2, 4, 3, 48)
    y = _sentinel(2 * 4 * 3 * 192)

    def call(x, w, out, n, cin, cout, coutpad):
        # (x, w, scale, bias, residual, y, N, H, W, Cin, Cout, CoutPad, R, S, stride, pad_y, pad_x, Ho, Wo, OH, OW, osy, osx, ooy, oox, relu, stream)
        return lib.vatl_conv2d_fwd_ex(p(x), p(w), None, None, None, p(out), n, 4, 3, cin, cout, coutpad, 1, 1, 1, 0, 0, 4, 3, 4, 3, 1, 1, 0, 0, 0, st)

    w = z(256 * 48)
    with vh.flop_meter() as fm:
        start = fm.launches_now()
        assert call(x48, w, y, 2, 48, 64, 64) == EINVAL                                        # Cin % 32 != 0
        assert b"multiple of 32" in lib.vatl_last_error()
        for cout, coutpad in ((96, 96), (64, 32), (64, 96), (192, 192), (16, 16)):             # CoutPad no multiple of the 128 / 64 / 32 column tile
            assert call(x32, w, y, 2, 32, cout, coutpad) == EINVAL, (cout, coutpad)
            assert b"CoutPad" in lib.vatl_last_error()
        assert call(x32, w, None, 2, 32, 64, 64) == EINVAL                                     # null output
        assert call(None, w, y, 2, 32, 64, 64) == EINVAL and call(x32, None, y, 2, 32, 64, 64) == EINVAL
        assert call(x32, w, y, 0, 32, 64, 64) == EINVAL                                        # empty batch
        with pytest.raises(vh.VatlError):                                                      # the wrapper raises on the same arguments
            vh.conv2d_fwd_ex(x48, w.view(64, 1, 192)[:, :, :48].contiguous(), 64, 1, 1, 1, 0, 0, 4, 3, 4, 3, 1, 1, 0, 0)
        with pytest.raises(vh.VatlError):
            vh.conv2d_fwd_ex(x32, z(96, 1, 32), 96, 1, 1, 1, 0, 0, 4, 3, 4, 3, 1, 1, 0, 0)
        assert fm.launches_now() == start == 0
    torch.cuda.synchronize()
    assert sum(fm.routes.values()) == 0 and fm.total == 0 and (_bits(y) == SENTINEL).all()
    assert call(x32, w, y, 2, 32, 64, 64) == 0                                                 # conforming arguments of the same shapes pass
    torch.cuda.synchronize()
    assert not (_bits(y[:2 * 4 * 3 * 64]) == SENTINEL).any() and (_bits(y[2 * 4 * 3 * 64:]) == SENTINEL).all()
