"""Weight-gradient kernels (csrc/conv_wgrad.hip, csrc/winograd_wgrad.hip), every tile, packing, walk and split branch on its own at
small batch: the cases, the float64 reference and the impulse inputs of tests/wgrad_cases.py (proved in tests/test_wgrad_cpu.py).

    random inputs    normwise error against float64 below the bars of the neighbouring files (5e-5 direct, TOL Winograd, 2 TOL between
                     the routes), two runs bit-identical, and for the direct kernels |got - ref| <= 2 gamma_n S element by element
    impulse inputs   the direct kernels copy the gathered operand bit for bit; the Winograd kernels to TOL * max|x|
    branch           the route counters, the metered FLOPs and the library's own slice count are what the case's comment claims
    writes           the words around ``out`` and behind the workspace keep their sentinel
    refusals         bad channel counts and mismatched operand grids are refused before any launch

Measured figures per case: profiles/wgrad_notes.md."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import wgrad_cases as W
from tests.gpu_util import dev, record, rel_err, to_dev

pytestmark = pytest.mark.gpu

DIRECT_TOL = 5e-5     # tests/test_gpu_train.py::test_conv_dgrad_wgrad
TOL = 2e-5            # tests/test_gpu_winograd.py
IDS = [W.case_id(c) for c in W.CASES]
DIRECT_CASES = [c for c in W.CASES if not W.is_winograd(c)]
SENTINEL = 0x7FC12345                                            # a NaN no kernel writes: compared as bits
BY_ID = dict(zip(IDS, W.CASES))
# stem, head in 32 channels, packed taps, transposed conv, Winograd with one and with two halves
WRITE_CASES = [BY_ID[i] for i in ("conv-1x8x8-3-64-k7s2", "conv-2x8x6-128-17in32-k3s1", "conv-2x8x6-32-32-k3s1", "deconv-3x5x4-32-32-k4s2",
                                  "wino-2x8x6-256-288-k3s1", "wino-2x8x6-256-256-k3s1")]


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


@functools.lru_cache(maxsize=None)
def _random(case):
    """(plain, gathered) on the device, the float64 reference and S of the case's random inputs: computed once, shared, left alone."""
    plain, gathered = W.random_inputs(case)
    return to_dev(plain), to_dev(gathered), W.reference(case, (plain, gathered)), W.abs_sum(case, (plain, gathered))


def _run(vh, case, plain, gathered, out=None, entry=None):
    entry = entry or case[0]
    _, _, _, _, cin, cout, _, k, stride, pad = case
    if entry == W.DIRECT:
        return vh.conv2d_wgrad(gathered, plain, cout, cin, k, k, stride, pad, out=out)
    if entry == W.WINO:
        return vh.conv3x3_winograd_wgrad(gathered, plain, out=out)
    return (vh.deconv4x4s2_wgrad if entry == W.DECONV else vh.deconv4x4s2_winograd_wgrad)(plain, gathered, out=out)


def _other_route(case):
    """The entry point of the other route where it accepts the shape."""
    entry, _, _, _, cin, cout, coutg, k, stride, pad = case
    if entry == W.DIRECT:
        return W.WINO if (k, stride, pad) == (3, 1, 1) and coutg == cout and cin != 3 else None
    return {W.DECONV: W.WINO_DECONV, W.WINO: W.DIRECT, W.WINO_DECONV: W.DECONV}[entry]


def _library_slices(vh, case):
    """Partial gradients a direct launch sums, from the library's own workspace size."""
    _, _, _, _, cin, cout, _, k, _, _ = case
    g = W.geometry(case)
    floats = vh.lib().vatl_deconv4x4s2_wgrad_workspace_floats(cin, cout, g["M"]) if W.is_deconv(case) else \
        vh.lib().vatl_conv2d_wgrad_workspace_floats(cout, cin, k, k, g["M"])
    packed = cin * 16 * cout if W.is_deconv(case) else (cout * k * 32 if cin == 3 else cout * k * k * cin)
    assert floats > 0 and floats % packed == 0, (floats, packed)
    return floats // packed, floats


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_random_inputs_against_float64(vh, case):
    plain, gathered, ref, s = _random(case)
    dw = _run(vh, case, plain, gathered)
    got = dw.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    e = rel_err(got, ref)
    ratio = float((np.abs(got - ref)[s > 0] / (W.U * s[s > 0])).max())
    slices = None if W.is_winograd(case) else _library_slices(vh, case)[0]
    record("wgrad_" + W.case_id(case), rel=e, ratio=ratio, slices=slices, M=W.geometry(case)["M"])
    print(f"{W.case_id(case)}: rel {e:.3e} max |err| / (u S) {ratio:.3f} slices {slices}")
    assert e < (TOL if W.is_winograd(case) else DIRECT_TOL), e
    assert torch.equal(_run(vh, case, plain, gathered), dw)                                       # fixed reduction order
    if not W.is_winograd(case):
        bound = W.elementwise_bound(case, slices, s)
        worst = np.unravel_index(np.argmax(np.abs(got - ref) - bound), got.shape)
        assert (np.abs(got - ref) <= bound).all(), (worst, got[worst], ref[worst], bound[worst])
    other = _other_route(case)
    if other is not None:
        e2 = rel_err(_run(vh, case, plain, gathered, entry=other).cpu().numpy(), got)
        print(f"{W.case_id(case)}: against {other} {e2:.3e}")
        assert e2 < 2 * TOL, (other, e2)


@pytest.mark.parametrize("case", W.TWO_HALF_CASES, ids=[W.case_id(c) for c in W.TWO_HALF_CASES])
def test_two_half_shapes_on_one_half_blocks(vh, case):
    """vatl_tune_set(23, 1) sends a two-half shape through the one-half kernel.  The knob changes the summation order, so only the
    profiling variant of the library has it (include/vatl_hip.h); the shipped library must refuse it, and then no launch of it can
    leave the two-half kernel."""
    plain, gathered, ref, _ = _random(case)
    try:
        vh.tune_set(23, 1)
    except vh.VatlError as err:
        assert "not a product knob" in str(err)
        with vh.flop_meter() as fm:
            _run(vh, case, plain, gathered)
        assert fm.routes["winograd_wgrad_2h"] == 1 and fm.routes["winograd_wgrad"] == 0
        return
    try:
        with vh.flop_meter() as fm:
            dw = _run(vh, case, plain, gathered)
        e = rel_err(dw.cpu().numpy(), ref)
        record("wgrad_one_half_" + W.case_id(case), rel=e)
        assert fm.routes["winograd_wgrad"] == 1 and fm.routes["winograd_wgrad_2h"] == 0
        assert e < TOL, e
    finally:
        vh.tune_set(23, 2)


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_impulse_inputs_copy_the_gathered_operand(vh, case):
    plain, gathered, expected = W.impulse(case)
    dw = _run(vh, case, to_dev(plain), to_dev(gathered)).cpu()
    assert tuple(dw.shape) == expected.shape
    if W.is_winograd(case):
        err = float(np.abs(dw.numpy().astype(np.float64) - expected).max())
        record("wgrad_impulse_" + W.case_id(case), err=err)
        assert err <= TOL * float(np.abs(gathered).max()), err
        return
    want = torch.from_numpy(expected.astype(np.float32))
    assert np.array_equal(want.numpy().astype(np.float64), expected)
    bad = np.argwhere((dw + 0.0 != want + 0.0).numpy())                                           # + 0.0: -0 counts as +0
    assert torch.equal(dw + 0.0, want + 0.0), (len(bad), bad[:5].tolist(), [(float(dw[tuple(i)]), float(want[tuple(i)])) for i in bad[:5]])


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_the_case_reaches_the_branch_its_comment_names(vh, case):
    plain, gathered, _, _ = _random(case)
    g, claim = W.geometry(case), W.CLAIMS[case]
    with vh.flop_meter() as fm:
        _run(vh, case, plain, gathered)
    routes = {k: v for k, v in fm.routes.items() if v}
    cdiv = lambda a, b: -(-a // b)
    if not W.is_winograd(case):
        (bn, bj), tpt = claim["tile"], claim["tpt"]
        stem = (bn, bj) == (64, 32)                                                                # one column tile per filter row: 8 taps x 4 channels
        tiles = cdiv(g["Cn"], bn) * (g["R"] if stem else cdiv(g["R"] * g["S"], tpt) * cdiv(g["Cx"], bj))
        assert routes == {"wgrad": 1}, routes
        assert fm.winograd == 0 and fm.direct == 2.0 * tiles * bn * bj * 32 * cdiv(g["M"], 32), (fm.direct, tiles, bn, bj)
        assert _library_slices(vh, case)[0] == claim["slices"]
        return
    q = W.winograd_plan(case)
    assert (q["halves"], q["table"], q["splits"]) == (claim["halves"], claim["table"], claim["splits"])
    want = {"winograd_wgrad_2h" if claim["halves"] == 2 else "winograd_wgrad": 1}
    if claim["table"]:
        want["winograd_wgrad_table"] = 1
    assert routes == want, routes
    _, n, h, w, cin, cout, _, _, _, _ = case
    ws = vh.lib().vatl_deconv4x4s2_winograd_wgrad_workspace_floats(cin, cout, n, h, w) if W.is_deconv(case) else \
        vh.lib().vatl_conv3x3_winograd_wgrad_workspace_floats(cout, cin, n, h, w)
    assert ws == q["floats"], (ws, q)                                                              # pins the split count, the halves and the tables
    assert fm.direct == 0 and fm.winograd == q["flops"], (fm.winograd, q["flops"])


def _sentinel(numel):
    return torch.full((numel,), SENTINEL, dtype=torch.int32, device=dev()).view(torch.float32)


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("case", WRITE_CASES, ids=[W.case_id(c) for c in WRITE_CASES])
def test_writes_stay_inside_the_output_and_the_workspace(vh, case):
    plain, gathered, _, _ = _random(case)
    want = _run(vh, case, plain, gathered)
    numel, margin = want.numel(), 256
    buf = _sentinel(numel + 2 * margin)
    got = _run(vh, case, plain, gathered, out=buf[margin:margin + numel])
    assert got.data_ptr() == buf[margin:].data_ptr()
    assert (_bits(buf[:margin]) == SENTINEL).all() and (_bits(buf[margin + numel:]) == SENTINEL).all()
    assert not (_bits(buf[margin:margin + numel]) == SENTINEL).any()                               # every element written
    assert torch.equal(buf[margin:margin + numel], want.reshape(-1))
    if W.is_winograd(case):
        return
    # the C ABI with a workspace 4096 floats longer than the library asks for: the tail keeps its sentinel
    _, n, h, w, cin, cout, coutg, k, stride, pad = case
    floats = _library_slices(vh, case)[1]
    ws, dw = _sentinel(floats + 4096), torch.empty_like(want)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if W.is_deconv(case):
        rc = vh.lib().vatl_deconv4x4s2_wgrad(plain.data_ptr(), gathered.data_ptr(), dw.data_ptr(), ws.data_ptr(), n, h, w, cin, cout, st)
    else:
        rc = vh.lib().vatl_conv2d_wgrad(gathered.data_ptr(), plain.data_ptr(), dw.data_ptr(), ws.data_ptr(), n, h, w, cin, cout, coutg, k, k, stride, pad, st)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(dw, want)
    assert (_bits(ws[floats:]) == SENTINEL).all()


def test_bad_channel_counts_are_refused_before_any_launch(vh):
    z = lambda *shape: torch.zeros(shape, device=dev())
    EINVAL = -1
    lib, st = vh.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, dz, dw, ws = z(1, 4, 4, 16), z(1, 4, 4, 16), z(4096), z(1 << 16)
    p = lambda t: t.data_ptr()
    with vh.flop_meter() as fm:
        # (N, H, W, Cin, Cout, CoutG, R, S, stride, pad)
        for args in ((1, 4, 4, 6, 8, 8, 3, 3, 1, 1),          # Cin % 4 != 0 on a non-stem layer
                     (1, 4, 4, 8, 4, 6, 3, 3, 1, 1),          # CoutG % 4 != 0
                     (1, 4, 4, 8, 12, 8, 3, 3, 1, 1),         # CoutG < Cout
                     (1, 4, 4, 3, 8, 8, 9, 9, 2, 4)):         # stem filter wider than 8
            assert lib.vatl_conv2d_wgrad(p(x), p(dz), p(dw), p(ws), *args, st) == EINVAL, args
        assert lib.vatl_deconv4x4s2_wgrad(p(x), p(dz), p(dw), p(ws), 1, 2, 2, 6, 8, st) == EINVAL
        for cin, cout in ((6, 8), (8, 6)):                    # Winograd channel counts that are no multiples of 4
            assert lib.vatl_conv3x3_winograd_wgrad(p(x), p(dz), p(dw), p(ws), 1, 4, 4, cin, cout, st) == EINVAL
            assert lib.vatl_deconv4x4s2_winograd_wgrad(p(x), p(dz), p(dw), p(ws), 1, 2, 2, cin, cout, st) == EINVAL
        # the wrappers raise on the same arguments
        with pytest.raises(vh.VatlError):
            vh.conv2d_wgrad(z(1, 4, 4, 6), z(1, 4, 4, 8), 8, 6, 3, 3, 1, 1)
        with pytest.raises(vh.VatlError):
            vh.conv2d_wgrad(z(1, 4, 4, 8), z(1, 4, 4, 6), 4, 8, 3, 3, 1, 1)
        with pytest.raises(vh.VatlError):
            vh.conv2d_wgrad(z(1, 4, 4, 8), z(1, 4, 4, 8), 12, 8, 3, 3, 1, 1)
        with pytest.raises(vh.VatlError):
            vh.conv2d_wgrad(z(1, 4, 4, 4), z(1, 2, 2, 8), 8, 3, 9, 9, 2, 4)
        with pytest.raises(vh.VatlError):
            vh.conv3x3_winograd_wgrad(z(1, 4, 4, 6), z(1, 4, 4, 8))
        with pytest.raises(vh.VatlError):
            vh.deconv4x4s2_winograd_wgrad(z(1, 2, 2, 8), z(1, 4, 4, 6))
    assert sum(fm.routes.values()) == 0 and fm.total == 0


def test_mismatched_operands_are_refused_before_any_launch(vh):
    """The kernels take the gradient's pixel grid from the input's shape and the filter geometry: a gradient of another grid or batch
    would be read with the wrong strides, so the wrappers refuse it."""
    z = lambda *shape: torch.zeros(shape, device=dev())
    with vh.flop_meter() as fm:
        for dz in (z(2, 5, 3, 16), z(2, 4, 4, 16), z(3, 4, 3, 16), z(2, 12, 16), z(2, 8, 6, 16)):    # 3x3 stride 2 pad 1 of 8x6 gives 4x3
            with pytest.raises(vh.VatlError):
                vh.conv2d_wgrad(z(2, 8, 6, 8), dz, 16, 8, 3, 3, 2, 1)
        with pytest.raises(vh.VatlError):
            vh.conv2d_wgrad(z(2, 8, 6, 16), z(2, 4, 3, 16), 16, 8, 3, 3, 2, 1)                        # input carries 16 channels, the layer reads 8
        with pytest.raises(vh.VatlError):
            vh.conv2d_wgrad(z(2, 8, 6, 3), z(2, 4, 3, 16), 16, 3, 7, 7, 2, 3)                         # the stem's input comes in 4 channels
        with pytest.raises(vh.VatlError):
            vh.conv2d_wgrad(z(2, 2, 2, 8), z(2, 0, 0, 16), 16, 8, 5, 5, 1, 0)                         # filter larger than the padded image
        for f in (vh.deconv4x4s2_wgrad, vh.deconv4x4s2_winograd_wgrad):
            for dy in (z(2, 4, 3, 8), z(2, 8, 7, 8), z(2, 9, 6, 8), z(1, 8, 6, 8), z(2, 48, 8)):
                with pytest.raises(vh.VatlError):
                    f(z(2, 4, 3, 16), dy)
        for dz in (z(2, 8, 5, 16), z(2, 7, 6, 16), z(3, 8, 6, 16), z(2, 4, 3, 16), z(96, 16)):
            with pytest.raises(vh.VatlError):
                vh.conv3x3_winograd_wgrad(z(2, 8, 6, 8), dz)
    assert sum(fm.routes.values()) == 0 and fm.total == 0
    # conforming operands of the same shapes pass
    assert tuple(vh.conv2d_wgrad(z(2, 8, 6, 8), z(2, 4, 3, 16), 16, 8, 3, 3, 2, 1).shape) == (16, 8, 3, 3)
    assert tuple(vh.deconv4x4s2_wgrad(z(2, 4, 3, 16), z(2, 8, 6, 8)).shape) == (16, 8, 4, 4)
    assert tuple(vh.deconv4x4s2_winograd_wgrad(z(2, 4, 3, 16), z(2, 8, 6, 8)).shape) == (16, 8, 4, 4)
    assert tuple(vh.conv3x3_winograd_wgrad(z(2, 8, 6, 8), z(2, 8, 6, 16)).shape) == (16, 8, 3, 3)
