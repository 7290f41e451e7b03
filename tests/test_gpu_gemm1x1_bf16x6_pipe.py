"""The software-pipelined k-loop of the bf16x6 GEMM (csrc/gemm1x1_bf16x6.hip: the fragments and the split of stage s + 1 between the MFMAs of stage s), all
forms, reached through vatl_hip.conv2d_fwd / conv1x1_rows_fwd / conv1x1_dual_fwd(..., u_x6=), at the places where such a loop goes wrong: its first stages,
its last three, the dual crossing, partial tiles (tests/bf16x6_pipe_cases.py).  Exact equality on small integers (an A fragment paired with another
stage's B fragment cannot cancel: every stage has its own data), the bits the parent commit's kernel gave on normal data
(tests/golden/bf16x6_parent_bits.npz, tools/make_bf16x6_bits.py), the float64 house bar, and row independence between NaN neighbours."""
import numpy as np
import pytest
import torch

from tests import bf16x6_pipe_cases as pc
from tests.gpu_util import record, rel_err, to_dev

BAR = 2e-5         # of the layer maximum, against float64 (tests/test_gpu_gemm1x1_bf16x6.py)


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def test_cases_cover_every_axis_and_the_integer_sums_are_exact_in_fp32():
    """No GPU: every shape, row count, residual and ReLU state occurs with every form (the dual form takes no residual), every case is one the route
    admits by its documented rule, and the int64 reference of the integer data stays below 2^24."""
    for form, shapes in pc.SHAPES.items():
        mine = [c for c in pc.CASES if c[0] == form]
        assert {c[1:4] for c in mine} == set(shapes) and {c[4] for c in mine} == set(pc.ROWS)
        assert {(c[1:4], c[4]) for c in mine} == {(s, r) for s in shapes for r in pc.ROWS}
        assert {c[5] for c in mine} == ({False} if form == "dual" else {False, True}) and {c[6] for c in mine} == {False, True}
        for c in mine:
            k = c[1] + c[2]
            assert k % 64 == 0 and (k // 16) % 4 == 0 and c[3] % 128 == 0
            assert (128 <= k < 512 and c[3] >= 512) if form == "short" else (k >= 512 if form == "long" else (k >= 384 and c[1] % 64 == 0 and c[2] % 64 == 0))
    assert len(pc.BITS) >= 8 and {c[0] for c in pc.BITS} == set(pc.SHAPES)
    for c in pc.CASES:
        d = pc.inputs(c, integers=True)
        assert all(np.abs(v).max() <= 8 and np.array_equal(v, np.round(v)) for v in d.values() if v is not None)
        assert np.abs(pc.reference(c, d, np.int64)).max() < 2 ** 24
        # every 16-k stage of a row differs from the next: a fragment of the wrong stage cannot give the right sum
        a = d["a"].reshape(-1, c[1])
        assert not any(np.array_equal(a[:, 16 * s:16 * s + 16], a[:, 16 * s + 16:16 * s + 32]) for s in range(c[1] // 16 - 1))


@pytest.mark.gpu
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_small_integers_are_exact(vh, case):
    d = pc.inputs(case, integers=True)
    want = pc.reference(case, d, np.int64)
    got = pc.run(vh, case, d, to_dev).cpu().numpy().reshape(want.shape)
    assert np.array_equal(got, want.astype(np.float32)) and np.array_equal(got.astype(np.int64), want)


@pytest.mark.gpu
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_against_float64(vh, case):
    d = pc.inputs(case, integers=False)
    want = pc.reference(case, d, np.float64)
    got = pc.run(vh, case, d, to_dev).cpu().numpy().reshape(want.shape)
    e = rel_err(got, want)
    record("gemm1x1_bf16x6_pipe_" + pc.case_id(case), vs_fp64=e)
    print(f"bf16x6 pipe {pc.case_id(case)}: {e:.3e}")
    assert e < BAR, e


@pytest.fixture(scope="module")
def parent_bits():
    return np.load(pc.GOLDEN)


@pytest.mark.gpu
@pytest.mark.parametrize("case", pc.BITS, ids=pc.case_id)
def test_the_bits_of_the_parent_kernel(vh, parent_bits, case):
    """The pipelined loop pairs the same pieces, in the same order, into the same two accumulator sets: not one bit moves."""
    y = pc.run(vh, case, pc.inputs(case, integers=False), to_dev).cpu().numpy()
    name = pc.case_id(case)
    assert np.array_equal(y.reshape(-1)[:64].view(np.uint32), parent_bits[name + "_head"]), name
    assert np.array_equal(pc.digest(y), parent_bits[name + "_sha256"]), name


# one M = 144 case per form and residual state (two m-tiles, the second partial); rows: the first | 56 .. 63 of the first wave row's 64 (in the short + residual
# form their residual travels in registers, not through the ring) | 120 and 127, the same of the second wave row | 128 and 143 in the last, partial tile
INDEPENDENT = tuple(c for c in pc.CASES if c[4] == (3, 8, 6) and (c[0], c[1]) in (("short", 128), ("short", 448), ("long", 576), ("dual", 64), ("dual", 320)))
ROWS_ALONE = (0,) + tuple(range(56, 64)) + (120, 127, 128, 143)


@pytest.mark.gpu
@pytest.mark.parametrize("case", INDEPENDENT, ids=pc.case_id)
def test_a_row_has_the_same_bits_alone_and_between_nan_rows(vh, case):
    form, k1, k2, n, (b, h, w), res, relu = case
    d = pc.inputs(case, integers=False)
    packed = pc.pack(vh, case, d, to_dev)
    solo_case = (form, k1, k2, n, (1, 1, 1), res, relu)
    a, sc = to_dev(d["a"]), None if d["scale"] is None else to_dev(d["scale"])
    x2 = None if d["x2"] is None else to_dev(d["x2"])
    rs = to_dev(d["res"]) if res else None
    full = pc.launch(vh, case, packed, a, x2, sc, rs).reshape(-1, n)
    nan = float("nan")
    for row in ROWS_ALONE:
        img, rem = divmod(row, h * w)
        oy, ox = divmod(rem, w)
        a1 = a[img, oy, ox].reshape(1, 1, 1, k1).contiguous()
        x1 = None if x2 is None else x2[img, 2 * oy, 2 * ox].reshape(1, 1, 1, k2).contiguous()
        r1 = rs[img, oy, ox].reshape(1, 1, 1, n).contiguous() if res else None
        solo = pc.launch(vh, solo_case, packed, a1, x1, sc, r1)
        assert torch.equal(solo.reshape(-1), full[row]), row
        an = torch.full_like(a, nan)
        an[img, oy, ox] = a[img, oy, ox]
        xn = rn = None
        if x2 is not None:
            xn = torch.full_like(x2, nan)
            xn[img, 2 * oy, 2 * ox] = x2[img, 2 * oy, 2 * ox]
        if res:
            rn = torch.full_like(rs, nan)
            rn[img, oy, ox] = rs[img, oy, ox]
        poisoned = pc.launch(vh, case, packed, an, xn, sc, rn).reshape(-1, n)
        assert torch.equal(poisoned[row], full[row]), row
