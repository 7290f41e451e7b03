"""Kernels whose bits are pinned to what the library of the commit before a refactor wrote (tools/make_scorer_bits.py, tests/golden/README.md):
  tests/scorer_cases.py  tests/golden/scorer_bits.npz  the scorer kernels (csrc/decode.hip, localpeak.hip, heatmap_criteria.hip, pose_feature.hip).
                         Their contract with the reference is exactness — integer results, HP, decoded coordinates.
  tests/glue_cases.py    tests/golden/glue_bits.npz    the HBM-bound passes of the fine-tune step (csrc/layout.hip, pool.hip, fusion.hip, pack.hip,
                         bn_train.hip): the fused stem tail relies on the pool kernels agreeing bit for bit, and the step on being reproducible.
  tests/wino43_cases.py  tests/golden/wino43_bits.npz  the F(4x3,2x2) Winograd kernels and their filter packs (csrc/winograd_deconv43.hip, winograd_s2_43.hip,
                         winograd43.h, winograd_stage.h, tile_order.h) and one layer per route of csrc/conv_winograd.hip's launcher.
  tests/train_epilogue_cases.py  tests/golden/train_epilogue_bits.npz  the training write-outs of the convolutions (csrc/bn_epilogue.h in conv_igemm.h,
                         conv_winograd.hip, winograd_f4.hip): stored tensor, float64 (sum, sum^2) / (sum g, sum g * xhat) partials, block and route counts.
Any moved bit is a failure, whatever moved it."""
import numpy as np
import pytest

from tests import glue_cases, scorer_cases, train_epilogue_cases, wino43_cases

pytestmark = pytest.mark.gpu

MODULES = (scorer_cases, glue_cases, wino43_cases, train_epilogue_cases)
assert len({name for m in MODULES for name in m.CASES}) == sum(len(m.CASES) for m in MODULES)


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


@pytest.fixture(scope="module")
def golden_bits():
    return {m: np.load(m.GOLDEN) for m in MODULES}


def test_fixture_holds_exactly_the_cases(golden_bits):
    for m in MODULES:
        have = {k.rsplit(".", 1)[0] for k in golden_bits[m].files if k != "parent_commit"}
        assert have == set(m.CASES), (m.__name__, sorted(have ^ set(m.CASES)))


@pytest.mark.parametrize("cases,name", [pytest.param(m, name, id=name) for m in MODULES for name in m.CASES])
def test_bits_are_the_recorded_ones(vh, golden_bits, cases, name):
    got = cases.run(vh, name)
    assert got, name
    for key, have in got.items():
        want = golden_bits[cases][key]
        assert have.dtype == want.dtype and have.shape == want.shape, (key, have.dtype, have.shape, want.dtype, want.shape)
        bad = np.flatnonzero(have.reshape(-1) != want.reshape(-1))
        print(f"{key}: {bad.size} of {want.size} stored words differ", bad[:8])
        assert bad.size == 0, (key, bad[:8], have.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])
