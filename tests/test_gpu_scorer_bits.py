"""The scorer kernels (csrc/decode.hip, localpeak.hip, heatmap_criteria.hip, pose_feature.hip) against tests/golden/scorer_bits.npz: the
bits the library of the commit before they were re-cut by family wrote for the cases of tests/scorer_cases.py (tools/make_scorer_bits.py,
tests/golden/README.md).  Their contract with the reference is exactness — integer results, HP, decoded coordinates — so any moved bit
is a failure, whatever moved it."""
import numpy as np
import pytest

from tests import scorer_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


@pytest.fixture(scope="module")
def golden_bits():
    return np.load(scorer_cases.GOLDEN)


def test_fixture_holds_exactly_the_cases(golden_bits):
    have = {k.rsplit(".", 1)[0] for k in golden_bits.files if k != "parent_commit"}
    assert have == set(scorer_cases.CASES), sorted(have ^ set(scorer_cases.CASES))


@pytest.mark.parametrize("name", list(scorer_cases.CASES))
def test_bits_are_the_recorded_ones(vh, golden_bits, name):
    got = scorer_cases.run(vh, name)
    assert got, name
    for key, have in got.items():
        want = golden_bits[key]
        assert have.dtype == want.dtype and have.shape == want.shape, (key, have.dtype, have.shape, want.dtype, want.shape)
        bad = np.flatnonzero(have.reshape(-1) != want.reshape(-1))
        print(f"{key}: {bad.size} of {want.size} stored words differ", bad[:8])
        assert bad.size == 0, (key, bad[:8], have.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])
