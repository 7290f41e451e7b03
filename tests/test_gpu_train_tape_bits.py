"""The float64 reference step and the bf16 step of SimplePose-R50 give, bit for bit, what they gave before the two trainers were put on one
tape (alphapose/models/hip_train_tape.py) and the two weight-gradient kernels on one geometry (csrc/wgrad_generic.h): every tensor of the
cases of tests/train_tape_cases.py against tests/golden/train_tape_parent_bits.npz (tools/make_train_tape_bits.py, recorded on the parent commit)."""
import numpy as np
import pytest

from tests import train_tape_cases as C
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


@pytest.fixture(scope="module")
def golden():
    return np.load(C.GOLDEN)


def _compare(golden, shape, run, records):
    names, sha, head = C.reduce(records)
    key = f"{C.shape_id(shape)}/{run}/"
    assert names == str(golden[key + "names"]), "the recorded tensors changed"
    bad = [n for n, a, b in zip(records, sha, golden[key + "sha256"]) if not np.array_equal(a, b)]
    print(key, len(records), "tensors,", len(bad), "differ")
    assert not bad, (key, len(bad), bad[:8])
    np.testing.assert_array_equal(head, golden[key + "head"])


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_float64_step_keeps_the_parents_bits(vh, golden, shape):
    """Heat-maps, all 170 gradients and the four statistics of all 56 BatchNorm layers."""
    _compare(golden, shape, "f64", C.run_f64(shape, dev()))


@pytest.mark.parametrize("plan", [True, False], ids=["plan", "noplan"])
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_bf16_steps_keep_the_parents_bits(vh, golden, shape, plan):
    """Heat-maps, loss, all gradients (through the arena) and every BatchNorm buffer of two steps, the second after every parameter moved: its
    filters refreshed by the plan's one launch, or per tensor."""
    one, two = C.run_h16(vh, shape, dev(), plan)
    if plan:
        _compare(golden, shape, "h16_step1", one)
    _compare(golden, shape, "h16_step2_plan" if plan else "h16_step2_noplan", two)
