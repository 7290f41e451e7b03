"""The fp32 fine-tune step of SimplePose, FastPose (plain and with deformable convs) and HRNet gives, bit for bit, what it gave before the layer classes
of alphapose/models/hip_train.py were put on one data-gradient assembler (_igemm_dgrad) and one BatchNorm tape (_bn_backward): every tensor of the cases
of tests/train_step_cases.py against tests/golden/train_step_parent_bits.npz (tools/make_train_step_bits.py, recorded on the parent commit)."""
import numpy as np
import pytest

from tests import train_step_cases as C
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


def _compare(golden, name, run, records):
    names, sha, head = C.reduce(records)
    key = f"{name}/{run}/"
    assert names == str(golden[key + "names"]), "the recorded tensors changed"
    bad = [n for n, a, b in zip(records, sha, golden[key + "sha256"]) if not np.array_equal(a, b)]
    print(key, len(records), "tensors,", len(bad), "differ")
    assert not bad, (key, len(bad), bad[:8])
    np.testing.assert_array_equal(head, golden[key + "head"])


def test_the_fixture_holds_every_case_and_run(golden):
    want = {f"{name}/{run}/{part}" for name, (_, _, runs) in C.CASES.items() for run in runs for part in ("names", "sha256", "head")}
    assert set(golden.files) == want | {"parent_commit"}


@pytest.mark.parametrize("plan", [True, False], ids=["plan", "noplan"])
@pytest.mark.parametrize("name", list(C.CASES))
def test_fp32_steps_keep_the_parents_bits(vh, golden, name, plan):
    """Heat-maps, loss, all gradients (through the arena) and every BatchNorm buffer of two steps, the second after every parameter moved: its packed
    filters refreshed by the plan's one launch, or each by its own."""
    one, two = C.run(vh, name, dev(), plan=plan)
    if plan:
        _compare(golden, name, "step1", one)
    _compare(golden, name, "step2", two)


def test_unfused_batchnorm_backward_keeps_the_parents_bits(vh, golden):
    """_FUSE_BN_BWD off: every layer takes the stand-alone BatchNorm backward, every data gradient the plain entry."""
    name = next(n for n, (_, _, runs) in C.CASES.items() if "step1_unfused" in runs)
    _compare(golden, name, "step1_unfused", C.run(vh, name, dev(), fuse=False, steps=1)[0])
