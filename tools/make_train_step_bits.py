"""Writes tests/golden/train_step_parent_bits.npz: the bits the PARENT commit gives for the cases of tests/train_step_cases.py.

    VATL_HIP_LIB=<parent tree>/vatl4pose-wacv2024_amd/vatl_hip/libvatl_hip.so python tools/make_train_step_bits.py <parent commit hash> <parent tree> [out.npz]

Run on the MI355X against a checkout of the commit BEFORE a change to the fp32 fine-tune step (``<parent tree>``: its Python package is imported, its
library loaded through VATL_HIP_LIB), never against the tree's own code: the fixture exists so that a refactor of alphapose/models/hip_train.py or of
the kernels and bindings under it that moves a bit — a launch that moved, another argument, another order — shows as a failure of
tests/test_gpu_train_step_bits.py.  Per case and run: the names of the recorded tensors, the SHA-256 of each tensor's bytes and its first values as bit
patterns.  Step 2 is recorded with the pack plan; the same step with a launch per re-pack must hash alike on the parent already, which is asserted here.
The cases and the oracle data come from THIS tree (tests/train_step_cases.py, oracle/synth.py).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if not os.environ.get("VATL_HIP_LIB"):
    sys.exit("make_train_step_bits: set VATL_HIP_LIB to the parent commit's libvatl_hip.so (see the docstring)")
if len(sys.argv) < 3:
    sys.exit(__doc__)
sys.path[:0] = [os.path.join(os.path.abspath(sys.argv[2]), "vatl4pose-wacv2024_amd"), ROOT]

import torch  # noqa: E402

import vatl_hip as vh  # noqa: E402
from alphapose.models import hip_train  # noqa: E402
from tests import train_step_cases as C  # noqa: E402


def main():
    parent = os.path.abspath(sys.argv[2])
    assert os.path.abspath(vh.__file__).startswith(parent) and os.path.abspath(hip_train.__file__).startswith(parent), (vh.__file__, hip_train.__file__)
    dev = torch.device("cuda:0")
    out = {"parent_commit": np.array(sys.argv[1])}
    for name, (_, _, runs) in C.CASES.items():
        one, two = C.run(vh, name, dev)
        records = {"step1": one, "step2": two}
        noplan = C.reduce(C.run(vh, name, dev, plan=False)[1])
        assert noplan[0] == C.reduce(two)[0] and np.array_equal(noplan[1], C.reduce(two)[1]), f"{name}: step 2 differs between the plan and per-tensor packs"
        if "step1_unfused" in runs:
            records["step1_unfused"] = C.run(vh, name, dev, fuse=False, steps=1)[0]
        assert tuple(records) == runs
        for run, rec in records.items():
            names, sha, head = C.reduce(rec)
            key = f"{name}/{run}/"
            out[key + "names"], out[key + "sha256"], out[key + "head"] = np.array(names), sha, head
            print(key, len(rec), "tensors", bytes(sha[0]).hex()[:16], flush=True)
    path = sys.argv[3] if len(sys.argv) > 3 else C.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
