"""Writes tests/golden/train_tape_parent_bits.npz: the bits the PARENT commit gives for the cases of tests/train_tape_cases.py.

    VATL_HIP_LIB=<parent tree>/vatl4pose-wacv2024_amd/vatl_hip/libvatl_hip.so python tools/make_train_tape_bits.py <parent commit hash> <parent tree> [out.npz]

Run on the MI355X against a checkout of the commit BEFORE a change to the float64 or bf16 training step (``<parent tree>``: its Python package is
imported, its library loaded through VATL_HIP_LIB), never against the tree's own code: the fixture exists so that a refactor of the two trainers, of their
weight-gradient and glue kernels or of their bindings that moves a bit — a call that moved, another argument, another summation order — shows as a failure
of tests/test_gpu_train_tape_bits.py.  Per shape and run: the names of the recorded tensors, the SHA-256 of each tensor's bytes and its first 64 values as
bit patterns.  The cases and the oracle data come from THIS tree (tests/train_tape_cases.py, oracle/synth.py).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if not os.environ.get("VATL_HIP_LIB"):
    sys.exit("make_train_tape_bits: set VATL_HIP_LIB to the parent commit's libvatl_hip.so (see the docstring)")
if len(sys.argv) < 3:
    sys.exit(__doc__)
sys.path[:0] = [os.path.join(os.path.abspath(sys.argv[2]), "vatl4pose-wacv2024_amd"), ROOT]

import torch  # noqa: E402

import vatl_hip as vh  # noqa: E402
from tests import train_tape_cases as C  # noqa: E402


def main():
    assert os.path.abspath(vh.__file__).startswith(os.path.abspath(sys.argv[2])), vh.__file__
    dev = torch.device("cuda:0")
    out = {"parent_commit": np.array(sys.argv[1])}
    for shape in C.SHAPES:
        for run, records in C.runs(vh, shape, dev).items():
            names, sha, head = C.reduce(records)
            key = f"{C.shape_id(shape)}/{run}/"
            out[key + "names"], out[key + "sha256"], out[key + "head"] = np.array(names), sha, head
            print(key, len(records), "tensors", bytes(sha[0]).hex()[:16], flush=True)
    path = sys.argv[3] if len(sys.argv) > 3 else C.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
