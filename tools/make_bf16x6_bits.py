"""Writes tests/golden/bf16x6_parent_bits.npz: the bits the PARENT commit's library gives for the cases BITS of tests/bf16x6_pipe_cases.py.

    VATL_HIP_LIB=/path/to/parent/libvatl_hip.so python tools/make_bf16x6_bits.py <parent commit hash> [out.npz]

Run on the MI355X against a library built from the commit BEFORE a change to csrc/gemm1x1_bf16x6.hip (tools/ab_build.sh leaves it as
vatl_hip/libvatl_hip_base.so), never against the tree's own library: the fixture exists so that a change of the kernel's schedule that moves a bit — a
product paired with the wrong stage, another accumulation order, another epilogue expression — shows as a failure of
tests/test_gpu_gemm1x1_bf16x6_pipe.py.  Per case, on seeded normal data: the SHA-256 of the output's bytes and its first 64 values as uint32 bit patterns.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vatl4pose-wacv2024_amd")]

if not os.environ.get("VATL_HIP_LIB"):
    sys.exit("make_bf16x6_bits: set VATL_HIP_LIB to the parent commit's libvatl_hip.so (see the docstring)")
if len(sys.argv) < 2:
    sys.exit(__doc__)

import torch  # noqa: E402

import vatl_hip as vh  # noqa: E402
from tests.bf16x6_pipe_cases import BITS, GOLDEN, case_id, digest, inputs, run  # noqa: E402
from tests.gpu_util import to_dev  # noqa: E402


def main():
    out = {"parent_commit": np.array(sys.argv[1])}
    for c in BITS:
        y = run(vh, c, inputs(c, integers=False), to_dev)
        torch.cuda.synchronize()
        y = y.cpu().numpy()
        out[case_id(c) + "_sha256"] = digest(y)
        out[case_id(c) + "_head"] = y.reshape(-1)[:64].view(np.uint32).copy()
        print(case_id(c), y.shape, bytes(out[case_id(c) + "_sha256"]).hex()[:16])
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
