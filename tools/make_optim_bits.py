"""Writes tests/golden/optim_bits.npz: the bits the PARENT commit's library gives for the cases of tests/optim_cases.py.

    VATL_HIP_LIB=/path/to/parent/libvatl_hip.so python tools/make_optim_bits.py <parent commit hash> [out.npz]

Run on the MI355X against a library built from the commit BEFORE a change to csrc/optim.hip (git worktree add ../parent <hash>;
python ../parent/vatl4pose-wacv2024_amd/build.py), never against the tree's own library: the fixture exists so that a change of the
optimisers' arithmetic — a compiler upgrade, an edit — shows as a failure of tests/test_gpu_optim.py.  Each kind runs through its
per-tensor entry on 16-byte-aligned tensors; p and the state buffers after step 3 are stored as uint32 bit patterns.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vatl4pose-wacv2024_amd")]

if not os.environ.get("VATL_HIP_LIB"):
    sys.exit("make_optim_bits: set VATL_HIP_LIB to the parent commit's libvatl_hip.so (see the docstring)")
if len(sys.argv) < 2:
    sys.exit(__doc__)

import torch  # noqa: E402

import vatl_hip as vh  # noqa: E402
from tests.optim_cases import CASES, GOLDEN, bits, inputs, run  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    out = {"parent_commit": np.array(sys.argv[1])}
    for kind, (_, names, _) in CASES.items():
        p0, gs = inputs(kind)
        p = torch.from_numpy(p0).to(dev)
        bufs = [torch.zeros_like(p) for _ in names]
        run(vh, kind, p, [torch.from_numpy(g).to(dev) for g in gs], bufs)
        torch.cuda.synchronize()
        out[kind + "_p"] = bits(p)
        for name, b in zip(names, bufs):
            out[f"{kind}_{name}"] = bits(b)
        print(kind, {k: hex(int(v[-1])) for k, v in out.items() if k.startswith(kind + "_")})
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
