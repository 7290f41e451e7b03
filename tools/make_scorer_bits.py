"""Writes a bit fixture under tests/golden/: the bits the PARENT commit's library gives for the cases of a cases module.

    VATL_HIP_LIB=/path/to/parent/libvatl_hip.so python tools/make_scorer_bits.py <parent commit hash> [out.npz] [--cases tests.glue_cases]

A cases module has ``CASES`` (name -> case), ``GOLDEN`` (the fixture's path) and ``run(vatl_hip, name) -> {key: bits}``.  There are four:
  tests.scorer_cases (the default)  tests/golden/scorer_bits.npz   csrc/decode.hip, localpeak.hip, heatmap_criteria.hip, pose_feature.hip, scorer_common.h
  tests.glue_cases                  tests/golden/glue_bits.npz     csrc/layout.hip, pool.hip, fusion.hip, pack.hip (bn_fold), bn_train.hip, glue_common.h
  tests.wino43_cases                tests/golden/wino43_bits.npz   csrc/winograd_deconv43.hip, winograd_s2_43.hip, winograd43.h, winograd_stage.h, tile_order.h, conv_winograd.hip (launcher)
  tests.train_epilogue_cases        tests/golden/train_epilogue_bits.npz  csrc/bn_epilogue.h and the training write-outs of conv_igemm.h, conv_winograd.hip, winograd_f4.hip

Run on the MI355X against a library built from the commit BEFORE a change to those kernels, never against the tree's own library: the
fixture exists so that a change of their arithmetic — a compiler upgrade, an edit — shows as a failure of tests/test_gpu_scorer_bits.py.
The parent library can be cross-compiled on a host without a GPU (git worktree add ../parent <hash>; python ../parent/vatl4pose-wacv2024_amd/build.py)
and carried to the GPU box.  The hash is stored as given (`parent_commit`): the tool cannot tell which commit a library was built from, so it is
the word of whoever ran it, as in make_optim_bits.py.  Outputs only: float32 / float64 as uint32 / uint64 bit patterns, masks as packed bits, integers raw.
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vatl4pose-wacv2024_amd")]

argv = sys.argv[1:]
module = "tests.scorer_cases"
if "--cases" in argv:
    k = argv.index("--cases")
    module = argv[k + 1]
    del argv[k:k + 2]
if not os.environ.get("VATL_HIP_LIB"):
    sys.exit("make_scorer_bits: set VATL_HIP_LIB to the parent commit's libvatl_hip.so (see the docstring)")
if not argv:
    sys.exit(__doc__)

import vatl_hip as vh  # noqa: E402

cases = importlib.import_module(module)


def main():
    out = {"parent_commit": np.array(argv[0])}
    for name in cases.CASES:
        got = cases.run(vh, name)
        out.update(got)
        print(name, {k.rsplit(".", 1)[1]: (v.dtype.name, v.shape) for k, v in got.items()})
    path = argv[1] if len(argv) > 1 else cases.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(cases.CASES), "cases of", module, "library", vh.LIB_PATH)


if __name__ == "__main__":
    main()
