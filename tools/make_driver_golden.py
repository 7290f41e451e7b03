#!/usr/bin/env python3
"""Generate tests/golden/driver_namespace.json by running the REFERENCE's own driver set-up (build container only).

Usage:  python tools/make_driver_golden.py [--ref /root/reference] [--out tests/golden/driver_namespace.json]

For every case below the reference's ``scripts/Run_active_learning.py`` is run as far as the constructor needs it:
``parse_args`` -> ``setup_opt`` -> ``update_config`` -> ``set_dir`` in a scratch working directory that holds a copy of
the reference's ``configs/`` (the yaml files, and the JRDB scene lists the constructor reads relative to the working
directory).  Then the reference's ``ActiveLearning`` is constructed with ``builder.build_dataset`` replaced by a
function that records the config it is handed and stops the constructor, and the reference's ``initialize_AE`` runs on a
stand-in object with ``Wholebody`` and ``torch.load`` replaced so that the checkpoint path is recorded.

The import shims are those of tools/make_golden.py, plus an attribute fall-back for ``cv2`` and empty modules for the
third-party packages the driver imports but never reaches before ``build_dataset`` (skimage, cachetools, optuna,
seaborn, umap, alipy, annoy).  The fixture holds data only (argv, the option namespace, the config before and after the
derivation, the derived paths, the auto-encoder path, the JRDB lines read); output is deterministic.
"""
from __future__ import annotations

import argparse
import builtins
import copy
import importlib.util
import json
import os
import re
import shutil
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

POSETRACK = "configs/posetrack21/al_simple_posetrack.yaml"
JRDB = "configs/jrdb-pose/al_simple_jrdb.yaml"
SH_LINE = ["--uncertainty", "THC+WPU", "--representativeness", "None", "--filter", "Coreset", "--memo", "WACV_without_transfer",
           "--seedfix", "--continual"]                  # scripts/run_active_learning.sh
CASES = {
    "a_posetrack": ["--cfg", POSETRACK, "--video_id", "000342", *SH_LINE],
    "b_posetrack_optimize": ["--cfg", POSETRACK, "--video_id", "000342", *SH_LINE, "--optimize"],
    "c_posetrack_pcit": ["--cfg", POSETRACK, "--video_id", "000342", *SH_LINE, "--PCIT"],
    "d_jrdb": ["--cfg", JRDB, "--video_id", "00", *SH_LINE],
    "e_jrdb_optimize": ["--cfg", JRDB, "--video_id", "00", *SH_LINE, "--optimize"],
    "f_posetrack_influence_weighted": ["--cfg", POSETRACK, "--video_id", "000522", "--uncertainty", "None", "--representativeness", "Influence",
                                       "--filter", "weighted", "--seedfix", "--continual"],
}
TIMESTAMP = re.compile(r"\d{4}-\d{2}-\d{2}_\d{2}-\d{2}-\d{2}")


class _Stop(Exception):
    pass


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def install_shims():
    shims = _load_by_path("make_golden", os.path.join(HERE, "make_golden.py"))
    edict = shims.install_shims()
    sys.modules["cv2"].__getattr__ = lambda name: 0          # constants of the plotting helpers (never called here)

    class _Placeholder:
        def __init__(self, *a, **k):
            pass

        def __call__(self, *a, **k):
            return self

    def empty(name):
        m = types.ModuleType(name)
        m.__getattr__ = lambda attr: (_ for _ in ()).throw(AttributeError(attr)) if attr.startswith("__") else _Placeholder
        sys.modules[name] = m
        return m
    for name in ("skimage", "skimage.feature", "cachetools", "optuna", "seaborn", "umap", "alipy", "alipy.experiment", "alipy.index", "annoy"):
        empty(name)
    return edict


def plain(x):
    """EasyDict / namespace values -> JSON data."""
    if isinstance(x, dict):
        return {str(k): plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    return str(x)


def run_case(ref, argv, driver, almod, torch):
    """-> the fixture entry of one argv, run inside the current (scratch) working directory."""
    sys.argv = ["scripts/Run_active_learning.py", *argv]
    opt = driver.setup_opt(driver.parse_args())
    cfg = driver.update_config(opt.cfg)
    opt = driver.set_dir(cfg, opt)
    cfg_before = plain(copy.deepcopy(cfg))

    captured, opened = {}, []
    real_open, real_build = builtins.open, almod.builder.build_dataset

    def recording_open(file, *a, **k):
        opened.append(str(file))
        return real_open(file, *a, **k)

    def capture(dataset_cfg, **kw):
        captured["cfg"] = copy.deepcopy(cfg)
        raise _Stop
    builtins.open, almod.builder.build_dataset = recording_open, capture
    try:
        almod.ActiveLearning(cfg, opt)
    except _Stop:
        pass
    finally:
        builtins.open, almod.builder.build_dataset = real_open, real_build
    assert "cfg" in captured, "the reference constructor did not reach build_dataset"
    derived = captured["cfg"]

    # initialize_AE (ActiveLearning.py:886-903) on a stand-in: the checkpoint path it asks torch.load for
    stand_in = types.SimpleNamespace(cfg=derived, opt=opt, dataset=derived.DATASET.EVAL.TYPE, video_id=opt.video_id)
    ae_path, real_load, real_wb = [], torch.load, almod.Wholebody

    def record_load(path, *a, **k):
        ae_path.append(str(path))
        raise _Stop
    torch.load, almod.Wholebody = record_load, (lambda *a, **k: None)
    try:
        almod.ActiveLearning.initialize_AE(stand_in)
    except _Stop:
        pass
    finally:
        torch.load, almod.Wholebody = real_load, real_wb
    assert len(ae_path) == 1

    jrdb = {}
    for path in opened:
        if path.endswith(".txt"):
            with real_open(path) as f:
                jrdb[path] = f.readlines()
    o = {k: plain(v) for k, v in vars(opt).items()}
    o["work_dir"] = TIMESTAMP.sub("<timestamp>", o["work_dir"])
    return {"argv": list(argv), "opt": o, "cfg_before": cfg_before, "cfg_after": plain(derived),
            "derived": {split: {k: derived.DATASET[split][k] for k in ("ROOT", "IMG_PREFIX", "ANN")} for split in ("EVAL", "TRAIN")},
            "ae_path": ae_path[0], "jrdb_lines": jrdb}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "driver_namespace.json"))
    a = ap.parse_args()
    ref = os.path.abspath(a.ref)
    out = os.path.abspath(a.out)
    install_shims()
    sys.path.insert(0, ref)
    import torch
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):                # the driver's banners
        driver = _load_by_path("Run_active_learning", os.path.join(ref, "scripts", "Run_active_learning.py"))
    almod = sys.modules["active_learning.ActiveLearning"]
    cases = {}
    cwd = os.getcwd()
    for name, argv in CASES.items():
        with tempfile.TemporaryDirectory() as wd:
            shutil.copytree(os.path.join(ref, "configs"), os.path.join(wd, "configs"))
            os.chdir(wd)
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    cases[name] = run_case(ref, argv, driver, almod, torch)
            finally:
                os.chdir(cwd)
    with open(out, "w") as f:
        json.dump({"cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(cases)} cases")


if __name__ == "__main__":
    main()
