"""What the unchanged driver (scripts/Run_active_learning.py) leaves for the constructor to work out: the annotation file and
frame folder of ``opt.video_id`` (reference: active_learning/ActiveLearning.py:55, 67-94) and the WPU auto-encoder checkpoint
(:886-903).  Host code only, resolved once per construction; importable without a GPU.

Deviations from the reference, all in favour of callers that build their own configs:

* an explicit ``DATASET.EVAL.ANN`` that this rule could not have produced is kept (the reference overwrites it);
* a dataset type the rule does not know (``FrameVideo``, ``SyntheticVideo``, ...) leaves the config untouched (the reference
  raises ``UnboundLocalError``);
* a config with neither ``AE.PRETRAINED`` nor ``AE.PRETRAINED_ROOT`` starts the auto-encoder from random weights;
* the auto-encoder's input width is read from the checkpoint (38, 42 or 51: SURVEY.md §9 item 1), not assumed.
"""
from __future__ import annotations

import os
import re

JRDB_LISTS = {True: os.path.join("configs", "jrdb-pose", "jrdb_val.txt"), False: os.path.join("configs", "jrdb-pose", "jrdb_test.txt")}

# every annotation path the rule below produces, whatever the video id: a config that still holds one of these was derived
# for an earlier video (the --optimize loop constructs one object per video on the same config) and is derived again
_DERIVED_ANN = re.compile(r"^(activelearning/train_val/[^/]+_bonn_train\.json|activelearning/val/[^/]+_mpii_test\.json|"
                          r"annotations/eval/[^/]+\.json|activelearning/(val|test)/[^/]+_jrdb-pose\.json)$")


def _jrdb_scene(vid, optimize: bool) -> str:
    """Line ``int(vid)`` of the JRDB scene list, read relative to the working directory like the reference; ``readlines()``
    keeps the trailing newline (``IMG_PREFIX`` is not used by the video loaders, which join ``ROOT`` and ``file_name``)."""
    path = JRDB_LISTS[bool(optimize)]
    try:
        with open(path, "r") as f:
            lines = f.readlines()
    except FileNotFoundError as e:
        raise FileNotFoundError(f"JRDB scene list {path} (relative to {os.getcwd()}) is missing: the driver runs from the "
                                f"project root, where configs/jrdb-pose/ holds it") from e
    return lines[int(vid)]


def video_paths(dataset_type: str, opt) -> tuple[str, str] | None:
    """(IMG_PREFIX, ANN) of ``opt.video_id`` in the reference's branch order, or None for a type without a rule."""
    pcit = bool(getattr(opt, "PCIT", False))
    if dataset_type not in ("Posetrack21", "JRDB2022") and not pcit:
        return None
    vid = getattr(opt, "video_id", None)
    if vid is None:
        raise ValueError(f"a {dataset_type} config without DATASET.EVAL.ANN needs opt.video_id (the driver's --video_id)")
    optimize = bool(getattr(opt, "optimize", False))
    if dataset_type == "Posetrack21":
        if optimize:
            return f"images/train/{vid}_bonn_train/", f"activelearning/train_val/{vid}_bonn_train.json"
        return f"images/val/{vid}_mpii_test/", f"activelearning/val/{vid}_mpii_test.json"
    if pcit:                                         # second: a Posetrack21 config with --PCIT takes the branch above (ROOT data/PCIT/)
        return f"images/{vid}_PCIT_eval/", f"annotations/eval/{vid}.json"
    if dataset_type == "JRDB2022":
        scene = _jrdb_scene(vid, optimize)
        split = "val" if optimize else "test"
        return f"images/image_stitched/{scene}/", f"activelearning/{split}/{vid}_jrdb-pose.json"
    return None


def derive_video_paths(cfg, opt) -> dict:
    """Set ``cfg.DATASET.{EVAL,TRAIN}.{IMG_PREFIX,ANN}`` for ``opt.video_id`` when the config leaves them to the constructor
    (``EVAL.ANN`` empty, or a path this rule made for another video).  Returns what was set ({} when nothing was)."""
    ev = cfg.DATASET.EVAL
    ann = str(ev.get("ANN", "") or "")
    if ann and not _DERIVED_ANN.match(ann):
        return {}
    paths = video_paths(ev.TYPE, opt)
    if paths is None:
        return {}
    prefix, ann = paths
    for split in ("EVAL", "TRAIN"):
        if split in cfg.DATASET:
            cfg.DATASET[split].IMG_PREFIX = prefix
            cfg.DATASET[split].ANN = ann
    return {"IMG_PREFIX": prefix, "ANN": ann}


def resolve_ae_checkpoint(cfg) -> str | None:
    """The WPU auto-encoder checkpoint a config asks for: a non-empty ``AE.PRETRAINED``, else
    ``<AE.PRETRAINED_ROOT>/Hybrid/WholeBodyAE_zdim<Z_DIM>.pth`` (ActiveLearning.py:895), else None (random initialisation).
    A checkpoint asked for through ``PRETRAINED_ROOT`` must exist: there is no silent fall-back to random weights."""
    ae = cfg.get("AE", None) or {}
    explicit = ae.get("PRETRAINED", "")
    if explicit:
        return str(explicit)
    if "PRETRAINED_ROOT" not in ae:
        return None
    path = os.path.join(ae["PRETRAINED_ROOT"], "Hybrid", f"WholeBodyAE_zdim{ae['Z_DIM']}.pth")
    if not os.path.isfile(path):
        raise FileNotFoundError(f"WPU auto-encoder checkpoint {path} (from AE.PRETRAINED_ROOT = {ae['PRETRAINED_ROOT']!r}, relative to "
                                f"{os.getcwd()}) does not exist; set AE.PRETRAINED to another file, or remove AE.PRETRAINED_ROOT for a random start")
    return path


def load_ae_checkpoint(path: str, cfg) -> tuple[dict, int, int]:
    """(CPU state dict, input_dim, z_dim) of an auto-encoder checkpoint.  The input width is the checkpoint's
    (``encoder.0.weight`` columns); ``AE.Z_DIM`` and an ``AE.INPUT_DIM`` the config sets must agree with it."""
    import torch
    sd = torch.load(path, map_location="cpu")
    try:
        input_dim, z_dim = int(sd["encoder.0.weight"].shape[1]), int(sd["encoder.6.weight"].shape[0])
    except (KeyError, TypeError, AttributeError, IndexError) as e:
        raise ValueError(f"{path} is not a WholeBodyAE state dict (encoder.0.weight / encoder.6.weight)") from e
    if z_dim != int(cfg.AE.Z_DIM):
        raise ValueError(f"{path} has z_dim {z_dim}, the config's AE.Z_DIM is {cfg.AE.Z_DIM}")
    want = cfg.AE.get("INPUT_DIM", None)
    if want is not None and int(want) != input_dim:
        raise ValueError(f"{path} has input_dim {input_dim}, the config's AE.INPUT_DIM is {want}")
    return sd, input_dim, z_dim
