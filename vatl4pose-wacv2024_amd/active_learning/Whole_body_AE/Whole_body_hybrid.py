"""Pre-training data set of the whole-body auto-encoder (reference: Whole_body_AE/Whole_body_hybrid.py:12-85).

One item per annotated person with at least one visible key-point: the hybrid feature of the pose (``compute_hybrid``, 42 values
for 17 key-points) or, with ``kp_direct``, its 51 raw key-point values.  File derivation, cache location and cache format are the
reference's, so a cache written by either side loads in the other:

    data/<PoseTrack21|JRDB2022>/activelearning/hybrid_feature/<mode>/<json_name>.npy     pickled object array of {"ann_id", "feature"}

The hybrid features of a whole file come from ONE ``vatl_hybrid_feature_f64`` launch and are copied to the host; the items are host
data, so ``DataLoader`` workers never touch the device.  ``kp_direct=True`` needs no device at all.

Deviation: the reference creates its item dict once, outside the loop over the annotations, so every element
of the list it builds (and caches) is the LAST kept annotation.  This class builds one dict per annotation, which is what the code
plainly intends and what ``retrain_AE`` here already does.  A cache file the reference wrote is loaded as it is.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch
from torch.utils.data import Dataset

_ID_DIGITS = {"PoseTrack21": 2, "JRDB2022": 3}          # ann_id = last digits of `id`, followed by `image_id`


def annotation_file(mode: str, retrain_video_id=None, dataset_type: str = "Posetrack21", data_root: str = "data"):
    """(cache directory name, json name, json path or None) as the reference derives them.  A PoseTrack21 ``retrain_video_id`` names a
    file only for the modes ``val`` and ``train_val`` (the reference sets no path for any other mode)."""
    if dataset_type == "Posetrack21":
        root = os.path.join(data_root, "PoseTrack21", "activelearning")
        if retrain_video_id is None:
            name = f"000000_integrated_{mode}.json"
        else:
            name = {"val": f"{retrain_video_id}_mpii_test.json", "train_val": f"{retrain_video_id}_bonn_train.json"}.get(mode)
        return "PoseTrack21", name, (os.path.join(root, mode, name) if name else None)
    if dataset_type == "JRDB2022":
        root = os.path.join(data_root, "jrdb-pose", "activelearning")
        name = f"{retrain_video_id}_jrdb-pose.json" if retrain_video_id is not None else f"integrated_{mode}.json"
        return "JRDB2022", name, os.path.join(root, mode, name)
    raise ValueError(f"dataset_type must be Posetrack21 or JRDB2022, not {dataset_type!r}")


class Wholebody(Dataset):
    """``Wholebody(mode, kp_direct=False, retrain_video_id=None, dataset_type="Posetrack21")`` like the reference, plus
    ``data_root`` (the reference reads ``data/`` under the working directory) and ``feature_dim`` (None keeps the whole vector;
    an integer keeps its leading values, as ``retrain_AE`` does for a 38-wide module).  See the module docstring for the one
    deliberate deviation: one dict per annotation, not one dict aliased by every element."""

    def __init__(self, mode: str, kp_direct=False, retrain_video_id=None, dataset_type="Posetrack21", data_root="data", feature_dim=None) -> None:
        super().__init__()
        self.mode = mode
        self.eval_joints = [0, 1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
        self.retrain_video_id = retrain_video_id
        self.feature_dim = feature_dim
        cache_type, json_name, self.file = annotation_file(mode, retrain_video_id, dataset_type, data_root)
        if json_name is None:
            raise ValueError(f"PoseTrack21 with retrain_video_id has files for the modes 'val' and 'train_val' only, not {mode!r}")
        self.cache = os.path.join(data_root, cache_type, "activelearning", "hybrid_feature", mode, f"{json_name}.npy")
        if os.path.isfile(self.cache):
            self.items = list(np.load(self.cache, allow_pickle=True))
            print(f"loaded {len(self.items)} human body from {self.cache}")
        else:
            self.items = self._from_annotations(cache_type, bool(kp_direct))
            os.makedirs(os.path.dirname(self.cache), exist_ok=True)
            np.save(self.cache, self.items)
            print(f"saved {len(self.items)} hybrid feature calculated from {self.file}")
        self.num = len(self.items)

    def _from_annotations(self, cache_type: str, kp_direct: bool):
        with open(self.file, "r") as f:
            anns = [a for a in json.load(f)["annotations"] if sum(a["keypoints"][2::3]) != 0]      # at least one visible key-point
        digits = _ID_DIGITS[cache_type]
        ids = [int(str(int(a["id"]))[-digits:] + str(a["image_id"])) for a in anns]
        if kp_direct or not anns:
            feats = [a["keypoints"] for a in anns]
        else:
            from .hybrid_feature import compute_hybrid_batch
            if not torch.cuda.is_available():
                import vatl_hip as vh
                raise vh.VatlError("Wholebody computes hybrid features on MI355X only (no CPU fallback); kp_direct=True needs no device")
            feat, status = compute_hybrid_batch([a["bbox"] for a in anns], [a["keypoints"] for a in anns])
            status = status.cpu().numpy()
            assert not (status == 1).any(), "height of human body must be positive!"
            assert not (status == 2).any(), "at least one visible keypoint is required!"
            feats = list(feat.cpu().numpy())
        items = [{"ann_id": i, "feature": f} for i, f in zip(ids, feats)]
        return sorted(items, key=lambda x: x["ann_id"])

    def features(self) -> torch.Tensor:
        """All items as one (len, width) float32 CPU tensor — what the device-resident trainer uploads once."""
        rows = np.asarray([np.asarray(it["feature"], np.float64) for it in self.items], np.float64).reshape(len(self.items), -1)
        if self.feature_dim is not None:
            rows = rows[:, :self.feature_dim]
        return torch.from_numpy(rows.astype(np.float32))

    def __getitem__(self, index: int) -> torch.Tensor:
        feat = self.items[index]["feature"]
        if self.feature_dim is not None:
            feat = feat[:self.feature_dim]
        return torch.tensor(feat, dtype=torch.float32)

    def __len__(self) -> int:
        return self.num
