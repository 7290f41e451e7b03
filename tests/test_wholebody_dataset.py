"""The pre-training data set of the whole-body auto-encoder (active_learning/Whole_body_AE/Whole_body_hybrid.py) on the host:
file derivation, skip / ann_id / sort rules, cache location and format against tests/golden/wholebody.npz (tests/golden/wholebody.md).
``kp_direct=True`` needs no device; the hybrid features are checked in tests/test_gpu_ae_pretrain.py."""
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wholebody.npz")
DIGITS = {"Posetrack21": 2, "JRDB2022": 3}
# (dataset_type, mode, retrain_video_id) -> (json path under data_root, cache path under data_root): the reference's derivation
FILES = {
    ("Posetrack21", "train", None): ("PoseTrack21/activelearning/train/000000_integrated_train.json",
                                     "PoseTrack21/activelearning/hybrid_feature/train/000000_integrated_train.json.npy"),
    ("Posetrack21", "train_val", None): ("PoseTrack21/activelearning/train_val/000000_integrated_train_val.json",
                                         "PoseTrack21/activelearning/hybrid_feature/train_val/000000_integrated_train_val.json.npy"),
    ("Posetrack21", "val", "000342"): ("PoseTrack21/activelearning/val/000342_mpii_test.json",
                                       "PoseTrack21/activelearning/hybrid_feature/val/000342_mpii_test.json.npy"),
    ("Posetrack21", "train_val", "001001"): ("PoseTrack21/activelearning/train_val/001001_bonn_train.json",
                                             "PoseTrack21/activelearning/hybrid_feature/train_val/001001_bonn_train.json.npy"),
    ("JRDB2022", "train", None): ("jrdb-pose/activelearning/train/integrated_train.json",
                                  "JRDB2022/activelearning/hybrid_feature/train/integrated_train.json.npy"),
    ("JRDB2022", "val", 3): ("jrdb-pose/activelearning/val/3_jrdb-pose.json",
                             "JRDB2022/activelearning/hybrid_feature/val/3_jrdb-pose.json.npy"),
}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def annotations(g, dtype):
    return [{"id": int(i), "image_id": int(m), "bbox": b.tolist(), "keypoints": k.tolist()}
            for i, m, b, k in zip(g[f"{dtype}_id"], g[f"{dtype}_image_id"], g[f"{dtype}_bbox"], g[f"{dtype}_keypoints"])]


def ann_id(a, dtype):
    return int(str(int(a["id"]))[-DIGITS[dtype]:] + str(a["image_id"]))


def kept(anns):
    return [a for a in anns if sum(a["keypoints"][2::3]) != 0]


def write_json(root, rel, anns):
    path = os.path.join(root, rel)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"annotations": anns}, f)
    return path


def test_package_exports_the_references_names():
    import active_learning.Whole_body_AE as pkg
    from active_learning.Whole_body_AE import WholeBodyAE, Wholebody
    assert pkg.__all__ == ["WholeBodyAE", "Wholebody"]
    assert pkg.WholeBodyAE is WholeBodyAE and pkg.Wholebody is Wholebody
    assert issubclass(Wholebody, torch.utils.data.Dataset)


def test_fixture_has_the_cases_it_promises(golden):
    for dtype in DIGITS:
        anns = annotations(golden, dtype)
        k = kept(anns)
        assert len(anns) == 40 and 0 < len(k) < len(anns)                                  # people without a visible key-point
        ids = [ann_id(a, dtype) for a in k]
        assert ids != sorted(ids) and len(set(ids)) == len(ids)                            # file order is not ann_id order
        tails = [str(a["id"])[-DIGITS[dtype]:] for a in anns]
        assert len(set(tails)) < len(tails)                                                # two people share the kept digits
        assert int(golden[f"{dtype}_ref_len"]) == len(k) and bool(golden[f"{dtype}_ref_item0_is_last_kept"])


@pytest.mark.parametrize("dtype,mode,vid", list(FILES))
def test_kp_direct_items_cache_and_reload(golden, tmp_path, dtype, mode, vid):
    from active_learning.Whole_body_AE import Wholebody
    root = str(tmp_path / "data")
    rel_json, rel_cache = FILES[(dtype, mode, vid)]
    anns = annotations(golden, dtype)
    path = write_json(root, rel_json, anns)
    ds = Wholebody(mode, kp_direct=True, retrain_video_id=vid, dataset_type=dtype, data_root=root)
    assert os.path.normpath(ds.file) == os.path.normpath(path)
    assert len(ds) == int(golden[f"{dtype}_ref_len"])
    want = sorted(kept(anns), key=lambda a: ann_id(a, dtype))
    assert [it["ann_id"] for it in ds.items] == [ann_id(a, dtype) for a in want]
    for i, a in enumerate(want):
        item = ds[i]
        assert item.dtype == torch.float32 and item.device.type == "cpu" and item.shape == (51,)
        assert torch.equal(item, torch.tensor(a["keypoints"], dtype=torch.float32))
    cache = os.path.join(root, rel_cache)
    assert os.path.isfile(cache)
    stored = np.load(cache, allow_pickle=True)
    assert stored.dtype == object and stored.shape == (len(want),) and set(stored[0]) == {"ann_id", "feature"}
    os.remove(path)                                                                        # the second construction can only read the cache
    again = Wholebody(mode, kp_direct=True, retrain_video_id=vid, dataset_type=dtype, data_root=root)
    assert len(again) == len(ds)
    assert all(torch.equal(again[i], ds[i]) for i in range(len(ds)))
    assert torch.equal(again.features(), torch.stack([ds[i] for i in range(len(ds))]))
    assert torch.equal(Wholebody(mode, kp_direct=True, retrain_video_id=vid, dataset_type=dtype, data_root=root, feature_dim=38)[1], ds[1][:38])


@pytest.mark.parametrize("dtype", list(DIGITS))
def test_a_cache_in_the_references_aliased_format_loads_as_it_is(golden, tmp_path, dtype):
    """What the reference's np.save leaves behind: an object array whose elements are ONE dict.  It is loaded, not repaired."""
    from active_learning.Whole_body_AE import Wholebody
    root = str(tmp_path / "data")
    _, rel_cache = FILES[(dtype, "train", None)]
    n = int(golden[f"{dtype}_ref_len"])
    item = {"ann_id": 7, "feature": golden[f"{dtype}_ref_item0_direct"].astype(np.float64).tolist()}
    os.makedirs(os.path.dirname(os.path.join(root, rel_cache)))
    np.save(os.path.join(root, rel_cache), [item] * n)
    ds = Wholebody("train", kp_direct=True, dataset_type=dtype, data_root=root)            # no json exists: only the cache can serve
    assert len(ds) == n
    for i in (0, n // 2, n - 1):
        assert torch.equal(ds[i], torch.from_numpy(golden[f"{dtype}_ref_item0_direct"]))


@pytest.mark.parametrize("dtype", list(DIGITS))
def test_aliasing_deviation_is_pinned(golden, tmp_path, dtype):
    """The reference's element 0 (every element, through its aliased dict) is the person that comes LAST in file order among the kept
    ones; here that person sits at its ann_id rank and element 0 is the smallest ann_id."""
    from active_learning.Whole_body_AE import Wholebody
    root = str(tmp_path / "data")
    anns = annotations(golden, dtype)
    write_json(root, FILES[(dtype, "train", None)][0], anns)
    ds = Wholebody("train", kp_direct=True, dataset_type=dtype, data_root=root)
    last = kept(anns)[-1]
    ref0 = torch.from_numpy(golden[f"{dtype}_ref_item0_direct"])
    assert torch.equal(torch.tensor(last["keypoints"], dtype=torch.float32), ref0)
    rank = sorted(ann_id(a, dtype) for a in kept(anns)).index(ann_id(last, dtype))
    assert rank != 0 and torch.equal(ds[rank], ref0) and not torch.equal(ds[0], ref0)


def test_unknown_dataset_type_and_mode_are_refused(tmp_path):
    from active_learning.Whole_body_AE import Wholebody
    with pytest.raises(ValueError):
        Wholebody("train", kp_direct=True, dataset_type="COCO", data_root=str(tmp_path))
    with pytest.raises(ValueError):
        Wholebody("train", kp_direct=True, retrain_video_id="000342", dataset_type="Posetrack21", data_root=str(tmp_path))


def test_trainer_keeps_the_scripts_schedule_and_stopping_rule():
    from active_learning.Whole_body_AE import pretrain
    assert [pretrain.learning_rate(e) for e in (0, 11, 12, 39, 40, 79)] == [1e-3, 1e-3, 2e-4, 2e-4, 5e-5, 5e-5]
    assert (pretrain.TRAIN_BATCH, pretrain.VALID_BATCH, pretrain.WEIGHT_DECAY, pretrain.PATIENCE) == (10000, 8000, 0.01, 30)
    stop = pretrain.EarlyStopping(patience=3)
    assert [stop(v) for v in (5.0, 4.0, 4.0, 4.5, 3.9, 4.0, 4.0, 4.0)] == [False, False, False, False, False, False, False, True]
    opt = pretrain.parse_args(["--dataset_type", "JRDB2022", "--z", "4", "--kp_direct", "--input_dim", "38"])
    assert (opt.z, opt.epoch, opt.pretrained, opt.kp_direct, opt.dataset_type, opt.input_dim) == (4, 80, False, True, "JRDB2022", 38)
