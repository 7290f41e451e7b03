"""PoseTrack21 / JRDB-Pose video datasets from COCO-format annotation json (reference: alphapose/datasets/custom.py:24-176,
posetrack21.py:12-129, jrdb2022.py).

The annotation semantics are the reference's (``_load_jsons`` / ``_check_load_keypoints``): boxes converted xywh -> xyxy
and clipped to the frame, persons without a positive box / key-points / visible joint dropped, one item per person, items
sorted by ``id`` = last two (PoseTrack) or three (JRDB) digits of the annotation id + image id, ``track_id`` as the reference
builds it.  Only the plumbing differs: the json is indexed with a few dict lookups instead of pycocotools, frames are decoded
on demand — baseline JPEG files by the hybrid decoder (Huffman pass on the host, pixels on the device, ``DECODER``), everything
else with Pillow (the reference uses ``cv2.imread`` + BGR->RGB; both sit on libjpeg) — and the crops / targets of a whole batch
come from the device (``FrameVideo``).
Config keys as in the reference's yaml: ``ROOT``, ``IMG_PREFIX``, ``ANN``, optional ``AUG``; ``PRESET`` is injected by
``builder.build_dataset``.
"""
from __future__ import annotations

import json
import os
from collections import OrderedDict

import numpy as np

from alphapose.models.builder import DATASET
from alphapose.utils.bbox import bbox_clip_xyxy, bbox_xywh_to_xyxy
from alphapose.utils.presets.simple_transform import FrameArena

from .frame_video import FrameVideo


class CocoIndex:
    """The four pycocotools queries the loaders need (getCatIds/loadCats, getImgIds/loadImgs, getAnnIds/loadAnns)."""

    def __init__(self, path):
        with open(path) as f:
            data = json.load(f)
        self.cats = list(data.get("categories", []))
        self.imgs = {im["id"]: im for im in data.get("images", [])}
        self.anns_of = {}
        for a in data.get("annotations", []):
            self.anns_of.setdefault(a["image_id"], []).append(a)

    def category_names(self):
        return [c["name"] for c in self.cats]

    def images_sorted(self):
        return [self.imgs[i] for i in sorted(self.imgs)]


def _read_rgb(path):
    try:
        from PIL import Image
    except ImportError as e:                                     # pragma: no cover
        raise RuntimeError("decoding video frames needs Pillow (the reference uses cv2.imread)") from e
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def _read_coefficients(path):
    """The hybrid decoder's host half, what a decode-ahead worker runs in place of `_read_rgb`: file bytes -> the frame's coefficient
    blocks (`vh.jpeg_entropy_decode`; the pixels are made on the device, a batch at a time, by `cache_frames`).  A file the probe refuses
    (progressive, 4:2:2, PNG, ...) or whose entropy-coded data the decoder rejects goes through Pillow as before.  (The bit-for-bit
    agreement with Pillow holds for intact files.  A damaged file that this decoder happens to get through without an error is cached as
    the pixels it gave; Pillow might have raised on it, or concealed the damage differently.)"""
    import vatl_hip as vh
    try:
        with open(path, "rb") as f:
            data = f.read()
        if vh.jpeg_probe(data).admitted:
            return vh.jpeg_entropy_decode(data)
    except (OSError, vh.VatlError):
        pass                                                     # an unreadable or damaged file: Pillow's verdict is the data set's, as on the host path
    return _read_rgb(path)


def _read_packed(path):
    """The worker's share when the Huffman pass runs on the device too (DECODER = "device-huffman"): file bytes -> the packed scan
    (`vh.jpeg_pack`: markers parsed, byte stuffing removed).  A file that does not pack — refused by the probe, more than 768 KiB between
    restart markers, a restart marker missing — goes the way of `_read_coefficients`, which carries the host decoder's verdict and
    after it Pillow's."""
    import vatl_hip as vh
    try:
        with open(path, "rb") as f:
            data = f.read()
        return vh.jpeg_pack(data)                                # (raises for a stream the probe refuses: the header is parsed here alone)
    except (OSError, vh.VatlError):
        pass
    return _read_coefficients(path)


def frame_loader(dataset):
    """The function that turns one frame path into what `dataset.cache_frames` takes (looked up per call: tests replace `_read_rgb`)."""
    decoder = getattr(dataset, "DECODER", "host")
    return _read_rgb if decoder == "host" else _read_packed if decoder == "device-huffman" else _read_coefficients


class _CocoVideo(FrameVideo):
    CLASSES = ["person"]
    num_joints = 17
    ID_DIGITS = 2                     # digits of the annotation id that lead the sort key (posetrack21.py:103)
    STRICT_BOX = True                 # posetrack21.py:84 drops xmax <= xmin; jrdb2022.py only xmax < xmin
    FRAME_CACHE = 64                  # decoded frames kept (an id-sorted stream revisits a frame for every person in it)
    # Who decodes the frame files.  "host": Pillow, frames cached on the host and uploaded per batch.  "device": baseline 4:4:4 / 4:2:0 /
    # grayscale JPEG files (`vh.jpeg_probe`) are Huffman-decoded on the host and turned into pixels on the device, one
    # `vh.jpeg_decode_batch` call per batch, and cached as device tensors; every other file goes through Pillow.  "auto": the same as
    # "device".  The batches are the same bit for bit; profiles/jpeg_decode_notes.md has the measurement behind the default
    # (1280x720 frames on eight threads: 3.4x the frames/s of the Pillow path, 1.8x the training steps/s).  "device-huffman" (opt-in):
    # the Huffman pass runs on the device as well — the workers only pack the scan (`vh.jpeg_pack`), `vh.jpeg_decode_packed_batch` decodes a
    # batch's frames, and a frame whose stream the device rejects is read again through the "device" path; the batches are the same
    # again (profiles/jpeg_huffman_notes.md).
    DECODER = "auto"

    def __init__(self, train=True, dpg=False, skip_empty=True, lazy_import=False, get_prenext=False, **cfg):
        if dpg:
            raise NotImplementedError("DPG augmentation is broken in the reference itself (simple_transform.py:184-185)")
        self._root, self._img_prefix = cfg["ROOT"], cfg.get("IMG_PREFIX", "")
        self._ann_file = os.path.join(self._root, cfg["ANN"])
        self._skip_empty = skip_empty
        db = CocoIndex(self._ann_file)
        assert db.category_names() == self.CLASSES, "Incompatible category names with " + type(self).__name__
        anns = []
        for count, frame in enumerate(db.images_sorted()):
            path = self._image_path(frame)
            if not os.path.exists(path):
                raise IOError(f"Image: {path} not exists.")
            persons = self._persons(db, frame)
            for person in persons:
                person["frame"] = path
                person["img_id"] = frame.get("image_id", frame["id"])
                person.setdefault("id", len(anns))               # image datasets keep file order
                anns.append(person)
            if persons and self._stop_after(count + 1):          # (the reference checks its image counter only after a labelled image)
                break
        super().__init__(frames=[], annotations=anns, train=train, get_prenext=get_prenext, PRESET=cfg.get("PRESET"), AUG=cfg.get("AUG"))
        self._items = [{"path": a["frame"], "img_id": a["img_id"], "ann_id": a.get("ann_id"), "id": a["id"], "track_id": a.get("track_id"),
                        "keypoint": a.get("keypoint")} for a in self._labels]
        self._decoded = OrderedDict()

    def _image_path(self, frame):
        return os.path.join(self._root, frame["file_name"])      # posetrack21.py:53-54

    def _stop_after(self, n_images):
        return False

    def _track_id(self, frame, obj):
        return str(frame["vid_id"]) + str(obj["track_id"])       # posetrack21.py:105

    def _persons(self, db, frame):
        """``_check_load_keypoints`` (posetrack21.py:77-129)."""
        width, height = int(frame["width"]), int(frame["height"])
        out = []
        for obj in db.anns_of.get(frame["image_id"], db.anns_of.get(frame["id"], [])):
            if "bbox" not in obj:
                continue
            xmin, ymin, xmax, ymax = bbox_clip_xyxy(bbox_xywh_to_xyxy(obj["bbox"]), width, height)
            if (xmax <= xmin or ymax <= ymin) if self.STRICT_BOX else (xmax < xmin or ymax < ymin):
                continue
            if max(obj["keypoints"]) == 0:
                continue
            joints_3d = np.zeros((self.num_joints, 3, 2), dtype=np.float32)
            kp = obj["keypoints"]
            for i in range(self.num_joints):
                joints_3d[i, 0, 0], joints_3d[i, 1, 0] = kp[i * 3 + 0], kp[i * 3 + 1]
                joints_3d[i, :2, 1] = min(1, kp[i * 3 + 2])
            if np.sum(joints_3d[:, 0, 1]) < 1:
                continue
            ann_id = int(obj["id"])
            out.append({"bbox": (float(xmin), float(ymin), float(xmax), float(ymax)), "width": width, "height": height, "joints_3d": joints_3d,
                        "keypoint": list(kp), "id": int(str(ann_id)[-self.ID_DIGITS:] + str(frame["image_id"])), "ann_id": ann_id,
                        "track_id": self._track_id(frame, obj)})
        if not out and not self._skip_empty:                     # dummy invalid label (posetrack21.py:117-128)
            out.append({"bbox": (-1.0, -1.0, 0.0, 0.0), "width": width, "height": height, "joints_3d": np.zeros((self.num_joints, 3, 2), np.float32),
                        "keypoint": [0.0] * (self.num_joints * 3), "id": -1, "ann_id": -1, "track_id": -1})
        return out

    # The host frame cache: at most FRAME_CACHE decoded frames, least recently used first out.  Everything that puts a frame in goes
    # through cache_frames, so the bound holds whoever decoded it (this thread on a miss, or a consumer that decodes ahead).

    def cache_frames(self, frames):
        """Take decoded frames {path: (H, W, 3) uint8} into the cache (as most recently used) and evict down to FRAME_CACHE.  Frames that
        arrive as coefficient blocks (device decoding) become pixels here, all of them in ONE `vh.jpeg_decode_batch` call on the
        calling thread, and are cached as device tensors."""
        import vatl_hip as vh
        packed = [(path, f) for path, f in frames.items() if isinstance(f, vh.JpegPacked)]
        if packed:                                                   # Huffman decoding on the device: one call, one status read-back for the batch
            data, offsets, hw, status = vh.jpeg_decode_packed_batch([f for _, f in packed])
            frames = dict(frames)
            for (path, _), off, (h, w), bad in zip(packed, offsets.tolist(), hw.tolist(), status.tolist()):
                frames[path] = _read_coefficients(path) if bad else data[off:off + h * w * 3].view(h, w, 3).clone()
        pending = [(path, f) for path, f in frames.items() if isinstance(f, vh.JpegCoefficients)]
        if pending:
            data, offsets, hw = vh.jpeg_decode_batch([f for _, f in pending])
            frames = dict(frames)
            for (path, _), off, (h, w) in zip(pending, offsets.tolist(), hw.tolist()):
                frames[path] = data[off:off + h * w * 3].view(h, w, 3).clone()       # its own buffer: a cached frame must not keep the batch's arena alive
        for path, img in frames.items():
            self._decoded[path] = img
            self._decoded.move_to_end(path)
        while len(self._decoded) > self.FRAME_CACHE:
            self._decoded.popitem(last=False)
        return frames

    def reserve_frame_cache(self, n_frames):
        """Make room for ``n_frames`` frames at least (a consumer that decodes a batch ahead holds two batches' frames)."""
        self.FRAME_CACHE = max(int(self.FRAME_CACHE), int(n_frames))

    def uncached_frames(self, idxs):
        """Paths of the items' frames that are not in the cache now (each path once)."""
        paths = (self._labels[int(i)]["frame"] for i in idxs)
        return [p for p in OrderedDict.fromkeys(paths) if p not in self._decoded]

    def _frame(self, path):
        img = self._decoded.get(path)
        if img is None:
            img = self.cache_frames({path: frame_loader(self)(path)})[path]
        else:
            self._decoded.move_to_end(path)
        return img

    def _frames_for(self, keys):
        uniq = list(OrderedDict.fromkeys(keys))
        have = {path: self._frame(path) for path in uniq if path in self._decoded}
        load = frame_loader(self)                                # the batch's misses go into the cache together: with device decoding, one pixel call for all of them
        have.update(self.cache_frames({path: load(path) for path in uniq if path not in have}))
        return FrameArena([have[path] for path in uniq]), {path: k for k, path in enumerate(uniq)}


@DATASET.register_module
class Posetrack21(_CocoVideo):
    """PoseTrack21 (posetrack21.py:12-24)."""
    EVAL_JOINTS = list(range(17))
    joint_pairs = [[5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]


@DATASET.register_module
class JRDB2022(_CocoVideo):
    """JRDB-Pose (jrdb2022.py:12-25)."""
    EVAL_JOINTS = list(range(17))
    joint_pairs = [[1, 2], [0, 4], [3, 4], [8, 10], [5, 7], [10, 13], [14, 16], [4, 5], [7, 12], [4, 8], [3, 6], [13, 15], [11, 14], [6, 9], [8, 11]]
    ID_DIGITS = 3
    STRICT_BOX = False

    def _track_id(self, frame, obj):
        return obj["track_id"]


class _CocoImages(_CocoVideo):
    """Image-only key-point datasets (pre-training): items are ``CustomDataset.__getitem__``'s 5-tuple
    (img (3,H,W), label, label_mask, img_id, bbox) (custom.py:96-113)."""
    REQUIRE_AREA = False

    def __init__(self, train=True, dpg=False, skip_empty=True, lazy_import=False, get_prenext=False, **cfg):
        super().__init__(train=train, dpg=dpg, skip_empty=skip_empty, lazy_import=lazy_import, get_prenext=False, **cfg)
        self.ID_SORTED_STREAM = False

    def _persons(self, db, frame):
        """``_check_load_keypoints`` of mscoco.py:60-115 / mpii.py:62-110 (``_check_centers`` is off in the reference)."""
        width, height = frame["width"], frame["height"]
        out = []
        for obj in db.anns_of.get(frame["id"], []):
            if obj.get("iscrowd", 0):
                continue
            if max(obj["keypoints"]) == 0:
                continue
            xmin, ymin, xmax, ymax = bbox_clip_xyxy(bbox_xywh_to_xyxy(obj["bbox"]), width, height)
            if (self.REQUIRE_AREA and obj["area"] <= 0) or xmax <= xmin or ymax <= ymin:
                continue
            if obj["num_keypoints"] == 0:
                continue
            joints_3d = np.zeros((self.num_joints, 3, 2), dtype=np.float32)
            kp = obj["keypoints"]
            for i in range(self.num_joints):
                joints_3d[i, 0, 0], joints_3d[i, 1, 0] = kp[i * 3 + 0], kp[i * 3 + 1]
                joints_3d[i, :2, 1] = min(1, kp[i * 3 + 2])
            if np.sum(joints_3d[:, 0, 1]) < 1:
                continue
            out.append({"bbox": (float(xmin), float(ymin), float(xmax), float(ymax)), "width": width, "height": height, "joints_3d": joints_3d})
        if not out and not self._skip_empty:
            out.append({"bbox": (-1.0, -1.0, 0.0, 0.0), "width": width, "height": height, "joints_3d": np.zeros((self.num_joints, 3, 2), np.float32)})
        return out

    collated = None                                          # (5-tuple items: no video columns; loaders go through __getitems__)

    def __getitems__(self, idxs):
        idxs = [int(i) for i in idxs]
        labels = [dict(self._labels[i]) for i in idxs]
        arena, where = self._frames_for([lb["frame"] for lb in labels])
        img, target, weight, boxes = self.transformation.call_batch(arena, [where[lb["frame"]] for lb in labels], labels)
        ids = [int(os.path.splitext(os.path.basename(lb["frame"]))[0]) for lb in labels]      # custom.py:103
        return [(img[k], target[k], weight[k], ids[k], boxes[k]) for k in range(len(idxs))]

    @staticmethod
    def my_collate_fn(batch):
        import torch
        cols = list(zip(*batch))
        return torch.stack(cols[0]), torch.stack(cols[1]), torch.stack(cols[2]), list(cols[3]), torch.stack(cols[4])


@DATASET.register_module
class Mscoco(_CocoImages):
    """COCO person key-points (mscoco.py:9-25).  ``SHORTEN`` is the reference's own switch: it stops after 30 images."""
    EVAL_JOINTS = list(range(17))
    joint_pairs = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
    SHORTEN = True
    REQUIRE_AREA = True

    def _image_path(self, frame):
        dirname, filename = frame["coco_url"].split("/")[-2:]    # mscoco.py:41-42
        return os.path.join(self._root, dirname, filename)

    def _stop_after(self, n_images):
        return self.SHORTEN and n_images >= 30                   # mscoco.py:53-55


@DATASET.register_module
class Mpii(_CocoImages):
    """MPII human pose, 16 joints (mpii.py:13-34)."""
    num_joints = 16
    EVAL_JOINTS = list(range(16))
    joint_pairs = [[0, 5], [1, 4], [2, 3], [10, 15], [11, 14], [12, 13]]

    def _image_path(self, frame):
        return os.path.join(self._root, self._img_prefix, frame["file_name"])                 # mpii.py:47-48
