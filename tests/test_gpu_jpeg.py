"""Device half of the hybrid JPEG decoder (csrc/jpeg.hip through vh.jpeg_decode_batch) against Pillow's own bytes
(tests/golden/jpeg.npz), and the data sets with DECODER = "device" against DECODER = "host"."""
import json
import os

import numpy as np
import pytest
import torch

import jpeg_cases
from gpu_util import dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


@pytest.fixture(scope="module")
def cases():
    return jpeg_cases.load()[0]


@pytest.fixture(scope="module")
def decoded(vh, cases):
    """{name: coefficient frame} of every admitted case (host pass, once)."""
    return {n: vh.jpeg_entropy_decode(cases[n][0]) for n in jpeg_cases.ADMITTED_NAMES}


@pytest.mark.parametrize("name", jpeg_cases.ADMITTED_NAMES)
def test_each_case_alone_equals_pillow(vh, cases, decoded, name):
    rgb = cases[name][1]
    data, offsets, hw = vh.jpeg_decode_batch([decoded[name]], dev())
    assert data.dtype == torch.uint8 and data.numel() == rgb.size and offsets.tolist() == [0] and hw.tolist() == [list(rgb.shape[:2])]
    got = data.cpu().numpy().reshape(rgb.shape)
    assert np.array_equal(got, rgb), f"{name}: {np.count_nonzero(got != rgb)} bytes differ"


@pytest.mark.parametrize("order", ["fixture", "reversed"])
def test_all_cases_in_one_call(vh, cases, decoded, order):
    """One call for the sixteen frames: offsets are running sums of h*w*3 (the second frame of the fixture order starts at byte 243),
    every frame equals Pillow's bytes, and the guard region behind the arena's last byte stays as it was."""
    names = list(jpeg_cases.ADMITTED_NAMES) if order == "fixture" else list(reversed(jpeg_cases.ADMITTED_NAMES))
    want = np.concatenate([cases[n][1].reshape(-1) for n in names])
    guard = 4096
    out = torch.full((want.size + guard,), 0xA5, dtype=torch.uint8, device=dev())
    data, offsets, hw = vh.jpeg_decode_batch([decoded[n] for n in names], dev(), out=out)
    assert data.data_ptr() == out.data_ptr()
    sizes = [cases[n][1].size for n in names]
    assert offsets.tolist() == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    if order == "fixture":
        assert offsets[1] == 243
    assert any(o % 4 for o in offsets.tolist()) and hw.tolist() == [list(cases[n][1].shape[:2]) for n in names]
    got = out.cpu().numpy()
    for n, o, s in zip(names, offsets.tolist(), sizes):
        assert np.array_equal(got[o:o + s], cases[n][1].reshape(-1)), f"{n} at offset {o}"
    assert np.array_equal(got[:want.size], want)
    assert np.all(got[want.size:] == 0xA5), "bytes behind the arena were written"


def test_crops_over_the_device_decoded_arena(vh, cases, decoded):
    """SimpleTransform.test_transform_batch reads the decoder's arena as it reads FrameArena(Pillow's frames): the same crops, bit for bit."""
    from alphapose.datasets.frame_video import FrameVideo
    from alphapose.utils.presets.simple_transform import FrameArena, SimpleTransform
    names = list(jpeg_cases.ADMITTED_NAMES)
    arena = FrameArena.from_packed(*vh.jpeg_decode_batch([decoded[n] for n in names], dev()))
    ref = FrameArena([cases[n][1] for n in names])
    assert np.array_equal(arena.offsets, ref.offsets) and np.array_equal(arena.hw, ref.hw)
    st = SimpleTransform(FrameVideo, scale_factor=0, add_dpg=False, input_size=[64, 48], output_size=[16, 12], rot=0, sigma=2, train=False)
    idx = list(range(len(names)))
    boxes = np.array([[1.0, 1.0, cases[n][1].shape[1] - 2.0, cases[n][1].shape[0] - 1.5] for n in names])
    a, box_a = st.test_transform_batch(arena, idx, boxes)
    b, box_b = st.test_transform_batch(ref, idx, boxes)
    assert torch.equal(a, b) and torch.equal(box_a, box_b)
    # ... and FrameArena over device tensors (what the data set caches) mixed with host frames is the same arena
    views = [arena.data[o:o + h * w * 3].view(h, w, 3) for o, (h, w) in zip(arena.offsets.tolist(), arena.hw.tolist())]
    mixed = FrameArena([v if k % 3 else cases[n][1] for k, (n, v) in enumerate(zip(names, views))])
    assert torch.equal(mixed.data, ref.data) and np.array_equal(mixed.offsets, ref.offsets) and np.array_equal(mixed.hw, ref.hw)


def _write_posetrack(root, cases):
    """A PoseTrack layout whose frames are the fixture's 40x56 streams as they are: 4:2:0, 4:4:4 and the progressive one (refused by the
    probe, so the Pillow fall-back is on the path)."""
    os.makedirs(os.path.join(root, "images", "vid0"), exist_ok=True)
    os.makedirs(os.path.join(root, "annotations"), exist_ok=True)
    rng = np.random.RandomState(5)
    images, anns = [], []
    for f, name in enumerate(["c40x56_420", "c40x56_444", "progressive", "c40x56_420"]):
        file_name = os.path.join("images", "vid0", f"{f:06d}.jpg")
        with open(os.path.join(root, file_name), "wb") as fh:
            fh.write(cases[name][0])
        image_id = 1000300 + f
        images.append({"id": image_id, "image_id": image_id, "vid_id": 3, "file_name": file_name, "width": 56, "height": 40})
        for t in range(2):
            x, y, w, h = 3.0 + 18 * t + f, 2.0 + f, 24.0, 30.0
            kp = []
            for _ in range(17):
                kp += [float(rng.uniform(x, x + w)), float(rng.uniform(y, y + h)), 1]
            anns.append({"id": image_id * 100 + t, "image_id": image_id, "track_id": t, "bbox": [x, y, w, h], "keypoints": kp, "category_id": 1})
    with open(os.path.join(root, "annotations", "val.json"), "w") as fh:
        json.dump({"images": images, "annotations": anns, "categories": [{"id": 1, "name": "person"}]}, fh)
    return os.path.join("annotations", "val.json")


def _same_batch(a, b):
    assert len(a) == len(b) == 11
    for col, (x, y) in enumerate(zip(a, b)):
        if torch.is_tensor(x):
            assert torch.equal(x.cpu(), y.cpu()), f"column {col} differs"
        else:
            assert x == y, f"column {col} differs"


def test_posetrack_batches_do_not_depend_on_the_decoder(vh, cases, tmp_path):
    from alphapose import pretrain
    from alphapose.datasets.coco_video import Posetrack21
    ann = _write_posetrack(str(tmp_path), cases)
    preset = {"IMAGE_SIZE": [64, 48], "HEATMAP_SIZE": [16, 12], "SIGMA": 2}

    def make(decoder):
        ds = Posetrack21(train=False, get_prenext=True, ROOT=str(tmp_path), ANN=ann, PRESET=preset)
        ds.DECODER = decoder
        return ds
    host, device = make("host"), make("device")
    assert Posetrack21.DECODER in ("host", "auto") and len(host) == 8
    lists = pretrain.epoch_batches(len(host), 3)
    want = [host.collated(idxs) for idxs in lists]
    for idxs, w in zip(lists, want):
        _same_batch(device.collated(idxs), w)
    cached = {os.path.basename(p): f for p, f in device._decoded.items()}
    assert len(cached) == 4
    for file_name, f in cached.items():
        if file_name == "000002.jpg":                             # the progressive frame came through Pillow
            assert isinstance(f, np.ndarray)
        else:
            assert torch.is_tensor(f) and f.is_cuda and f.dtype == torch.uint8 and tuple(f.shape) == (40, 56, 3)
    assert all(isinstance(f, np.ndarray) for f in host._decoded.values())
    # through decode-ahead workers: the pool runs read-file + Huffman decode, the calling thread makes the pixels
    ahead_ds = make("device")
    ahead = pretrain.DecodeAhead(ahead_ds, workers=4, batch_size=3)
    try:
        got = list(ahead.batches(lists))
    finally:
        ahead.close()
    for g, w in zip(got, want):
        _same_batch(g, w)
    assert sum(torch.is_tensor(f) for f in ahead_ds._decoded.values()) == 3
