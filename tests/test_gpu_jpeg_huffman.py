"""Huffman decoding on the device (csrc/jpeg_huffman.hip through vh.jpeg_huffman_batch / vh.jpeg_decode_packed_batch) against the host
decoder vh.jpeg_entropy_decode — the coefficients, int16 for int16 — and through it against Pillow's bytes; and the data sets with
DECODER = "device-huffman" against "device" and "host"."""
import io
import os

import numpy as np
import pytest
import torch

import jpeg_cases
import jpeg_synth
from gpu_util import dev
from test_gpu_jpeg import _same_batch, _write_posetrack

pytestmark = pytest.mark.gpu

NAMES = jpeg_cases.ADMITTED_NAMES + ("synth",)


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


@pytest.fixture(scope="module")
def cases():
    return jpeg_cases.load()[0]


@pytest.fixture(scope="module")
def streams(cases):
    out = {n: cases[n][0] for n in jpeg_cases.ADMITTED_NAMES}
    out["synth"] = jpeg_synth.gray_block_stream(jpeg_synth.SHORT_CODE_TABLE, jpeg_synth.SHORT_CODE_COEFFICIENTS)[0]
    return out


@pytest.fixture(scope="module")
def host(vh, streams):
    """{name: the host decoder's coefficient frame}: the yardstick, made once."""
    return {n: vh.jpeg_entropy_decode(streams[n]) for n in NAMES}


def _pillow(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def _check_batch(vh, packed, want_coef, want_rgb):
    """One call for ``packed``: every status 0, every frame's coefficients the host decoder's, every frame's pixels ``want_rgb``'s."""
    coef, table, status = vh.jpeg_huffman_batch(packed, dev())
    assert status.tolist() == [0] * len(packed)
    for k, want in enumerate(want_coef):
        got = coef[int(table[k, 4]) * 64:int(table[k + 1, 4]) * 64].cpu()
        assert torch.equal(got, want), f"frame {k}: {int((got != want).sum())} coefficients differ"
    data, offsets, hw, status = vh.jpeg_decode_packed_batch(packed, dev())
    assert status.tolist() == [0] * len(packed)
    got = data.cpu().numpy()
    for k, (rgb, o) in enumerate(zip(want_rgb, offsets.tolist())):
        assert hw[k].tolist() == list(rgb.shape[:2]) and np.array_equal(got[o:o + rgb.size], rgb.reshape(-1)), f"frame {k}: pixels differ"


def test_all_fixture_streams_in_one_batch(vh, cases, streams, host):
    rgb = [cases[n][1] if n in cases else _pillow(streams[n]) for n in NAMES]
    _check_batch(vh, [vh.jpeg_pack(streams[n]) for n in NAMES], [host[n].coef for n in NAMES], rgb)


# --- states that have to cross thread-block boundaries --------------------------------------------------------------

def _jpeg(img, **save):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", **save)
    return b.getvalue()


@pytest.fixture(scope="module")
def long_frames(vh):
    """name -> (bytes, packed, the host decoder's coefficients, Pillow's pixels), seeded content written by Pillow here."""
    rng = np.random.RandomState(20241019)
    noise = rng.randint(0, 256, (256, 256, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:256, 0:256]
    smooth = np.stack([xx, yy, 127 + 120 * np.sin(0.05 * xx + 0.03 * yy)], -1).clip(0, 255).astype(np.uint8)
    made = {
        "noise_q100_420": _jpeg(noise, quality=100, subsampling="4:2:0"),
        "noise_q100_420_rst": _jpeg(noise, quality=100, subsampling="4:2:0", restart_marker_rows=1),
        "noise_q95_444": _jpeg(rng.randint(0, 256, (200, 312, 3)).astype(np.uint8), quality=95, subsampling="4:4:4"),
        "smooth_q50": _jpeg(smooth, quality=50),
    }
    return {n: (d, vh.jpeg_pack(d), vh.jpeg_entropy_decode(d).coef, _pillow(d)) for n, d in made.items()}


def test_the_long_frames_span_thread_blocks(vh, long_frames):
    """The sizes the tests below rely on, from the pack output: the noise frames cover three thread blocks at least, the frame with
    restart markers has sixteen segments that start inside blocks, the smooth frame is a few dozen subsequences with many blocks each."""
    per_block = vh.JPEG_BLOCK_SUBS * vh.JPEG_SUB_BYTES
    for name in ("noise_q100_420", "noise_q100_420_rst", "noise_q95_444"):
        assert long_frames[name][1].scan.numel() > 3 * per_block, name
    assert long_frames["noise_q100_420"][1].segments.shape[0] == 1
    rows = long_frames["noise_q100_420_rst"][1].segments
    assert rows.shape[0] == 16 and sum(int(r[0]) % per_block != 0 for r in rows) >= 12
    smooth = long_frames["smooth_q50"][1]
    assert 8 <= smooth.scan.numel() // vh.JPEG_SUB_BYTES <= 64 and smooth.blocks > 20 * (smooth.scan.numel() // vh.JPEG_SUB_BYTES)


@pytest.mark.parametrize("name", ["noise_q100_420", "noise_q100_420_rst", "noise_q95_444", "smooth_q50"])
def test_each_long_frame_alone(vh, long_frames, name):
    _, packed, coef, rgb = long_frames[name]
    _check_batch(vh, [packed], [coef], [rgb])


def test_long_frames_in_one_mixed_batch(vh, long_frames, streams, host, cases):
    """The four long frames with small fixture frames between them: one launch sequence serves segments of one and of five thread blocks."""
    names = ["c9x9_420", "noise_q100_420", "smooth_q50", "noise_q95_444", "c17x23_gray", "noise_q100_420_rst", "noise_q100"]
    packed = [long_frames[n][1] if n in long_frames else vh.jpeg_pack(streams[n]) for n in names]
    coef = [long_frames[n][2] if n in long_frames else host[n].coef for n in names]
    rgb = [long_frames[n][3] if n in long_frames else cases[n][1] for n in names]
    _check_batch(vh, packed, coef, rgb)
    stats = {}
    vh.jpeg_huffman_batch(packed, dev(), stats=stats)
    assert stats["launches"] >= 4 and stats["active_blocks"][0] == sum(-(-p.scan.numel() // (vh.JPEG_BLOCK_SUBS * vh.JPEG_SUB_BYTES)) for p in packed)
    assert stats["active_blocks"][1] >= 1 and stats["active_blocks"][2] >= 1     # quality-100 noise: states cross two block boundaries at least
    alone = {}
    vh.jpeg_huffman_batch([long_frames["noise_q100_420"][1]], dev(), stats=alone)
    assert alone["launches"] == 4 and alone["active_blocks"][0] == 4 and alone["active_blocks"][2] >= 1      # ... in that frame by itself too


# --- damaged streams ---------------------------------------------------------------------------------------------

def test_damaged_streams_fail_alone(vh, streams, host):
    """The fixture's damaged streams (those that pack), one batch per case, each between two intact frames: status 0 exactly where the host
    decoder succeeds, and then its coefficients; the intact frames keep theirs; nothing outside the batch's coefficients or arena is written."""
    guard, rejected, survived = 4096, 0, 0
    intact = ("noise_q50", "c33x47_420_rst_rows1")
    for name in jpeg_cases.ADMITTED_NAMES:
        frames, want = [vh.jpeg_pack(streams[intact[0]])], [host[intact[0]].coef]
        for label, data in jpeg_cases.damaged(name, streams[name]):
            if not vh.jpeg_probe(data).admitted:
                continue
            try:
                frames.append(vh.jpeg_pack(data))
            except vh.VatlError:
                with pytest.raises(vh.VatlError):                      # a restart marker is missing: the host decoder says so too
                    vh.jpeg_entropy_decode(data)
                continue
            try:
                want.append(vh.jpeg_entropy_decode(data).coef)
            except vh.VatlError:
                want.append(None)
        frames.append(vh.jpeg_pack(streams[intact[1]]))
        want.append(host[intact[1]].coef)
        total = 64 * sum(f.blocks for f in frames)
        whole = torch.full((guard + total + guard,), 0x5A5A, dtype=torch.int16, device=dev())      # canaries in front of the batch and behind it
        buf = whole[guard:]
        coef, table, status = vh.jpeg_huffman_batch(frames, dev(), coef=buf)
        assert coef.data_ptr() == buf.data_ptr()
        assert bool((whole[:guard] == 0x5A5A).all()) and bool((buf[total:] == 0x5A5A).all()), f"{name}: coefficients outside the batch were written"
        for k, (w, st) in enumerate(zip(want, status.tolist())):
            assert (st == 0) == (w is not None), f"{name} frame {k}: status {st}, host decoder {'succeeds' if w is not None else 'raises'}"
            if w is not None:
                assert torch.equal(buf[int(table[k, 4]) * 64:int(table[k + 1, 4]) * 64].cpu(), w), f"{name} frame {k}"
        rejected += sum(w is None for w in want)
        survived += sum(w is not None for w in want) - 2
        arena = sum(f.height * f.width * 3 for f in frames)
        around = torch.full((guard + arena + guard,), 0xA5, dtype=torch.uint8, device=dev())
        out = around[guard:]
        _, _, _, status2 = vh.jpeg_decode_packed_batch(frames, dev(), out=out)
        assert status2.tolist() == status.tolist()
        assert bool((around[:guard] == 0xA5).all()) and bool((out[arena:] == 0xA5).all()), f"{name}: bytes outside the arena were written"
    assert rejected > 50 and survived > 50


# --- the data set -----------------------------------------------------------------------------------------------

def test_posetrack_batches_do_not_depend_on_the_decoder(vh, cases, tmp_path, monkeypatch):
    """DECODER = "device-huffman" gives the batches of "device" and "host"; a truncated file is rejected on the device, read again through
    the "device" path's loader, and ends where it ends in every mode: with Pillow's error."""
    import json
    from alphapose import pretrain
    from alphapose.datasets import coco_video
    from alphapose.datasets.coco_video import Posetrack21
    ann = _write_posetrack(str(tmp_path), cases)
    with open(os.path.join(str(tmp_path), ann)) as fh:
        db = json.load(fh)
    cut = dict(db["images"][0], id=1000304, image_id=1000304, file_name=os.path.join("images", "vid0", "000004.jpg"))
    truncated = cases["c40x56_420"][0][:len(cases["c40x56_420"][0]) // 2]
    with open(os.path.join(str(tmp_path), cut["file_name"]), "wb") as fh:
        fh.write(truncated)
    # the truncated stream packs — a worker hands it on — and it is the device's status that rejects it
    _, _, status = vh.jpeg_huffman_batch([vh.jpeg_pack(cases["c40x56_444"][0]), vh.jpeg_pack(truncated)], dev())
    assert status.tolist()[0] == 0 and status.tolist()[1] != 0
    db["images"].append(cut)
    db["annotations"] += [dict(a, id=a["id"] + 400, image_id=1000304) for a in db["annotations"][:2]]
    with open(os.path.join(str(tmp_path), ann), "w") as fh:
        json.dump(db, fh)
    preset = {"IMAGE_SIZE": [64, 48], "HEATMAP_SIZE": [16, 12], "SIGMA": 2}
    reread = []
    plain = coco_video._read_coefficients
    monkeypatch.setattr(coco_video, "_read_coefficients", lambda path: (reread.append(os.path.basename(path)), plain(path))[1])

    def make(decoder):
        ds = Posetrack21(train=False, get_prenext=True, ROOT=str(tmp_path), ANN=ann, PRESET=preset)
        ds.DECODER = decoder
        return ds
    sets = {d: make(d) for d in ("host", "device", "device-huffman")}
    assert len(sets["host"]) == 10
    # batches by frame: items of the first three frames (whose neighbour frames are intact too), items of the truncated one, and a mixed batch
    frame_of = [os.path.basename(label["frame"]) for label in sets["host"]._labels]
    intact = [i for i, f in enumerate(frame_of) if f in ("000000.jpg", "000001.jpg", "000002.jpg")]
    broken = [i for i, f in enumerate(frame_of) if f == "000004.jpg"]
    assert len(intact) == 6 and len(broken) == 2
    lists = [intact[:3], intact[3:], broken[:1], [intact[0], broken[1]]]
    good, bad = [], 0
    for idxs in lists:
        try:
            want = sets["host"].collated(idxs)
        except OSError:
            bad += 1
            del reread[:]
            for d in ("device", "device-huffman"):
                with pytest.raises(OSError):
                    sets[d].collated(idxs)
            assert reread.count("000004.jpg") == 2                     # once per mode: "device-huffman" came back to this loader
            continue
        good.append(idxs)
        for d in ("device", "device-huffman"):
            _same_batch(sets[d].collated(idxs), want)
    assert good == lists[:2] and bad == 2
    cached = {os.path.basename(p): f for p, f in sets["device-huffman"]._decoded.items()}
    assert sum(torch.is_tensor(f) and f.is_cuda for f in cached.values()) >= 2 and "000004.jpg" not in cached
    assert isinstance(cached.get("000002.jpg", np.zeros(1)), np.ndarray)      # the progressive frame came through Pillow
    ahead_ds = make("device-huffman")                                  # through decode-ahead workers: the pool packs, the calling thread decodes
    ahead = pretrain.DecodeAhead(ahead_ds, workers=4, batch_size=3)
    try:
        got = list(ahead.batches(good))
    finally:
        ahead.close()
    for g, idxs in zip(got, good):
        _same_batch(g, sets["host"].collated(idxs))
