"""Frame decoding: Pillow on the host against the hybrid decoder (Huffman pass on the host, pixels on the device) and against Huffman
decoding on the device (the host only packs the scan), on one MI355X.

    python tools/jpeg_decode_bench.py [--frames 48] [--rounds 3] [--epochs 8] [--trainer-modes host,device,device-huffman] [--noise-frames 4] [--out FILE]

Input: ``--frames`` JPEG streams of 1280x720, 4:2:0, quality 90, written by Pillow from SYNTHETIC content (a smooth colour field with
textured regions and noise; there are no photographs here, and the Huffman pass's share of the decode time depends on the content).

  decode     frames/s of "file bytes in memory -> frames in a device arena", modes alternated ``--rounds`` times in one process, each
             timed window = whole batches of ``--frames`` frames for at least a second:
               pillow_T   `_read_rgb` on T threads + `FrameArena(frames)`
               hybrid_T   `vh.jpeg_entropy_decode` on T threads + ONE `vh.jpeg_decode_batch`
               huffman_T  `vh.jpeg_pack` on T threads + ONE `vh.jpeg_decode_packed_batch`
             for T = 1 and 8
  split      the hybrid path's parts: Huffman pass per frame (host clock, one thread), coefficient upload and the two pixel launches
             (HIP events) for the whole batch; the device-Huffman path's: pack per frame (host clock), scan + table upload, the Huffman
             launches together and the pixel launches (HIP events), the synchronisation launches and how many thread blocks worked in each
  noise      the same decode rates and split for ``--noise-frames`` 640x480 frames of uniform noise at quality 100 (a 1280x720 one is above the device path's segment cap) — codes that hardly ever fall in
             step, the slow end of the synchronisation
  trainer    `alphapose.pretrain.train_epoch` steps/s at batch 32 over those frames as a PoseTrack-layout data set, the DECODER modes of
             ``--trainer-modes`` alternated, `DecodeAhead(8)`, ``--epochs`` epochs per timed run; every epoch decodes every frame

One JSON line on stdout (and into --out).

Two side doors: ``--dump-noise-frame FILE`` writes the frame tools/jpeg_lane_rate.hip measures the single-lane rate on, and
``--trace-batches N`` only runs the device-Huffman path N times, for `rocprofv3 --kernel-trace -- python tools/jpeg_decode_bench.py
--trace-batches 5`: the C entry enqueues all its launches in one call, so its kernels' times come from a trace, not from events."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vatl4pose-wacv2024_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIMPLEPOSE = {"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50}
PRESET = {"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]}
THREADS = (1, 8)


def synthetic_frame(k, hw=(720, 1280), seed=11):
    """Smooth colour field + band-limited texture in a few regions + mild sensor-like noise."""
    h, w = hw
    r = np.random.RandomState(seed + k)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([120 + 90 * np.sin(xx / 211 + 0.3 * k) * np.cos(yy / 173), 110 + 80 * np.cos(xx / 97 + yy / 301), 128 + 100 * np.sin((xx + yy) / 257 + k)], -1)
    coarse = r.randint(-60, 61, (h // 4, w // 4, 3)).astype(np.float32)
    texture = np.kron(coarse, np.ones((4, 4, 1), np.float32))
    mask = ((np.sin(xx / 150 + k) > 0.2) & (np.cos(yy / 120) > -0.3))[..., None]
    img = img + mask * texture + r.normal(0, 3, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(frames, quality=90):
    from PIL import Image
    out = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, format="JPEG", quality=quality, subsampling="4:2:0")
        out.append(buf.getvalue())
    return out


def decode_rates(streams, rounds, dev, window_s=1.0):
    import vatl_hip as vh
    from alphapose.datasets.coco_video import _read_rgb
    from alphapose.utils.presets.simple_transform import FrameArena
    pools = {t: ThreadPoolExecutor(max_workers=t) for t in THREADS if t > 1}

    def each(fn, t):
        return [fn(s) for s in streams] if t == 1 else list(pools[t].map(fn, streams))

    def pillow(t):
        arena = FrameArena(each(lambda s: _read_rgb(io.BytesIO(s)), t), dev)
        torch.cuda.synchronize()
        return arena.data

    def hybrid(t):
        data, _, _ = vh.jpeg_decode_batch(each(vh.jpeg_entropy_decode, t), dev)
        torch.cuda.synchronize()
        return data

    def huffman(t):
        data, _, _, status = vh.jpeg_decode_packed_batch(each(vh.jpeg_pack, t), dev)
        assert not status.any().item(), "a frame was rejected on the device"     # the read-back the data set does per batch (and the synchronisation)
        return data
    assert torch.equal(pillow(1), hybrid(1)) and torch.equal(pillow(1), huffman(1)), "the paths disagree"   # also the warm-up: code objects, pinned staging
    for t in THREADS:
        pillow(t), hybrid(t), huffman(t)
    res = {}
    for _ in range(rounds):
        for t in THREADS:
            for label, fn in ((f"pillow_{t}", pillow), (f"hybrid_{t}", hybrid), (f"huffman_{t}", huffman)):
                done, t0 = 0, time.perf_counter()
                while done < 3 or time.perf_counter() - t0 < window_s:       # whole batches until the window is full
                    fn(t)
                    done += 1
                res.setdefault(label, []).append(done * len(streams) / (time.perf_counter() - t0))
    for p in pools.values():
        p.shutdown()
    return {k: {"frames_per_s": v, "median": statistics.median(v), "spread": max(v) - min(v)} for k, v in res.items()}


def hybrid_split(streams, rounds, dev):
    import vatl_hip as vh
    out = {"entropy_ms_per_frame": [], "upload_ms_per_batch": [], "pixels_ms_per_batch": [], "pillow_ms_per_frame": []}
    from alphapose.datasets.coco_video import _read_rgb
    for _ in range(rounds):
        t0 = time.perf_counter()
        frames = [vh.jpeg_entropy_decode(s) for s in streams]
        out["entropy_ms_per_frame"].append(1e3 * (time.perf_counter() - t0) / len(streams))
        marks = []
        vh.jpeg_decode_batch(frames, dev, marks=marks)
        torch.cuda.synchronize()
        out["upload_ms_per_batch"].append(marks[0].elapsed_time(marks[1]))
        out["pixels_ms_per_batch"].append(marks[1].elapsed_time(marks[2]))
        t0 = time.perf_counter()
        for s in streams:
            _read_rgb(io.BytesIO(s))
        out["pillow_ms_per_frame"].append(1e3 * (time.perf_counter() - t0) / len(streams))
    out["frames"] = len(streams)
    out["coefficient_bytes_per_frame"] = 2 * frames[0].coef.numel()
    out["stream_bytes_per_frame"] = int(statistics.mean(len(s) for s in streams))
    return out


def huffman_split(streams, rounds, dev):
    import vatl_hip as vh
    out = {"pack_ms_per_frame": [], "upload_ms_per_batch": [], "huffman_ms_per_batch": [], "pixels_ms_per_batch": []}
    for _ in range(rounds):
        t0 = time.perf_counter()
        frames = [vh.jpeg_pack(s) for s in streams]
        out["pack_ms_per_frame"].append(1e3 * (time.perf_counter() - t0) / len(streams))
        marks, stats = [], {}
        vh.jpeg_decode_packed_batch(frames, dev, marks=marks, stats=stats)
        torch.cuda.synchronize()
        out["upload_ms_per_batch"].append(marks[0].elapsed_time(marks[1]))
        out["huffman_ms_per_batch"].append(marks[1].elapsed_time(marks[2]))
        out["pixels_ms_per_batch"].append(marks[3].elapsed_time(marks[4]))
    out["frames"] = len(streams)
    out["scan_bytes_per_frame"] = int(statistics.mean(f.scan.numel() for f in frames))
    out["sync_launches"], out["active_blocks_per_launch"] = stats["launches"], stats["active_blocks"]
    return out


def write_video(root, streams, hw=(720, 1280), persons=2, seed=7):
    r = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "images", "vid0"), exist_ok=True)
    images, anns = [], []
    for f, s in enumerate(streams):
        name = os.path.join("images", "vid0", f"{f:06d}.jpg")
        with open(os.path.join(root, name), "wb") as fh:
            fh.write(s)
        image_id = 1000200 + f
        images.append({"id": image_id, "image_id": image_id, "vid_id": 2, "file_name": name, "width": hw[1], "height": hw[0]})
        for t in range(persons):
            x0, y0, w, h = 100.0 + 400 * t + 3 * f, 80.0 + 5 * t, 220.0, 480.0
            kp = []
            for _ in range(17):
                kp += [float(x0 + r.uniform(10, w - 10)), float(y0 + r.uniform(10, h - 10)), 1]
            anns.append({"id": image_id * 100 + t, "image_id": image_id, "track_id": t, "category_id": 1, "bbox": [x0, y0, w, h], "keypoints": kp})
    with open(os.path.join(root, "annotations.json"), "w") as fh:
        json.dump({"images": images, "annotations": anns, "categories": [{"id": 1, "name": "person"}]}, fh)
    return "annotations.json"


def trainer_rates(streams, rounds, epochs, batch, dev, modes=("host", "device")):
    from active_learning.optim import Adam
    from alphapose import pretrain
    from alphapose.models import builder
    from alphapose.utils.config import edict
    torch.manual_seed(0)
    m = builder.build_sppe(edict(SIMPLEPOSE), preset_cfg=edict(PRESET)).to(dev)
    opt = Adam(m.parameters(), lr=1e-4)
    res = {"batch": batch, "decode_ahead": 8}
    with tempfile.TemporaryDirectory() as root:
        ann = write_video(root, streams)
        node = edict({"TYPE": "Posetrack21", "ROOT": root, "IMG_PREFIX": "", "ANN": ann,
                      "AUG": {"SCALE_FACTOR": 0.25, "ROT_FACTOR": 30, "NUM_JOINTS_HALF_BODY": 8, "PROB_HALF_BODY": 0.3}})
        sets = {}
        for mode in modes:
            sets[mode] = builder.build_dataset(node, preset_cfg=edict(PRESET), train=True)
            sets[mode].DECODER = mode
            sets[mode].emit_neighbour_crops = False
        steps = -(-len(sets[modes[0]]) // batch)
        gen = torch.Generator()
        gen.manual_seed(0)

        def epoch(ds):
            ds._decoded.clear()                                  # every epoch decodes every frame, as an epoch over a real data set does
            ahead = pretrain.DecodeAhead(ds, 8, batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pretrain.train_epoch(m, ahead.batches(pretrain.epoch_batches(len(ds), batch, gen)), opt)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ahead.close()
            return dt
        for mode in modes:                                       # warm-up: code objects, weight packs, pinned staging
            epoch(sets[mode])
        for _ in range(rounds):
            for mode in modes:
                res.setdefault(mode, []).append(steps * epochs / sum(epoch(sets[mode]) for _ in range(epochs)))
        res["items"], res["steps_per_epoch"] = len(sets[modes[0]]), steps
    return {**res, **{f"{k}_steps_per_s": {"runs": res[k], "median": statistics.median(res[k]), "spread": max(res[k]) - min(res[k])} for k in modes}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=8, help="epochs per timed run of the trainer")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--skip-trainer", action="store_true")
    ap.add_argument("--trainer-modes", default="host,device,device-huffman", help="DECODER modes the trainer run alternates")
    ap.add_argument("--noise-frames", type=int, default=4, help="frames of the quality-100 noise batch (0: skip it)")
    ap.add_argument("--out", default="")
    ap.add_argument("--dump-noise-frame", default="", metavar="FILE", help="only write the 256x256 quality-100 noise frame (input of tools/jpeg_lane_rate.hip; no GPU needed)")
    ap.add_argument("--trace-batches", type=int, default=0, metavar="N", help="only decode the batch N times with the device-Huffman path: the run to put under a kernel trace")
    a = ap.parse_args()
    if a.dump_noise_frame:                                           # tests/test_gpu_jpeg_huffman.py's "noise_q100_420", seed and all
        from PIL import Image
        Image.fromarray(np.random.RandomState(20241019).randint(0, 256, (256, 256, 3)).astype(np.uint8)).save(a.dump_noise_frame, "JPEG", quality=100, subsampling="4:2:0")
        return
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_decode_bench needs an MI355X: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    if a.trace_batches:
        import vatl_hip as vh
        frames = [vh.jpeg_pack(s) for s in encode([synthetic_frame(k) for k in range(a.frames)])]
        for _ in range(a.trace_batches):
            vh.jpeg_decode_packed_batch(frames, dev)
            torch.cuda.synchronize()
        return
    from PIL import Image, features
    streams = encode([synthetic_frame(k) for k in range(a.frames)])
    res = {"device": torch.cuda.get_device_name(0), "frames": a.frames, "rounds": a.rounds, "pillow": Image.__version__,
           "jpeglib": f"jpg {features.version('jpg')} libjpeg_turbo={bool(features.check_feature('libjpeg_turbo'))}",
           "content": "synthetic: smooth colour field + textured regions + noise, 1280x720 4:2:0 quality 90"}
    res["decode"] = decode_rates(streams, a.rounds, dev)
    print(f"# decode: { {k: v['frames_per_s'] for k, v in res['decode'].items()} }", file=sys.stderr, flush=True)
    res["split"] = hybrid_split(streams, a.rounds, dev)
    print(f"# split: {res['split']}", file=sys.stderr, flush=True)
    res["huffman_split"] = huffman_split(streams, a.rounds, dev)
    print(f"# huffman split: {res['huffman_split']}", file=sys.stderr, flush=True)
    if a.noise_frames:
        r = np.random.RandomState(3)
        noise = encode([r.randint(0, 256, (480, 640, 3)).astype(np.uint8) for _ in range(a.noise_frames)], quality=100)
        res["noise"] = {"content": "uniform noise, 640x480 4:2:0 quality 100", "frames": a.noise_frames, "decode": decode_rates(noise, a.rounds, dev),
                        "huffman_split": huffman_split(noise, a.rounds, dev)}
        print(f"# noise: {res['noise']}", file=sys.stderr, flush=True)
    if not a.skip_trainer:
        res["trainer"] = trainer_rates(streams, a.rounds, a.epochs, a.batch, dev, tuple(a.trainer_modes.split(",")))
        print(f"# trainer: {res['trainer']}", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
