#!/usr/bin/env python3
"""Optimiser-step and trainer times of the pose-network pre-training path on one MI355X (profiles/pose_pretrain_notes.md).

    python tools/pose_pretrain_bench.py [--reps 100] [--rounds 3] [--batch 32] [--frames 48] [--skip-trainer] [--skip-optimiser] [--out FILE]

Optimiser step, HIP events around each warm step, median of ``--reps`` (>= 50), over the real parameter sets of SimplePose-R50,
FastPose-R50 and HRNet-W32 with persistent gradient tensors; per-tensor and multi alternate ``--rounds`` times in this one process:
  adam_per_tensor     one ``vatl_adam_step`` launch per tensor (the parent commit's ``optim.Adam.step``, unchanged kernel: the baseline)
  adam_multi          one ``vatl_adam_step_multi`` launch
  rmsprop_per_tensor  one ``vatl_rmsprop_step`` launch per tensor
  rmsprop_multi       one ``vatl_rmsprop_step_multi`` launch
with the bytes each step must move (Adam: read p, g, m, v, write p, m, v = 28 B per element; RMSprop: 20 B) over the median time.
Trainer, by the host clock around an epoch that ends in the epoch's read-back (SimplePose-R50, ``--batch`` items per step):
  synthetic           ``train_epoch`` on ``SyntheticVideo`` items (host-made tensors)
  png_decode_ahead_N  ``train_epoch`` on a PoseTrack-layout data set of ``--frames`` 1280x720 PNG frames written to a temporary
                      directory, the next batch's frames decoded ahead on N threads (0 = decoded on the calling thread)
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vatl4pose-wacv2024_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIMPLEPOSE = {"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50}
FASTPOSE = {"TYPE": "FastPose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50}
HRNET = {"TYPE": "PoseHighResolutionNet", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50, "FINAL_CONV_KERNEL": 1, "PRETRAINED_LAYERS": ["*"],
         "STAGE2": {"NUM_MODULES": 1, "NUM_BRANCHES": 2, "NUM_BLOCKS": [4, 4], "NUM_CHANNELS": [32, 64], "BLOCK": "BASIC", "FUSE_METHOD": "SUM"},
         "STAGE3": {"NUM_MODULES": 4, "NUM_BRANCHES": 3, "NUM_BLOCKS": [4, 4, 4], "NUM_CHANNELS": [32, 64, 128], "BLOCK": "BASIC", "FUSE_METHOD": "SUM"},
         "STAGE4": {"NUM_MODULES": 3, "NUM_BRANCHES": 4, "NUM_BLOCKS": [4, 4, 4, 4], "NUM_CHANNELS": [32, 64, 128, 256], "BLOCK": "BASIC", "FUSE_METHOD": "SUM"}}
PRESET = {"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]}


def timed(fn, reps, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_us": statistics.median(ms) * 1e3, "min_us": min(ms) * 1e3, "p90_us": sorted(ms)[int(0.9 * (len(ms) - 1))] * 1e3}


def optimiser_times(name, cfg, reps, rounds, dev):
    import vatl_hip as vh
    from alphapose.models import builder
    from alphapose.utils.config import edict
    torch.manual_seed(0)
    m = builder.build_sppe(edict(cfg), preset_cfg=edict(PRESET)).to(dev)
    ps = [p.data for p in m.parameters()]
    gs = [torch.randn_like(p) * 1e-3 for p in ps]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    step = [0]

    def adam_per_tensor():
        step[0] += 1
        for p, g, mm, v in zip(ps, gs, ms, vs):
            vh.adam_step(p, g, mm, v, step[0], 1e-4)

    def adam_multi():
        step[0] += 1
        vh.adam_step_multi(ps, gs, ms, vs, step[0], 1e-4)

    def rmsprop_per_tensor():
        for p, g, v in zip(ps, gs, vs):
            vh.rmsprop_step(p, g, v, 1e-4)

    def rmsprop_multi():
        vh.rmsprop_step_multi(ps, gs, vs, 1e-4)

    elems = sum(p.numel() for p in ps)
    res = {"tensors": len(ps), "elements": elems, "state_dict_tensors": len(m.state_dict())}
    for label, fn, bytes_per in (("adam_per_tensor", adam_per_tensor, 28), ("adam_multi", adam_multi, 28),
                                 ("rmsprop_per_tensor", rmsprop_per_tensor, 20), ("rmsprop_multi", rmsprop_multi, 20)):
        res[label] = {"rounds": [], "bytes": elems * bytes_per}
    for _ in range(rounds):                                    # alternate the variants: a drift of the box hits all of them alike
        for label, fn in (("adam_per_tensor", adam_per_tensor), ("adam_multi", adam_multi), ("rmsprop_per_tensor", rmsprop_per_tensor),
                          ("rmsprop_multi", rmsprop_multi)):
            res[label]["rounds"].append(timed(fn, reps))
    for label in ("adam_per_tensor", "adam_multi", "rmsprop_per_tensor", "rmsprop_multi"):
        med = statistics.median(r["median_us"] for r in res[label]["rounds"])
        res[label]["median_us"] = med
        res[label]["tb_per_s"] = res[label]["bytes"] / (med * 1e-6) / 1e12
    res["adam_speedup"] = res["adam_per_tensor"]["median_us"] / res["adam_multi"]["median_us"]
    res["rmsprop_speedup"] = res["rmsprop_per_tensor"]["median_us"] / res["rmsprop_multi"]["median_us"]
    print(f"# {name}: {json.dumps({k: (v['median_us'] if isinstance(v, dict) else v) for k, v in res.items()})}", file=sys.stderr, flush=True)
    return res


def write_png_video(root, n_frames, hw=(720, 1280), persons=2, seed=7):
    """A PoseTrack21-layout data set: ``n_frames`` PNG frames, ``persons`` tracks, one COCO-format json."""
    from PIL import Image
    r = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "images", "vid0"), exist_ok=True)
    base = r.randint(0, 255, (hw[0] // 8, hw[1] // 8, 3)).astype(np.uint8)
    images, anns = [], []
    for f in range(n_frames):
        img = np.kron(np.roll(base, f, axis=1), np.ones((8, 8, 1), np.uint8))         # blocky content: PNG compresses it, decode still walks every pixel
        img = (img.astype(np.int16) + r.randint(-6, 7, img.shape)).clip(0, 255).astype(np.uint8)
        name = os.path.join("images", "vid0", f"{f:06d}.png")
        Image.fromarray(img).save(os.path.join(root, name), compress_level=1)
        image_id = 1000200 + f
        images.append({"id": image_id, "image_id": image_id, "vid_id": 2, "file_name": name, "width": hw[1], "height": hw[0]})
        for t in range(persons):
            x0, y0, w, h = 100.0 + 400 * t + 3 * f, 80.0 + 5 * t, 220.0, 480.0
            kp = []
            for j in range(17):
                kp += [float(x0 + r.uniform(10, w - 10)), float(y0 + r.uniform(10, h - 10)), 1]
            anns.append({"id": image_id * 100 + t, "image_id": image_id, "track_id": t, "category_id": 1, "bbox": [x0, y0, w, h], "keypoints": kp})
    ann = os.path.join("annotations.json")
    with open(os.path.join(root, ann), "w") as f:
        json.dump({"images": images, "annotations": anns, "categories": [{"id": 1, "name": "person"}]}, f)
    return ann


def trainer_times(batch, n_frames, epochs, dev):
    from active_learning.optim import Adam
    from alphapose import pretrain
    from alphapose.models import builder
    from alphapose.utils.config import edict
    torch.manual_seed(0)
    m = builder.build_sppe(edict(SIMPLEPOSE), preset_cfg=edict(PRESET)).to(dev)
    opt = Adam(m.parameters(), lr=1e-4)
    res = {"batch": batch}

    def epochs_per_s(dataset, workers, label):
        if hasattr(dataset, "emit_neighbour_crops"):
            dataset.emit_neighbour_crops = False
        gen = torch.Generator()
        gen.manual_seed(0)
        times = []
        for e in range(epochs + 1):                             # the first epoch warms code objects, packs and the pinned staging
            if hasattr(dataset, "_decoded"):
                dataset._decoded.clear()                        # every epoch decodes every frame, as an epoch over a real data set does
            ahead = pretrain.DecodeAhead(dataset, workers, batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pretrain.train_epoch(m, ahead.batches(pretrain.epoch_batches(len(dataset), batch, gen)), opt)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            ahead.close()
        steps = -(-len(dataset) // batch)
        med = statistics.median(times[1:])
        res[label] = {"items": len(dataset), "steps_per_epoch": steps, "epoch_s": times[1:], "steps_per_s": steps / med, "items_per_s": len(dataset) / med}
        print(f"# {label}: {res[label]}", file=sys.stderr, flush=True)

    synth_set = builder.build_dataset(edict({"TYPE": "SyntheticVideo", "NUM_ITEMS": 4 * batch, "TRACKS": 2}), preset_cfg=edict(PRESET), train=True)
    epochs_per_s(synth_set, 0, "synthetic")
    with tempfile.TemporaryDirectory() as root:
        ann = write_png_video(root, n_frames)
        node = edict({"TYPE": "Posetrack21", "ROOT": root, "IMG_PREFIX": "", "ANN": ann,
                      "AUG": {"SCALE_FACTOR": 0.25, "ROT_FACTOR": 30, "NUM_JOINTS_HALF_BODY": 8, "PROB_HALF_BODY": 0.3}})
        png = builder.build_dataset(node, preset_cfg=edict(PRESET), train=True)
        for workers in (0, 8, 0, 8):                            # alternated: the same code twice shows the spread
            label = f"png_decode_ahead_{workers}"
            epochs_per_s(png, workers, label if label not in res else label + "_again")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--skip-trainer", action="store_true")
    ap.add_argument("--skip-optimiser", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_pretrain_bench needs an MI355X: a CPU run measures nothing")
    if a.reps < 50:
        raise SystemExit("--reps must be at least 50")
    dev = torch.device("cuda:0")
    res = {"reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "optimiser": {}}
    for name, cfg in (() if a.skip_optimiser else (("simplepose_r50", SIMPLEPOSE), ("fastpose_r50", FASTPOSE), ("hrnet_w32", HRNET))):
        res["optimiser"][name] = optimiser_times(name, cfg, a.reps, a.rounds, dev)
    if not a.skip_trainer:
        res["trainer"] = trainer_times(a.batch, a.frames, a.epochs, dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
