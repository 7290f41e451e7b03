"""Cases of tests/test_gpu_train_tape_bits.py and tools/make_train_tape_bits.py: the float64 reference step and the bf16 step of SimplePose-R50
(alphapose/models/hip_train_f64.py, hip_train_h16.py) on two small shapes, every tensor a step produces reduced to its SHA-256 and its first 64 values
as bit patterns.  The fixture tests/golden/train_tape_parent_bits.npz holds what the commit BEFORE the two trainers were put on one tape
(alphapose/models/hip_train_tape.py, csrc/wgrad_generic.h) gave: a call that moved, a changed argument or another summation order shows as a changed bit.

  B = 3 at 64x48: the stem output has 3 * 32 * 24 = 2304 pixels, so both weight-gradient kernels cross their 2048-pixel chunk once (a second split of
                  256 pixels); stages 2, 3 and 4 have 144, 36 and 12 pixels, no multiples of the 64-pixel (bf16) and, from stage 3 on, the 16-pixel
                  (float64) k-tile;
  B = 2 at 96x80: stages 3 and 4 run at 6x5 and 3x3 (odd extents): the four stride-2 data-gradient phases have different grids.
"""
import hashlib
import os

import numpy as np
import torch

from oracle import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_tape_parent_bits.npz")
SHAPES = ((3, 64, 48), (2, 96, 80))             # (B, H, W) of the crops
RUNS = ("f64", "h16_step1", "h16_step2_plan", "h16_step2_noplan")
SEED = 5
BUMP = 1.0 + 2.0 ** -10                         # every parameter is multiplied by this between the two bf16 steps: each filter is re-packed


def shape_id(shape):
    return "b%d_%dx%d" % shape


def model(dev):
    from alphapose.models import builder
    from alphapose.utils.config import edict
    cfg = edict({"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50})
    preset = edict({"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]})
    torch.manual_seed(SEED)
    return builder.build_sppe(cfg, preset_cfg=preset).to(dev).train()          # default initialisation under the seed


def heatmap_hw(h, w):
    """Five halvings (rounded up: 48 -> 2, 80 -> 3 columns in stage 4), three doublings."""
    for _ in range(5):
        h, w = (h + 1) // 2, (w + 1) // 2
    return 8 * h, 8 * w


def batch(shape, dev):
    b, h, w = shape
    x = synth.crops(b, seed=61, hw=(h, w))
    labels, masks = synth.gaussian_targets(b, seed=62, hw=heatmap_hw(h, w))
    return tuple(torch.from_numpy(np.ascontiguousarray(t)).float().to(dev) for t in (x, labels, masks))


def _np(t):
    return t.detach().cpu().numpy()


def run_f64(shape, dev):
    """One float64 reference step -> {name: array}: the heat-maps, every gradient, every entry of batch_statistics()."""
    from alphapose.models import hip_train_f64
    m = model(dev)
    x, labels, masks = batch(shape, dev)
    tr = hip_train_f64.trainer_for_f64(m)
    hm = tr.forward(x)
    grads = tr.backward((hm - labels.double()) * masks.double())
    stats = tr.batch_statistics()
    torch.cuda.synchronize()
    out = {"heatmaps": _np(hm)}
    for k, p in m.named_parameters():
        out["grad." + k] = _np(grads[p])
    for k, bn in m.named_modules():
        if isinstance(bn, torch.nn.BatchNorm2d):
            for key in ("mean", "var", "running_mean", "running_var"):
                out[f"stat.{k}.{key}"] = _np(stats[bn][key])
    return out


def _h16_step(vh, m, x, labels, masks):
    """forward + loss + backward into the arena -> {name: array}: heat-maps, loss, every gradient, every BatchNorm buffer afterwards."""
    from alphapose.models import hip_train, hip_train_h16
    tr, arena = hip_train_h16.trainer_for_h16(m), hip_train.arena_for(m)
    with torch.no_grad():
        hm = tr.forward(x)
        loss, dout = vh.masked_mse_fwd_bwd(hm, labels, masks)
        arena.begin()
        tr.backward(dout, arena=arena)
        arena.finish()
        arena.attach()
    torch.cuda.synchronize()
    out = {"heatmaps": _np(hm), "loss": np.asarray(_np(torch.as_tensor(loss)), np.float32).reshape(-1)}
    for k, p in m.named_parameters():
        out["grad." + k] = _np(arena.views[p])
    for k, bn in m.named_modules():
        if isinstance(bn, torch.nn.BatchNorm2d):
            for key in ("running_mean", "running_var", "num_batches_tracked"):
                out[f"buf.{k}.{key}"] = _np(getattr(bn, key))
    return out


def run_h16(vh, shape, dev, plan):
    """Two bf16 steps from one fresh model with hip_train_h16._USE_PACK_PLAN = ``plan``, every parameter scaled by BUMP in place between them (the second
    forward pass refreshes every bf16 filter: by the plan's one launch, or per tensor) -> (records of step 1, records of step 2)."""
    from alphapose.models import hip_train_h16
    m = model(dev)
    data = batch(shape, dev)
    keep, hip_train_h16._USE_PACK_PLAN = hip_train_h16._USE_PACK_PLAN, plan
    try:
        one = _h16_step(vh, m, *data)
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(BUMP)
        two = _h16_step(vh, m, *data)
    finally:
        hip_train_h16._USE_PACK_PLAN = keep
    return one, two


def runs(vh, shape, dev, which=RUNS):
    """{run: {name: array}} for the runs of ``which``."""
    out = {}
    if "f64" in which:
        out["f64"] = run_f64(shape, dev)
    if "h16_step1" in which or "h16_step2_plan" in which:
        out["h16_step1"], out["h16_step2_plan"] = run_h16(vh, shape, dev, True)
    if "h16_step2_noplan" in which:
        out["h16_step2_noplan"] = run_h16(vh, shape, dev, False)[1]
    return {k: v for k, v in out.items() if k in which}


def reduce(records):
    """{name: array} -> (names joined by newlines, (T,32) uint8 SHA-256 of each tensor's bytes, (T,64) uint64 bit patterns of its first 64 values, zero-padded)."""
    sha = np.zeros((len(records), 32), np.uint8)
    head = np.zeros((len(records), 64), np.uint64)
    for i, a in enumerate(records.values()):
        a = np.ascontiguousarray(a)
        sha[i] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)
        bits = a.reshape(-1)[:64].view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
        head[i, :bits.size] = bits
    return "\n".join(records), sha, head
