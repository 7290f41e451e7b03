"""Cases of tests/test_gpu_train_step_bits.py and tools/make_train_step_bits.py: the fp32 fine-tune step (alphapose/models/hip_train.py) of the three pose
networks on the smallest shapes that reach every branch of its data-gradient assembler and of its BatchNorm backward, every tensor a step produces
reduced to its SHA-256 and its first values as bit patterns.  The fixture tests/golden/train_step_parent_bits.npz holds what the commit BEFORE the layer
classes were given one data-gradient function and one BatchNorm tape gave: a launch that moved, a changed argument or another order shows as a changed bit.

  simplepose  B = 3 at 64x64   every layer of SimplePose-R50, stage 4 at 2x2; the one case that also runs with hip_train._FUSE_BN_BWD off (every
                               layer on the stand-alone BatchNorm backward)
  simplepose  B = 2 at 96x96   stages 3 and 4 at 6x6 and 3x3: the four stride-2 phases and the 1x1 / stride-2 projections work from an odd grid
  (64x48 and 96x80, the shapes of tests/train_tape_cases.py, are refused by the fp32 step: its stride-2 data gradients want even input extents and
  stage 3 would be 4x3 and 6x5.  These are the next larger multiples of 32.)
  fastpose    B = 2 at 128x96  SE blocks, _LinearT, DUC, pixel shuffle
  fastpose_dcn                 ... with modulated deformable conv2 in stages 2 - 4 on the ordered (bit-reproducible) path: the offset conv's data
                               gradient at stride 1 and at stride 2, in 32 carried channels
  hrnet       B = 2 at 128x96  HRNet-W32: _ChainT, _BasicBlockT, fusion rows, dx_residual chains

Runs per case: step 1; step 2 after every parameter was multiplied in place by 1 + 2^-10 (the pack plan replays and refreshes every packed filter);
step 2 again from a fresh model with hip_train._USE_PACK_PLAN off, which must give step 2's bits (so the fixture stores them once).
"""
import hashlib
import os

import numpy as np
import torch

from oracle import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_step_parent_bits.npz")
SEED = 5
BUMP = 1.0 + 2.0 ** -10
HEAD = 16                                       # values kept per tensor beside its hash: 6664 tensors, the fixture stays under 1 MB

PRESET = {"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]}
SIMPLEPOSE = {"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50}
FASTPOSE = {"TYPE": "FastPose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50}
FASTPOSE_DCN = dict(FASTPOSE, DCN={"MODULATED": True, "DEFORM_GROUP": 1, "FALLBACK_ON_STRIDE": False}, STAGE_WITH_DCN=[False, True, True, True])

# name -> (network, (B, H, W) of the crops, recorded runs)
STEPS = ("step1", "step2")
CASES = {
    "simplepose_b3_64x64": ("simplepose", (3, 64, 64), STEPS + ("step1_unfused",)),
    "simplepose_b2_96x96": ("simplepose", (2, 96, 96), STEPS),
    "fastpose_b2_128x96": ("fastpose", (2, 128, 96), STEPS),
    "fastpose_dcn_b2_128x96": ("fastpose_dcn", (2, 128, 96), STEPS),
    "hrnet_w32_b2_128x96": ("hrnet", (2, 128, 96), STEPS),
}


def _config(kind):
    if kind == "hrnet":
        from tests.test_train_f64_cpu import HRNET
        return HRNET
    return {"simplepose": SIMPLEPOSE, "fastpose": FASTPOSE, "fastpose_dcn": FASTPOSE_DCN}[kind]


def model(kind, dev):
    from alphapose.models import builder
    from alphapose.utils.config import edict
    torch.manual_seed(SEED)
    return builder.build_sppe(edict(_config(kind)), preset_cfg=edict(PRESET)).to(dev).train()          # default initialisation under the seed


def batch(shape, dev):
    """Crops and targets of oracle/synth.py; all three networks give heat-maps of a quarter of the crop at these multiples of 32."""
    b, h, w = shape
    assert h % 32 == 0 and w % 32 == 0
    x = synth.crops(b, seed=61, hw=(h, w))
    labels, masks = synth.gaussian_targets(b, seed=62, hw=(h // 4, w // 4))
    return tuple(torch.from_numpy(np.ascontiguousarray(t)).float().to(dev) for t in (x, labels, masks))


def _np(t):
    return t.detach().cpu().numpy()


def step(vh, m, x, labels, masks):
    """forward + loss + backward into the arena -> {name: array}: heat-maps, loss, every gradient, every BatchNorm buffer afterwards."""
    from alphapose.models import hip_train
    tr, arena = hip_train.trainer_for(m), hip_train.arena_for(m)
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


def run(vh, name, dev, plan=True, fuse=True, steps=2):
    """``steps`` fp32 steps from one fresh model of case ``name`` with hip_train._USE_PACK_PLAN = ``plan`` and _FUSE_BN_BWD = ``fuse``, every parameter
    scaled by BUMP in place between them -> [records of step 1, records of step 2].  A DCN case runs on the ordered deformable backward."""
    from alphapose.models import hip_train
    kind, shape, _ = CASES[name]
    m = model(kind, dev)
    data = batch(shape, dev)
    keep = (hip_train._USE_PACK_PLAN, hip_train._FUSE_BN_BWD, vh.deform_deterministic_mode())
    hip_train._USE_PACK_PLAN, hip_train._FUSE_BN_BWD = plan, fuse
    if kind == "fastpose_dcn":
        from alphapose.models.layers import dcn
        dcn.set_deterministic(True)
    try:
        out = []
        for k in range(steps):
            if k:
                with torch.no_grad():
                    for p in m.parameters():
                        p.mul_(BUMP)
            out.append(step(vh, m, *data))
        return out
    finally:
        hip_train._USE_PACK_PLAN, hip_train._FUSE_BN_BWD = keep[:2]
        vh.set_deform_deterministic(keep[2])


def reduce(records):
    """{name: array} -> (names joined by newlines, (T,32) uint8 SHA-256 of each tensor's bytes, (T,HEAD) uint64 bit patterns of its first values, zero-padded)."""
    sha = np.zeros((len(records), 32), np.uint8)
    head = np.zeros((len(records), HEAD), np.uint64)
    for i, a in enumerate(records.values()):
        a = np.ascontiguousarray(a)
        sha[i] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)
        bits = a.reshape(-1)[:HEAD].view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
        head[i, :bits.size] = bits
    return "\n".join(records), sha, head
