"""Opt-in bf16 pre-training of SimplePose (alphapose/pretrain.py, TRAIN.PRECISION / --precision): the epoch as its pinned pieces (which is
also the end-to-end proof of the one-launch filter re-pack: planned equal to unplanned over three optimiser updates), an eight-step
trajectory beside the fp32 trainer under the two pre-training optimisers, the command line end to end, and the untouched default."""
import json
import sys

import numpy as np
import pytest
import torch

from oracle import synth
from tests.gpu_util import dev, record, to_dev

pytestmark = pytest.mark.gpu

HW, HM = (96, 64), (24, 16)            # crops and heat-maps: layer4 runs at 3x2
SIMPLEPOSE = {"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50}


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def _preset():
    from alphapose.utils.config import edict
    return edict({"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": list(HW), "HEATMAP_SIZE": list(HM)})


def _fresh_simplepose(seed):
    from alphapose.models import builder
    from alphapose.utils.config import edict
    torch.manual_seed(seed)
    return builder.build_sppe(edict(SIMPLEPOSE), preset_cfg=_preset())          # default initialisation under the seed


def _fixed_batches(sizes, seed=500):
    """The data set's 11-tuples from fixed tensors (only columns 1-3 are read by the training step)."""
    out = []
    for k, n in enumerate(sizes):
        x = torch.from_numpy(synth.crops(n, seed=seed + k, hw=HW))
        labels, masks = synth.gaussian_targets(n, seed=seed + 10 + k, hw=HM)
        out.append((list(range(n)), x[:, None], torch.from_numpy(labels), torch.from_numpy(masks), None, None, None, None, None, None, None))
    return out


def test_bf16_train_epoch_is_the_pinned_pieces(vh, monkeypatch):
    """`train_epoch(..., precision="bf16")` over batches of 3, 3 and 2 equals — bit for bit, parameters and BatchNorm buffers — a loop
    written out here from hip_train_h16.trainer_for_h16, vh.masked_mse_fwd_bwd and the per-tensor vh.adam_step with the one-launch
    re-pack switched OFF; its averages are the batch-size weighted ones.  The epoch runs under the plan (recording step, then two
    refreshes behind an optimiser update each), so this is also planned == unplanned."""
    from active_learning.optim import Adam
    from alphapose import pretrain
    from alphapose.models import hip_train_h16
    from alphapose.utils.metrics import calc_accuracy
    batches = _fixed_batches((3, 3, 2))
    a = _fresh_simplepose(11).to(dev())
    b = _fresh_simplepose(11).to(dev())
    assert hip_train_h16._USE_PACK_PLAN is True
    loss_avg, acc_avg = pretrain.train_epoch(a, batches, Adam(a.parameters(), lr=1e-3), precision="bf16")
    plan = a.__dict__["_vatl_trainer_h16"].__dict__["_pack_plan"]
    assert plan.ready and not plan.stale and len(plan.jobs) == 113
    assert "_vatl_trainer" not in a.__dict__

    monkeypatch.setattr(hip_train_h16, "_USE_PACK_PLAN", False)
    b.train()
    tr = hip_train_h16.trainer_for_h16(b)
    params = [p for p in b.parameters()]
    ms, vs = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    losses, accs, counts = [], [], []
    for step, (_, inps, labels, masks, *_rest) in enumerate(batches, 1):
        x, lab, msk = to_dev(inps[:, 0].numpy()), to_dev(labels.numpy()), to_dev(masks.numpy())
        with torch.no_grad():
            out = tr.forward(x)
            loss, dout = vh.masked_mse_fwd_bwd(out, lab, msk)
            grads = tr.backward(dout)
            accs.append(calc_accuracy(out * msk, lab * msk)); losses.append(float(loss)); counts.append(x.shape[0])
            for p, m, v in zip(params, ms, vs):
                vh.adam_step(p.data, grads[p].contiguous(), m, v, step, 1e-3)
                torch.autograd.graph.increment_version(p)    # a write through the C ABI: the trainer's filter packs key on the counter
    assert "_pack_plan" not in tr.__dict__
    for (k, pa), pb in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(pa.detach(), pb.detach()), k
    for (k, ba), bb in zip(a.named_buffers(), b.buffers()):
        assert torch.equal(ba, bb), k
    n = float(sum(counts))
    assert loss_avg == sum(l * c for l, c in zip(losses, counts)) / n
    assert acc_avg == sum(x * c for x, c in zip(accs, counts)) / n
    assert np.isfinite(loss_avg) and a.training


@pytest.mark.parametrize("optimizer", ["Adam", "RMSprop"])
def test_eight_step_trajectory_beside_the_fp32_trainer(vh, optimizer):
    """Eight steps of a pre-training optimiser (lr 1e-3) on one fixed batch of 8 from the same initialisation, once per trainer.
    Gradient rounding of about 2^-8 cannot halve the progress; a sign, a scale or a stale pack can: the bf16 loss decrease must be at
    least half of the fp32 trainer's (the rule and margin of tests/test_gpu_train_h16.py)."""
    from active_learning import optim
    from alphapose.models import hip_train, hip_train_h16
    x = to_dev(synth.crops(8, seed=81, hw=HW))
    labels, masks = (to_dev(t) for t in synth.gaussian_targets(8, seed=82, hw=HM))
    curves = {}
    for name, get in (("fp32", hip_train.trainer_for), ("bf16", hip_train_h16.trainer_for_h16)):
        m = _fresh_simplepose(7).to(dev()).train()
        tr, arena = get(m), hip_train.arena_for(m)
        opt = getattr(optim, optimizer)(m.parameters(), lr=1e-3)
        losses = []
        for _ in range(9):                                            # the ninth forward only measures the loss after eight steps
            with torch.no_grad():
                out = tr.forward(x)
                loss, dout = vh.masked_mse_fwd_bwd(out, labels, masks)
                losses.append(loss)
                if len(losses) == 9:
                    tr.backward(dout)                                 # leaves no tape behind
                    break
                arena.begin()
                tr.backward(dout, arena=arena)
                arena.finish()
                arena.attach()
            opt.step()
        curves[name] = [float(l) for l in losses]
    record("pretrain_h16_trajectory", optimizer=optimizer, fp32=curves["fp32"], bf16=curves["bf16"])
    print(optimizer, "fp32", curves["fp32"], "\nbf16", curves["bf16"])
    d32, d16 = curves["fp32"][0] - curves["fp32"][-1], curves["bf16"][0] - curves["bf16"][-1]
    assert all(np.isfinite(curves["bf16"])) and d32 > 0
    assert d16 >= 0.5 * d32, (d16, d32)


def _posetrack_yaml(root, ann, batch=4):
    """The yaml of a tmp-dir PNG PoseTrack layout (oracle.synth.write_coco_video), as tests/test_gpu_pose_pretrain.py builds it."""
    import yaml
    ds = {"TYPE": "Posetrack21", "ROOT": str(root), "IMG_PREFIX": "", "ANN": ann,
          "AUG": {"SCALE_FACTOR": 0.25, "ROT_FACTOR": 30, "NUM_JOINTS_HALF_BODY": 8, "PROB_HALF_BODY": 0.3}}
    cfg = {
        "DATASET": {"TRAIN": dict(ds), "VAL": dict(ds), "EVAL": dict(ds)},
        "DATA_PRESET": json.loads(json.dumps(_preset())), "MODEL": dict(SIMPLEPOSE), "LOSS": {"TYPE": "MSELoss"},
        "TRAIN": {"WORLD_SIZE": 1, "BATCH_SIZE": batch, "BEGIN_EPOCH": 0, "END_EPOCH": 3, "OPTIMIZER": "adam", "LR": 1e-3, "LR_FACTOR": 0.1,
                  "LR_STEP": [2], "DPG_MILESTONE": 0, "DPG_STEP": [2, 3]},
        "VAL": {"BATCH_SIZE": 4, "W_UNC": 0.01, "UNC_LAMBDA": 0.01, "QUERY_RATIO": [0.25, 1.0]},
    }
    path = root / "tiny_res50.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return path


def test_end_to_end_bf16_pretrain_from_the_command_line(vh, tmp_path, monkeypatch):
    """`pretrain.main --precision bf16 --max-epochs 1` on the PNG layout: the reference's files, fp32 CPU tensors under the reference's
    keys that load strictly, a log that names the precision, the bf16 trainer (and only it) on the model, validation records written."""
    from alphapose import pretrain
    from alphapose.models import builder
    from alphapose.utils.config import edict
    ann, frames, kept = synth.write_coco_video(str(tmp_path), n_frames=3, tracks=2)
    path = _posetrack_yaml(tmp_path, ann)
    monkeypatch.chdir(tmp_path)
    out = pretrain.main(["--cfg", str(path), "--exp-id", "h", "--snapshot", "1", "--seed", "3", "--workers", "2", "--precision", "bf16", "--max-epochs", "1"])
    work = tmp_path / "exp" / "h-tiny_res50"
    assert out["precision"] == "bf16" and out["epochs"] == [0] and out["ended"] == "dpg_milestone" and np.isfinite(out["train_loss"][0])
    for name in ("model_0.pth", "final.pth", "training.log", "predicted_kpt.json"):
        assert (work / name).exists(), name
    log = open(work / "training.log").read()
    assert "training precision: bf16" in log and "Train-0 epoch | loss:" in log
    assert len(json.load(open(work / "predicted_kpt.json"))) == 6
    m = out["model"]
    assert "_vatl_trainer_h16" in m.__dict__ and "_vatl_trainer" not in m.__dict__
    fresh = builder.build_sppe(edict(SIMPLEPOSE), preset_cfg=_preset())
    for name in ("model_0.pth", "final.pth"):
        sd = torch.load(work / name)
        assert list(sd) == list(fresh.state_dict())
        assert all(not v.is_cuda for v in sd.values())
        assert all(v.dtype == torch.float32 for k, v in sd.items() if not k.endswith("num_batches_tracked"))
        fresh.load_state_dict(sd, strict=True)
    assert all(torch.equal(sd[k], v.detach().cpu()) for k, v in m.state_dict().items())
    assert not all(torch.equal(v, w) for v, w in zip(sd.values(), _fresh_simplepose(3).state_dict().values()))      # it trained


def test_default_route_is_untouched(vh, monkeypatch):
    """With no precision given train_epoch asks hip_train.trainer_for for its trainer and never imports the bf16 module."""
    from active_learning.optim import Adam
    from alphapose import pretrain
    from alphapose.models import hip_train
    import alphapose.models as models_pkg
    monkeypatch.delitem(sys.modules, "alphapose.models.hip_train_h16", raising=False)
    monkeypatch.delattr(models_pkg, "hip_train_h16", raising=False)
    calls = []
    real = hip_train.trainer_for
    monkeypatch.setattr(hip_train, "trainer_for", lambda m: (calls.append(m), real(m))[1])
    m = _fresh_simplepose(13).to(dev())
    loss, acc = pretrain.train_epoch(m, _fixed_batches((2,)), Adam(m.parameters(), lr=1e-3))
    assert np.isfinite(loss) and calls and all(c is m for c in calls)
    assert "alphapose.models.hip_train_h16" not in sys.modules
    assert "_vatl_trainer" in m.__dict__ and "_vatl_trainer_h16" not in m.__dict__
    from alphapose.utils.config import edict
    assert pretrain.train_precision(edict({"MODEL": dict(SIMPLEPOSE), "TRAIN": {"BATCH_SIZE": 4}})) == "fp32"
