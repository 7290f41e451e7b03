"""Pose-network pre-training on the device (alphapose/pretrain.py); its one-launch optimiser steps (csrc/optim.hip) are in test_gpu_optim.py."""
import json
import os
import random

import numpy as np
import pytest
import torch

from oracle import synth
from tests.conftest import GOLDEN
from tests.gpu_util import dev, record, to_dev

pytestmark = pytest.mark.gpu

SIMPLEPOSE = {"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50}


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    return vatl_hip


def _preset(hw=(256, 192)):
    from alphapose.utils.config import edict
    return edict({"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": list(hw), "HEATMAP_SIZE": [hw[0] // 4, hw[1] // 4]})


def _fixed_batches(sizes=(4, 4, 3), hw=(256, 192), seed=400):
    """The data set's 11-tuples from fixed tensors (only columns 1-3 are read by the training step)."""
    out = []
    for k, n in enumerate(sizes):
        x = torch.from_numpy(synth.crops(n, seed=seed + k, hw=hw))
        labels, masks = synth.gaussian_targets(n, seed=seed + 10 + k, hw=(hw[0] // 4, hw[1] // 4))
        out.append((list(range(n)), x[:, None], torch.from_numpy(labels), torch.from_numpy(masks), None, None, None, None, None, None, None))
    return out


def _fresh_simplepose(seed, hw=(256, 192)):
    from alphapose.models import builder
    from alphapose.utils.config import edict
    torch.manual_seed(seed)
    return builder.build_sppe(edict(SIMPLEPOSE), preset_cfg=_preset(hw))


def test_train_epoch_is_the_pinned_pieces(vh):
    """`train_epoch` over batches of 4, 4 and 3 equals — bit for bit, parameters and BatchNorm buffers — a loop written out here from
    hip_train.trainer_for, vh.masked_mse_fwd_bwd and the per-tensor vh.adam_step; its averages are the batch-size weighted ones."""
    from active_learning.optim import Adam
    from alphapose import pretrain
    from alphapose.models import hip_train
    from alphapose.utils.metrics import calc_accuracy
    batches = _fixed_batches()
    a = _fresh_simplepose(11).to(dev())
    b = _fresh_simplepose(11).to(dev())
    loss_avg, acc_avg = pretrain.train_epoch(a, batches, Adam(a.parameters(), lr=1e-3))

    b.train()
    tr = hip_train.trainer_for(b)
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
                torch.autograd.graph.increment_version(p)    # a write through the C ABI: the trainer's weight packs key on the counter
    for (k, pa), pb in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(pa.detach(), pb.detach()), k
    for (k, ba), bb in zip(a.named_buffers(), b.buffers()):
        assert torch.equal(ba, bb), k
    n = float(sum(counts))
    assert loss_avg == sum(l * c for l, c in zip(losses, counts)) / n
    assert acc_avg == sum(x * c for x, c in zip(accs, counts)) / n
    assert np.isfinite(loss_avg) and a.training


def test_three_step_trajectory_vs_reference_golden(vh):
    """tests/golden/pose_pretrain.npz: three steps of the reference's `train()` arithmetic with torch.optim.Adam(lr=1e-3) at B = 4 on
    128x96 crops, in fp32 and in float64.  Yardstick per stored quantity (the loss vector, bn1.running_mean, each sampled parameter
    tensor): the L2 distance of the reference's fp32 values from the float64 ones — how far the reference's own arithmetic is from
    exact.  Ours must lie within 3 x that distance of the float64 values (the x3 of test_hrnet_finetune_step_vs_reference_golden: the
    device and the CPU sum in different orders, and Adam's normalisation turns sign-level gradient noise into +-lr steps).
    Accuracies must be equal unless the fixture's fp32 and float64 accuracies already differ.  Measured on MI355X: ours / reference =
    2.13 for the losses, 1.05 for bn1.running_mean, 0.88 - 1.47 over the 19 sampled tensors (profiles/pose_pretrain_notes.md)."""
    from active_learning.optim import Adam
    from alphapose import pretrain
    g = np.load(os.path.join(GOLDEN, "pose_pretrain.npz"))
    hw = tuple(int(v) for v in g["hw"])
    m = _fresh_simplepose(int(g["seed"]), hw)                    # default init under the fixture's seed = the fixture's weights
    np.testing.assert_allclose(sum(float(p.detach().double().abs().sum()) for p in m.parameters()), float(g["wsum"]), rtol=1e-12)
    m = m.to(dev())
    opt = Adam(m.parameters(), lr=float(g["lr"]))
    B, hm = int(g["batch"]), (hw[0] // 4, hw[1] // 4)
    losses, accs = [], []
    for s in range(int(g["steps"])):
        labels, masks = synth.gaussian_targets(B, seed=int(g["target_seed"]) + s, hw=hm)
        x = torch.from_numpy(synth.crops(B, seed=int(g["crop_seed"]) + s, hw=hw))
        batch = (list(range(B)), x[:, None], torch.from_numpy(labels), torch.from_numpy(masks), None, None, None, None, None, None, None)
        loss, acc = pretrain.train_epoch(m, [batch], opt)
        losses.append(loss); accs.append(acc)
    named = dict(m.named_parameters())
    quantities = [("loss", np.asarray(losses, np.float64), g["loss_f32"], g["loss_f64"]),
                  ("bn1.running_mean", m.preact.bn1.running_mean.cpu().numpy(), g["bn1_running_mean_f32"], g["bn1_running_mean_f64"])]
    keys = [k.split("::", 1)[1] for k in g.files if k.startswith("idx::")]
    assert len(keys) >= 18
    for k in keys:
        idx = torch.from_numpy(g[f"idx::{k}"].astype(np.int64)).to(dev())
        quantities.append((k, named[k].detach().reshape(-1)[idx].cpu().numpy(), g[f"param_f32::{k}"], g[f"param_f64::{k}"]))
    bad = []
    for name, got, ref32, exact in quantities:
        ours = float(np.linalg.norm(np.asarray(got, np.float64) - exact))
        theirs = float(np.linalg.norm(np.asarray(ref32, np.float64) - exact))
        print(f"pose_pretrain {name}: ours vs float64 {ours:.4e}, reference fp32 vs float64 {theirs:.4e}")
        record("pose_pretrain_trajectory", quantity=name, ours_vs_f64=ours, reference_vs_f64=theirs)
        if not ours <= 3 * theirs:
            bad.append((name, ours, theirs))
    print("pose_pretrain accuracies:", accs, g["acc_f32"].tolist(), g["acc_f64"].tolist())
    for s, acc in enumerate(accs):
        if g["acc_f32"][s] == g["acc_f64"][s]:
            assert acc == g["acc_f64"][s], (s, acc, float(g["acc_f64"][s]))
    assert not bad, bad


def _posetrack_cfg(root, ann, batch=4):
    from alphapose.utils.config import edict
    ds = {"TYPE": "Posetrack21", "ROOT": str(root), "IMG_PREFIX": "", "ANN": ann,
          "AUG": {"SCALE_FACTOR": 0.25, "ROT_FACTOR": 30, "NUM_JOINTS_HALF_BODY": 8, "PROB_HALF_BODY": 0.3}}
    return edict({
        "DATASET": {"TRAIN": dict(ds), "VAL": dict(ds), "EVAL": dict(ds)},
        "DATA_PRESET": dict(_preset()), "MODEL": dict(SIMPLEPOSE), "LOSS": {"TYPE": "MSELoss"},
        "TRAIN": {"WORLD_SIZE": 1, "BATCH_SIZE": batch, "BEGIN_EPOCH": 0, "END_EPOCH": 3, "OPTIMIZER": "adam", "LR": 1e-3, "LR_FACTOR": 0.1,
                  "LR_STEP": [2], "DPG_MILESTONE": 1, "DPG_STEP": [2, 3]},
        "AE": {"Z_DIM": 4, "INPUT_DIM": 42, "PRETRAINED": "", "EPOCH": 1, "LR": 1e-3},
        "RETRAIN": {"BATCH_SIZE": 8, "BASE": 1, "OPTIMIZER": "AdamW", "LR": 2.5e-4, "ALPHA": 2, "WEIGHT_DECAY": 0.7, "LR_GAMMA": 0.99},
        "VAL": {"BATCH_SIZE": 4, "W_UNC": 0.01, "UNC_LAMBDA": 0.01, "QUERY_RATIO": [0.25, 1.0]},
    })


def test_validate_records_on_a_png_posetrack_layout(vh, tmp_path):
    """`validate` on 6 items of a tmp-dir PoseTrack layout: every record's key-points are heatmap_to_coord_simple of that item's
    heat-maps (bit-identical), `score` = mean + 1.25 max, the reference's key set, and without the COCO API the metric is
    100 x the mean vatl_oks."""
    from alphapose import pretrain
    from alphapose.models import builder, hip_engine
    from alphapose.utils.bbox import bbox_xyxy_to_xywh
    from alphapose.utils.metrics import have_coco_tools
    from alphapose.utils.transforms import heatmap_to_coord_simple
    ann, frames, kept = synth.write_coco_video(str(tmp_path), n_frames=3, tracks=2)
    cfg = _posetrack_cfg(tmp_path, ann)
    ds = builder.build_dataset(cfg.DATASET.VAL, preset_cfg=cfg.DATA_PRESET, train=False)
    assert len(ds) == 6
    m = _fresh_simplepose(5)
    m.load_state_dict(synth.state_dict_for(m), strict=True)      # heat-maps with structure (a fresh head's are nearly flat)
    m = m.to(dev())
    work = tmp_path / "work"
    res = pretrain.validate(m, cfg, ds, str(work))
    recs = json.load(open(work / "predicted_kpt.json"))
    assert res["records"] == len(recs) == 6 and not m.training
    oks = []
    for i, rec in enumerate(recs):
        assert sorted(rec) == ["ann_id", "bbox", "category_id", "image_id", "keypoints", "score"]
        idx, inp, label, mask, gt, img_id, ann_id, bb_crop, bb_ann, _, _ = ds[i]
        assert (rec["image_id"], rec["ann_id"], rec["category_id"]) == (int(img_id), int(ann_id), 1) and ann_id in kept
        assert rec["bbox"] == bb_crop.cpu().numpy().tolist()
        hm = torch.empty((1, 17, 64, 48), device=dev())
        with torch.no_grad():
            hip_engine.forward_into(m, inp[0][None].to(dev()), hm)
        coords, scores = heatmap_to_coord_simple(hm[0][ds.EVAL_JOINTS], bb_crop.cpu().numpy().tolist())
        kp = np.concatenate((coords, scores), axis=1)
        assert rec["keypoints"] == kp.reshape(-1).tolist()
        assert rec["score"] == float(np.mean(scores) + 1.25 * np.max(scores))
        xywh = bbox_xyxy_to_xywh(bb_ann.numpy().astype(np.float64)[None])
        oks.append(float(vh.oks(to_dev(kp[None]), to_dev(gt.numpy().astype(np.float64)[None], torch.float64), to_dev(xywh, torch.float64))[0]))
    if not have_coco_tools():
        assert res["val_metric"] == "mOKS" and res["metric"] == pytest.approx(100.0 * float(np.mean(oks)), rel=1e-12)
    else:
        assert res["val_metric"] == "mAP"


def _run_main(tmp_path, monkeypatch, ann, exp_id):
    from alphapose import pretrain
    import yaml
    cfg = _posetrack_cfg(tmp_path, ann)
    plain = json.loads(json.dumps(cfg))
    path = tmp_path / "tiny_res50.yaml"
    path.write_text(yaml.safe_dump(plain))
    monkeypatch.chdir(tmp_path)
    out = pretrain.main(["--cfg", str(path), "--exp-id", exp_id, "--snapshot", "1", "--seed", "3", "--workers", "2"])
    return cfg, out, tmp_path / "exp" / f"{exp_id}-tiny_res50"


def test_end_to_end_pretrain_then_active_learning(vh, tmp_path, monkeypatch):
    """`pretrain.main` on the PNG layout (BATCH_SIZE 4, END_EPOCH 3, DPG_MILESTONE 1, --snapshot 1): the reference's files, the run
    ends at the milestone, `final.pth` loads strictly and is what ActiveLearning starts from through MODEL.PRETRAINED; a second run
    with the same seed writes the same bits."""
    import types
    from active_learning import ActiveLearning
    from alphapose.models import builder
    from alphapose.utils.config import edict
    ann, frames, kept = synth.write_coco_video(str(tmp_path), n_frames=4, tracks=2)
    cfg, out, work = _run_main(tmp_path, monkeypatch, ann, "a")
    assert out["ended"] == "dpg_milestone" and out["epochs"] == [0, 1] and out["val_metric"] in ("mOKS", "mAP")
    for name in ("model_0.pth", "model_1.pth", "final.pth", "training.log", "predicted_kpt.json"):
        assert (work / name).exists(), name
    assert not (work / "final_DPG.pth").exists() and not (work / "model_2.pth").exists()
    assert (work / "model_best.pth").exists() and out["best_score"] > 0          # the first validation exceeds the initial best of 0
    log = open(work / "training.log").read()
    assert "Train-0 epoch | loss:" in log and "Train-1 epoch | loss:" in log and "training ends" in log and "Train-2" not in log
    assert len(json.load(open(work / "predicted_kpt.json"))) == 8
    sd = torch.load(work / "final.pth")
    assert all(not v.is_cuda for v in sd.values())
    builder.build_sppe(edict(SIMPLEPOSE), preset_cfg=_preset()).load_state_dict(sd)            # strict
    assert all(torch.equal(sd[k], v.detach().cpu()) for k, v in out["model"].state_dict().items())

    _, out2, work2 = _run_main(tmp_path, monkeypatch, ann, "b")
    for name in ("model_0.pth", "model_1.pth", "final.pth"):
        one, two = torch.load(work / name), torch.load(work2 / name)
        assert list(one) == list(two) and all(torch.equal(one[k], two[k]) for k in one), name
    assert out2["train_loss"] == out["train_loss"] and out2["val"] == out["val"]

    cfg.MODEL.PRETRAINED = str(work / "final.pth")
    opt = types.SimpleNamespace(work_dir=str(tmp_path / "al"), uncertainty="THC+WPU", representativeness="None", filter="None", strategy="THC+WPU",
                                video_id="vid0", get_prenext=True, continual=True, num_gpu=1, onebyone=False, retrain_thresh=1, THCvsWPU="const")
    os.makedirs(opt.work_dir, exist_ok=True)
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    al = ActiveLearning(cfg, opt)
    assert all(torch.equal(sd[k], v.detach().cpu()) for k, v in al.model.state_dict().items())
    al.eval_and_query()
    assert len(al.labeled_id) == 2 and len(al.unlabeled_id) == 6
    al.flush_records()
