"""The constructor as the unchanged driver calls it: ``ActiveLearning(cfg, opt)`` with no dataset objects, the config and option
namespace of scripts/run_active_learning.sh as the reference's own set-up produces them (tests/golden/driver_namespace.json, case
a_posetrack), on a tiny PoseTrack21 layout at the derived paths.  The video's annotation file is found from ``opt.video_id``, the WPU
auto-encoder is loaded from ``AE.PRETRAINED_ROOT`` and scores with its checkpoint weights, ``latest_AE.pth`` is written after the
fine-tune, and a write through ``.data`` reaches the next evaluation's WPU scores."""
import copy
import json
import os
import shutil
import types

import pytest
import torch

from tests.conftest import GOLDEN
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu


def _case():
    with open(os.path.join(GOLDEN, "driver_namespace.json")) as f:
        return json.load(f)["cases"]["a_posetrack"]


def test_driver_constructor_paths_and_wpu_autoencoder(tmp_path, monkeypatch):
    import vatl_hip as vh
    from active_learning import ActiveLearning
    from active_learning.Whole_body_AE.AutoEncoder import WholeBodyAE
    from alphapose.models import builder
    from alphapose.utils.config import edict
    from oracle import synth

    case = _case()
    monkeypatch.chdir(tmp_path)
    cfg = edict(copy.deepcopy(case["cfg_before"]))                   # the shipped yaml after set_dir: IMG_PREFIX / ANN empty
    # 5 % of 8 items is no query at all: the first round queries 2 of them (VAL / RETRAIN / AE otherwise as shipped)
    cfg.VAL.QUERY_RATIO = [0.25, 1.0]
    ev = case["derived"]["EVAL"]

    # the derived PoseTrack21 layout: frames under ROOT, the video's annotation file at ROOT/ANN
    synth.write_coco_video(root=ev["ROOT"].rstrip("/"), n_frames=4, tracks=2)
    os.makedirs(os.path.join(ev["ROOT"], os.path.dirname(ev["ANN"])), exist_ok=True)
    shutil.move(os.path.join(ev["ROOT"], "annotations", "val.json"), os.path.join(ev["ROOT"], ev["ANN"]))

    torch.manual_seed(3)
    ckpt = WholeBodyAE(z_dim=4, input_dim=42).state_dict()           # seeded 42-d auto-encoder at the reference's path
    os.makedirs(os.path.dirname(case["ae_path"]), exist_ok=True)
    torch.save(ckpt, case["ae_path"])
    m = builder.build_sppe(cfg.MODEL, preset_cfg=cfg.DATA_PRESET)
    os.makedirs(os.path.dirname(cfg.MODEL.PRETRAINED), exist_ok=True)
    torch.save(synth.state_dict_for(m), cfg.MODEL.PRETRAINED)
    del m

    work_dir = tmp_path / "work"
    work_dir.mkdir()
    opt = types.SimpleNamespace(**{**case["opt"], "num_gpu": 1, "gpus": [0], "device": torch.device("cuda"), "work_dir": str(work_dir)})

    calls = []
    real = vh.hybrid_ae_wpu

    def recording(kpts, bbox, ae_flat, d, z, only38=False):
        wpu, status = real(kpts, bbox, ae_flat, d, z, only38)
        calls.append({"kpts": kpts.clone(), "bbox": bbox.clone(), "ae_flat": ae_flat.clone(), "dims": (d, z, only38), "wpu": wpu.clone()})
        return wpu, status
    monkeypatch.setattr(vh, "hybrid_ae_wpu", recording)

    torch.manual_seed(0)
    al = ActiveLearning(cfg, opt)
    try:
        assert al.dataset == "Posetrack21" and type(al.eval_dataset).__name__ == "Posetrack21" and len(al.eval_dataset) == 8
        assert al.cfg.DATASET.EVAL.ANN == ev["ANN"] and al.cfg.DATASET.EVAL.IMG_PREFIX == ev["IMG_PREFIX"]
        assert al.eval_dataset._ann_file == os.path.join(ev["ROOT"], ev["ANN"])
        sd = al.AE.state_dict()
        assert (al.AE.input_dim, al.AE.z_dim) == (42, 4)
        assert list(sd) == list(ckpt) and all(torch.equal(sd[k].cpu(), ckpt[k]) for k in ckpt)

        # first evaluation: WPU scored with the checkpoint's weights
        al.eval_and_query()
        assert len(calls) == 1
        c = calls[0]
        assert c["dims"] == (42, 4, False)
        assert torch.equal(c["ae_flat"], vh.pack_ae(ckpt, dev()))
        again, _ = real(c["kpts"], c["bbox"], vh.pack_ae(ckpt, dev()), 42, 4, False)
        assert torch.equal(c["wpu"], again) and torch.isfinite(c["wpu"]).all()
        assert len(al.labeled_id) == 2

        # one round: the auto-encoder is fine-tuned from the checkpoint and written where the reference writes it
        assert al.outcome() is None
        path = work_dir / "latest_AE.pth"
        assert path.exists()
        saved = torch.load(str(path), map_location="cpu")
        fresh = WholeBodyAE(input_dim=42, z_dim=4)
        fresh.load_state_dict(saved, strict=True)
        now = al.AE.state_dict()
        assert all(saved[k].device.type == "cpu" and torch.equal(saved[k], now[k].cpu()) for k in now)
        assert any(not torch.equal(saved[k], ckpt[k]) for k in ckpt)          # fine-tuned on the 2 labelled people

        al.eval_and_query()
        assert torch.equal(calls[-1]["ae_flat"], vh.pack_ae(al.AE.state_dict(), dev()))

        # a write that bumps no version counter still reaches the next evaluation
        w = al.AE.encoder[0].weight
        w2 = torch.randn(w.shape, generator=torch.Generator().manual_seed(5)).to(w.device)
        al.AE.encoder[0].weight.data.copy_(w2)
        al.eval_and_query()
        assert torch.equal(calls[-1]["ae_flat"][:w2.numel()], w2.reshape(-1))
        assert torch.equal(calls[-1]["ae_flat"], vh.pack_ae(al.AE.state_dict(), dev()))
    finally:
        al.close()
