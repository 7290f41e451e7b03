"""Loop logic of alphapose/pretrain.py without a GPU: the epoch loop with a stub training step and a stub validator, the three
branches of ``preset_model`` on a tiny module, configuration / file names / the log line, and the imports the module must not make."""
import os
import subprocess
import sys

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**train):
    from alphapose.utils.config import edict
    t = {"BATCH_SIZE": 4, "BEGIN_EPOCH": 0, "END_EPOCH": 8, "OPTIMIZER": "adam", "LR": 1e-3, "LR_FACTOR": 0.5, "LR_STEP": [2, 4],
         "DPG_MILESTONE": 6, "DPG_STEP": [1, 3]}
    t.update(train)
    return edict({"TRAIN": t, "MODEL": {"TYPE": "Tiny", "PRETRAINED": "", "TRY_LOAD": ""}, "DATA_PRESET": {"NUM_JOINTS": 17}, "FILE_NAME": "tiny"})


class Tiny(nn.Module):
    def __init__(self, width=3, **_):
        super().__init__()
        self.a = nn.Linear(2, width)
        self.b = nn.Linear(width, 1)
        self.initialized = False

    def _initialize(self):
        self.initialized = True
        with torch.no_grad():
            for p in self.parameters():
                p.fill_(0.25)


def _run(cfg, tmp_path, scores=None, **kw):
    """run_epochs with stubs -> (summary, log lines, {file name: lr when it was saved})."""
    from alphapose import pretrain
    m = Tiny()
    opt = torch.optim.SGD(m.parameters(), lr=cfg.TRAIN.LR)
    lines, saved, calls = [], {}, {"train": [], "val": []}

    def train_fn(i):
        calls["train"].append(i)
        opt.step()
        return 0.5 / (i + 1), 0.1 * i

    def validate_fn(i):
        calls["val"].append(i)
        return {"metric": (scores or {}).get(i, 0.0), "val_metric": "mOKS"}

    def save(model, path):
        saved[os.path.basename(path)] = opt.param_groups[0]["lr"]
        torch.save(pretrain.cpu_state_dict(model), path)
    out = pretrain.run_epochs(cfg, m, opt, train_fn, validate_fn, str(tmp_path), log=lines.append, save=save, **kw)
    return out, lines, saved, calls, opt


def test_lr_per_epoch_follows_multisteplr(tmp_path):
    out, lines, *_ = _run(_cfg(), tmp_path, snapshot=0)
    assert out["epochs"] == [0, 1, 2, 3, 4, 5, 6]
    assert out["lr"] == pytest.approx([1e-3, 1e-3, 5e-4, 5e-4, 2.5e-4, 2.5e-4, 2.5e-4])
    assert lines[0] == "epoch 0 starts, lr 0.001"


def test_dpg_step_is_shifted_by_the_milestone(tmp_path):
    from alphapose import pretrain
    y = tmp_path / "256x192_res50_lr1e-3_1x.yaml"
    y.write_text("TRAIN:\n  DPG_MILESTONE: 90\n  DPG_STEP: [110, 130]\n  LR: 0.001\nMODEL:\n  TYPE: SimplePose\n")
    cfg = pretrain.load_config(str(y))
    assert cfg.TRAIN.DPG_STEP == [20, 40]
    assert cfg.FILE_NAME == "256x192_res50_lr1e-3_1x"          # opt.py:53: everything before the first dot of the base name
    assert pretrain.work_dir_for("run7", cfg) == "./exp/run7-256x192_res50_lr1e-3_1x/"


def test_snapshot_cadence_and_best_so_far(tmp_path):
    scores = {1: 10.0, 3: 7.0, 5: 12.5}
    out, lines, saved, calls, _ = _run(_cfg(), tmp_path, scores=scores, snapshot=2)
    assert calls["val"] == [1, 3, 5]                            # (i + 1) % snapshot == 0
    assert [n for n in out["saved"] if n.startswith("model_") and n != "model_best.pth"] == ["model_1.pth", "model_3.pth", "model_5.pth"]
    assert out["saved"].count("model_best.pth") == 2            # epochs 1 and 5; 7.0 does not exceed 10.0
    assert (out["best_score"], out["best_epoch"], out["val_metric"]) == (12.5, 5, "mOKS")
    assert out["val"] == [(1, 10.0), (3, 7.0), (5, 12.5)]
    for name in ("model_1.pth", "model_3.pth", "model_5.pth", "model_best.pth", "final.pth"):
        assert (tmp_path / name).exists()
    assert not (tmp_path / "final_DPG.pth").exists()


def test_best_starts_at_zero(tmp_path):
    out, _, saved, _, _ = _run(_cfg(), tmp_path, scores={}, snapshot=1)          # every validation scores 0.0: never "exceeds"
    assert "model_best.pth" not in saved and out["best_epoch"] is None and out["best_score"] == 0


def test_milestone_saves_final_resets_lr_and_ends(tmp_path):
    out, lines, saved, calls, opt = _run(_cfg(DPG_MILESTONE=3), tmp_path, snapshot=2)
    assert out["ended"] == "dpg_milestone" and calls["train"] == [0, 1, 2, 3]
    assert saved["final.pth"] == pytest.approx(2.5e-4)          # saved before the reset, after the scheduler step of epoch 3 (both LR_STEPs passed)
    assert opt.param_groups[0]["lr"] == out["final_lr"] == 1e-3
    assert "training ends" in lines[-1] and "final.pth" in lines[-1]
    assert sorted(os.listdir(tmp_path)) == ["final.pth", "model_1.pth", "model_3.pth"]


def test_no_milestone_runs_to_end_epoch(tmp_path):
    out, *_ = _run(_cfg(DPG_MILESTONE=90, END_EPOCH=5, BEGIN_EPOCH=2), tmp_path, snapshot=0)
    assert out["ended"] == "end_epoch" and out["epochs"] == [2, 3, 4] and not os.listdir(tmp_path)


def test_max_epochs_only_shortens(tmp_path):
    out, lines, saved, calls, _ = _run(_cfg(), tmp_path, snapshot=2, max_epochs=3)
    assert out["ended"] == "max_epochs" and calls["train"] == [0, 1, 2] and calls["val"] == [1] and "final.pth" not in saved
    out, *_ = _run(_cfg(DPG_MILESTONE=1), tmp_path, snapshot=0, max_epochs=5)
    assert out["ended"] == "dpg_milestone" and out["epochs"] == [0, 1]


def test_unknown_optimiser_is_named():
    from alphapose import pretrain
    with pytest.raises(ValueError, match="'sgd'"):
        pretrain.build_optimizer(_cfg(OPTIMIZER="sgd"), Tiny().parameters())
    from active_learning import optim
    assert type(pretrain.build_optimizer(_cfg(), Tiny().parameters())) is optim.Adam
    rms = pretrain.build_optimizer(_cfg(OPTIMIZER="rmsprop", LR=3e-4), Tiny().parameters())
    assert type(rms) is optim.RMSprop
    assert rms.defaults == {"lr": 3e-4, "alpha": 0.99, "eps": 1e-8, "weight_decay": 0.0}
    assert optim.RMSprop(Tiny().parameters()).defaults["lr"] == 1e-2          # torch's constructor default
    assert optim.Adam._multi is not None


def test_epoch_info_line_and_training_log(tmp_path):
    from alphapose import pretrain
    assert pretrain.epoch_info("Train", 3, 0.00123456789, 0.98765) == "Train-3 epoch | loss:0.00123457 | acc:0.9877"
    work = str(tmp_path / "exp" / "a-b")
    logger = pretrain.make_logger(work)
    logger.info(pretrain.epoch_info("Train", 0, 1.0, 0.5))
    pretrain.close_logger(logger)
    assert open(os.path.join(work, "training.log")).read() == "Train-0 epoch | loss:1.00000000 | acc:0.5000\n"


def test_epoch_batches_keep_the_ragged_tail():
    from alphapose import pretrain
    g = torch.Generator(); g.manual_seed(5)
    b = pretrain.epoch_batches(11, 4, g)
    assert [len(x) for x in b] == [4, 4, 3] and sorted(sum(b, [])) == list(range(11)) and sum(b, []) != list(range(11))
    g.manual_seed(5)
    assert pretrain.epoch_batches(11, 4, g) == b
    assert pretrain.epoch_batches(5, 2) == [[0, 1], [2, 3], [4]]


def test_preset_model_three_branches(tmp_path):
    from alphapose import pretrain
    build = lambda node, preset_cfg: Tiny()
    lines = []
    cfg = _cfg()
    m = pretrain.preset_model(cfg, log=lines.append, build=build)
    assert m.initialized and float(m.a.weight.detach()[0, 0]) == 0.25 and lines == ["new model: _initialize()"]

    donor = Tiny()
    torch.save(donor.state_dict(), tmp_path / "full.pth")
    cfg.MODEL.PRETRAINED = str(tmp_path / "full.pth")
    m = pretrain.preset_model(cfg, log=lines.append, build=build)
    assert not m.initialized and all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), donor.state_dict().values()))
    partial = {k: v for k, v in donor.state_dict().items() if k != "b.bias"}
    torch.save(partial, tmp_path / "partial.pth")
    cfg.MODEL.PRETRAINED = str(tmp_path / "partial.pth")
    with pytest.raises(RuntimeError, match="b.bias"):           # PRETRAINED is a strict load
        pretrain.preset_model(cfg, log=lines.append, build=build)

    wide = Tiny(width=5).state_dict()                           # a.* and b.weight have other shapes; b.bias fits; one unknown name
    wide["b.bias"] = torch.full((1,), 7.0)
    wide["c.weight"] = torch.zeros(2)
    torch.save(wide, tmp_path / "wide.pth")
    cfg.MODEL.PRETRAINED, cfg.MODEL.TRY_LOAD = "", str(tmp_path / "wide.pth")
    torch.manual_seed(3)
    fresh = Tiny().state_dict()
    torch.manual_seed(3)
    m = pretrain.preset_model(cfg, log=lines.append, build=build)
    assert not m.initialized and float(m.b.bias.detach()) == 7.0
    for k in ("a.weight", "a.bias", "b.weight"):                # the wrong-shaped tensors were dropped: the module's own values stay
        assert torch.equal(m.state_dict()[k], fresh[k])


def test_module_imports_no_network_or_board_package():
    code = ("import sys; sys.path[:0] = [%r, %r]; import alphapose.pretrain as p; "
            "bad = [n for n in ('requests', 'tensorboardX', 'cachetools') if n in sys.modules]; assert not bad, bad; "
            "assert callable(p.train_epoch) and callable(p.validate) and callable(p.main)") % (ROOT, os.path.join(ROOT, "vatl4pose-wacv2024_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(ROOT, "vatl4pose-wacv2024_amd", "alphapose", "pretrain.py")).read()
    assert "cpu_count" not in src and "DataParallel(" not in src
    for name in ("requests", "tensorboardX", "cachetools"):
        assert f"import {name}" not in src and f"from {name}" not in src


def test_decode_ahead_passes_through_without_a_file_cache():
    from alphapose import pretrain

    class Plain:
        my_collate_fn = staticmethod(lambda items: items)

        def __getitem__(self, i):
            return i * 10
    d = pretrain.DecodeAhead(Plain(), workers=64, batch_size=4)
    assert d.pool is None and list(d.batches([[0, 1], [2]])) == [[0, 10], [20]]
    d.close()


def test_decode_ahead_keeps_the_frame_cache_bounded(monkeypatch):
    """A file-backed data set many times larger than its host cache, walked for two epochs with decode-ahead on: the cache never holds
    more than FRAME_CACHE frames (the data set's own eviction rule, whoever decoded the frame), every batch finds its frames decoded
    ahead, and a second epoch decodes again what the first one evicted."""
    from collections import OrderedDict
    import numpy as np
    from alphapose import pretrain
    from alphapose.datasets import coco_video
    decoded = []

    def fake_read(path):
        decoded.append(path)
        return np.zeros((2, 2, 3), np.uint8)
    monkeypatch.setattr(coco_video, "_read_rgb", fake_read)

    class FileBacked(coco_video._CocoVideo):
        FRAME_CACHE = 4

        def __init__(self, n):                                   # (the cache and the labels only: no annotation file, no device)
            self._labels = [{"frame": f"frame{i:03d}.png"} for i in range(n)]
            self._decoded = OrderedDict()
            self.peak, self.misses = 0, 0

        def collated(self, idxs):
            for i in idxs:
                before = len(decoded)
                self._frame(self._labels[i]["frame"])
                self.misses += len(decoded) - before
            self.peak = max(self.peak, len(self._decoded))
            return list(idxs)

    ds = FileBacked(40)
    ahead = pretrain.DecodeAhead(ds, workers=2, batch_size=3)
    assert ahead.workers == 2 and ds.FRAME_CACHE == 12           # room for 4 batches' frames, asked for through the data set
    for epoch in range(2):
        lists = pretrain.epoch_batches(40, 3)
        assert list(ahead.batches(lists)) == lists
        assert len(ds._decoded) <= 12
    ahead.close()
    assert ds.peak <= 12
    assert ds.misses == 2 * 3                                    # only the first batch of an epoch is decoded on the calling thread
    assert len(decoded) == 80 and len(set(decoded)) == 40        # epoch 2 decoded again what epoch 1's later frames had evicted
    ds.cache_frames({f"extra{i}": np.zeros((1, 1, 3), np.uint8) for i in range(30)})
    assert len(ds._decoded) == 12 and next(reversed(ds._decoded)) == "extra29"
