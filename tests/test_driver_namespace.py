"""The namespace the unchanged driver (scripts/Run_active_learning.py: parse_args -> setup_opt -> update_config -> set_dir)
hands the constructor, pinned from the reference itself (tests/golden/driver_namespace.json, tools/make_driver_golden.py):
the video's annotation / frame paths the constructor derives (ActiveLearning.py:55, 67-94) and the WPU auto-encoder
checkpoint it loads (:886-903).  CPU only."""
import copy
import json
import os
import types

import pytest
import torch

from tests.conftest import GOLDEN

with open(os.path.join(GOLDEN, "driver_namespace.json")) as _f:
    CASES = json.load(_f)["cases"]


def _cfg(d):
    from alphapose.utils.config import edict
    return edict(copy.deepcopy(d))


def _opt(case, **over):
    return types.SimpleNamespace(**{**case["opt"], **over})


def _lay_out(case, root):
    """The reference's working directory for one case: the JRDB scene lists it read, and an (empty) auto-encoder checkpoint file."""
    for path, lines in case["jrdb_lines"].items():
        os.makedirs(os.path.join(root, os.path.dirname(path)), exist_ok=True)
        with open(os.path.join(root, path), "w") as f:
            f.write("".join(lines))
    os.makedirs(os.path.join(root, os.path.dirname(case["ae_path"])), exist_ok=True)
    open(os.path.join(root, case["ae_path"]), "wb").close()


def _save_ae(path, input_dim=42, z_dim=4, seed=0):
    from active_learning.Whole_body_AE.AutoEncoder import WholeBodyAE
    torch.manual_seed(seed)
    ae = WholeBodyAE(z_dim=z_dim, input_dim=input_dim)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    torch.save(ae.state_dict(), path)
    return ae.state_dict()


def test_fixture_covers_the_driver_cases():
    kinds = {(c["cfg_before"]["DATASET"]["EVAL"]["TYPE"], c["opt"]["optimize"], c["opt"]["PCIT"]) for c in CASES.values()}
    assert {("Posetrack21", False, False), ("Posetrack21", True, False), ("Posetrack21", False, True),
            ("JRDB2022", False, False), ("JRDB2022", True, False)} <= kinds
    assert any(c["opt"]["uncertainty"] == "None" and c["opt"]["representativeness"] != "None" for c in CASES.values())
    for c in CASES.values():
        assert c["cfg_before"]["DATASET"]["EVAL"]["ANN"] == "" and c["cfg_before"]["DATASET"]["EVAL"]["IMG_PREFIX"] == ""


@pytest.mark.parametrize("name", sorted(CASES))
def test_derived_paths_match_the_reference(name, tmp_path, monkeypatch):
    from active_learning.driver_paths import derive_video_paths, resolve_ae_checkpoint
    case = CASES[name]
    _lay_out(case, str(tmp_path))
    monkeypatch.chdir(tmp_path)
    cfg, opt = _cfg(case["cfg_before"]), _opt(case)
    got = derive_video_paths(cfg, opt)
    for split in ("EVAL", "TRAIN"):
        for key in ("ROOT", "IMG_PREFIX", "ANN"):
            assert cfg.DATASET[split][key] == case["derived"][split][key], (split, key)
    assert got == {"IMG_PREFIX": case["derived"]["EVAL"]["IMG_PREFIX"], "ANN": case["derived"]["EVAL"]["ANN"]}
    assert cfg == case["cfg_after"]                                     # nothing else touched
    assert resolve_ae_checkpoint(cfg) == case["ae_path"]


@pytest.mark.parametrize("name", ["a_posetrack", "b_posetrack_optimize", "d_jrdb"])
def test_second_video_on_the_same_config_is_derived_again(name, tmp_path, monkeypatch):
    """--optimize: hyper_objective constructs one object per video on the SAME (already derived) config."""
    from active_learning.driver_paths import derive_video_paths
    case = CASES[name]
    _lay_out(case, str(tmp_path))
    monkeypatch.chdir(tmp_path)
    cfg = _cfg(case["cfg_before"])
    derive_video_paths(cfg, _opt(case))
    assert cfg.DATASET.EVAL.ANN == case["derived"]["EVAL"]["ANN"]
    other = "01" if case["opt"]["video_id"] == "00" else "000522"
    derive_video_paths(cfg, _opt(case, video_id=other))
    fresh = _cfg(case["cfg_before"])
    derive_video_paths(fresh, _opt(case, video_id=other))
    assert other in cfg.DATASET.EVAL.ANN and case["opt"]["video_id"] not in cfg.DATASET.EVAL.ANN.replace(other, "")
    assert cfg == fresh


def test_explicit_annotation_file_is_kept():
    from active_learning.driver_paths import derive_video_paths
    case = CASES["a_posetrack"]
    cfg = _cfg(case["cfg_before"])
    for split in ("EVAL", "TRAIN"):
        cfg.DATASET[split].ANN, cfg.DATASET[split].IMG_PREFIX = "annotations/val.json", ""
    before = copy.deepcopy(cfg)
    assert derive_video_paths(cfg, _opt(case)) == {}
    assert cfg == before


@pytest.mark.parametrize("kind", ["FrameVideo", "SyntheticVideo"])
def test_other_dataset_types_are_untouched(kind):
    from active_learning.driver_paths import derive_video_paths
    case = CASES["a_posetrack"]
    cfg = _cfg(case["cfg_before"])
    cfg.DATASET.EVAL.TYPE = cfg.DATASET.TRAIN.TYPE = kind
    before = copy.deepcopy(cfg)
    assert derive_video_paths(cfg, _opt(case)) == {}
    assert derive_video_paths(cfg, types.SimpleNamespace(uncertainty="HP")) == {}      # callers of these types need no video id
    assert cfg == before


@pytest.mark.parametrize("name", ["d_jrdb", "e_jrdb_optimize"])
def test_missing_jrdb_scene_list_raises(name, tmp_path, monkeypatch):
    from active_learning.driver_paths import derive_video_paths
    case = CASES[name]
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError, match="jrdb_val.txt" if case["opt"]["optimize"] else "jrdb_test.txt"):
        derive_video_paths(_cfg(case["cfg_before"]), _opt(case))


# ---------------------------------------------------------------------------------------------- WPU auto-encoder checkpoint

def _ae_cfg(**ae):
    from alphapose.utils.config import edict
    return edict({"AE": {"Z_DIM": 4, "EPOCH": 20, "LR": 8e-5, **ae}})


@pytest.mark.parametrize("input_dim", [42, 38])
def test_checkpoint_under_pretrained_root_is_found_and_its_width_inferred(input_dim, tmp_path, monkeypatch):
    from active_learning.driver_paths import load_ae_checkpoint, resolve_ae_checkpoint
    monkeypatch.chdir(tmp_path)
    cfg = _ae_cfg(PRETRAINED_ROOT="pretrained_models/wholebodyAE/Posetrack21")
    want = _save_ae("pretrained_models/wholebodyAE/Posetrack21/Hybrid/WholeBodyAE_zdim4.pth", input_dim=input_dim)
    path = resolve_ae_checkpoint(cfg)
    assert path == CASES["a_posetrack"]["ae_path"]
    sd, d, z = load_ae_checkpoint(path, cfg)
    assert (d, z) == (input_dim, 4)
    assert list(sd) == list(want) and all(torch.equal(sd[k], want[k]) for k in want)


def test_checkpoint_shape_disagreements_raise(tmp_path):
    from active_learning.driver_paths import load_ae_checkpoint
    path = str(tmp_path / "ae.pth")
    _save_ae(path, input_dim=42, z_dim=4)
    with pytest.raises(ValueError, match="z_dim"):
        load_ae_checkpoint(path, _ae_cfg(Z_DIM=2))
    with pytest.raises(ValueError, match="INPUT_DIM"):
        load_ae_checkpoint(path, _ae_cfg(INPUT_DIM=38))
    assert load_ae_checkpoint(path, _ae_cfg(INPUT_DIM=42))[1:] == (42, 4)


def test_missing_checkpoint_under_pretrained_root_raises(tmp_path, monkeypatch):
    from active_learning.driver_paths import resolve_ae_checkpoint
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError, match=r"WholeBodyAE_zdim4\.pth.*AE\.PRETRAINED_ROOT"):
        resolve_ae_checkpoint(_ae_cfg(PRETRAINED_ROOT="pretrained_models/wholebodyAE/Posetrack21"))


def test_explicit_pretrained_takes_precedence(tmp_path, monkeypatch):
    from active_learning.driver_paths import resolve_ae_checkpoint
    monkeypatch.chdir(tmp_path)
    _save_ae("mine.pth")
    assert resolve_ae_checkpoint(_ae_cfg(PRETRAINED="mine.pth", PRETRAINED_ROOT="pretrained_models/wholebodyAE/Posetrack21")) == "mine.pth"


def test_no_checkpoint_key_means_random_initialisation():
    from active_learning.driver_paths import resolve_ae_checkpoint
    assert resolve_ae_checkpoint(_ae_cfg()) is None
    assert resolve_ae_checkpoint(_ae_cfg(PRETRAINED="")) is None


def test_initialize_ae_loads_the_checkpoint_once_per_construction(tmp_path, monkeypatch):
    """Every fine-tune round restarts from the checkpoint (retrain_model calls initialize_AE again); the file is read once."""
    from active_learning import ActiveLearning
    monkeypatch.chdir(tmp_path)
    case = CASES["a_posetrack"]
    cfg = _cfg(case["cfg_before"])
    want = _save_ae(os.path.join(cfg.AE.PRETRAINED_ROOT, "Hybrid", "WholeBodyAE_zdim4.pth"), input_dim=42)
    loads = []
    real = torch.load
    monkeypatch.setattr(torch, "load", lambda *a, **k: loads.append(a[0]) or real(*a, **k))
    stand_in = types.SimpleNamespace(cfg=cfg, device=torch.device("cpu"))
    for _ in range(2):
        ae = ActiveLearning.initialize_AE(stand_in)
        assert (ae.input_dim, ae.z_dim) == (42, 4)
        assert all(torch.equal(ae.state_dict()[k], want[k]) for k in want)
        with torch.no_grad():
            ae.encoder[0].weight.add_(1.0)                          # a fine-tune of the previous round must not leak into the next
    assert loads == [case["ae_path"]]


def test_initialize_ae_refuses_random_weights_when_a_checkpoint_was_asked_for(tmp_path, monkeypatch):
    from active_learning import ActiveLearning
    monkeypatch.chdir(tmp_path)
    stand_in = types.SimpleNamespace(cfg=_cfg(CASES["d_jrdb"]["cfg_before"]), device=torch.device("cpu"))
    with pytest.raises(FileNotFoundError, match="JRDB2022/Hybrid/WholeBodyAE_zdim4.pth"):
        ActiveLearning.initialize_AE(stand_in)
