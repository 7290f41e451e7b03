"""``TRAIN.PRECISION`` / ``--precision`` of alphapose/pretrain.py without a GPU: what the key admits, what overrides what, and that a
refusal comes before any data set is built."""
import json

import pytest


def _cfg(precision="absent", model="SimplePose"):
    from alphapose.utils.config import edict
    train = {"BATCH_SIZE": 4, "BEGIN_EPOCH": 0, "END_EPOCH": 2, "OPTIMIZER": "adam", "LR": 1e-3, "LR_FACTOR": 0.1, "LR_STEP": [1],
             "DPG_MILESTONE": 1, "DPG_STEP": [2, 3]}
    if precision != "absent":
        train["PRECISION"] = precision
    mcfg = {"TYPE": model, "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50}
    if model == "SimplePose":
        mcfg["NUM_DECONV_FILTERS"] = [256, 256, 256]
    ds = {"TYPE": "Posetrack21", "ROOT": "/nonexistent", "IMG_PREFIX": "", "ANN": "none.json"}
    return edict({"DATASET": {"TRAIN": dict(ds), "VAL": dict(ds)}, "MODEL": mcfg, "TRAIN": train,
                  "DATA_PRESET": {"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]},
                  "VAL": {"BATCH_SIZE": 4}})


def _yaml(tmp_path, cfg):
    import yaml
    path = tmp_path / "tiny_pre.yaml"
    path.write_text(yaml.safe_dump(json.loads(json.dumps(cfg))))
    return str(path)


def test_absent_key_means_fp32():
    from alphapose import pretrain
    from alphapose.utils.config import edict
    assert pretrain.train_precision(_cfg()) == "fp32"
    assert pretrain.train_precision(_cfg(model="FastPose")) == "fp32"
    assert pretrain.train_precision(edict({"MODEL": {"TYPE": "SimplePose"}})) == "fp32"        # no TRAIN node at all


@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_both_precisions_pass_through_for_simplepose(name):
    from alphapose import pretrain
    assert pretrain.train_precision(_cfg(name)) == name
    assert pretrain.train_precision(_cfg(), override=name) == name


@pytest.mark.parametrize("model", ["FastPose", "PoseHighResolutionNet"])
def test_bf16_is_refused_for_other_networks_by_name(model):
    from alphapose import pretrain
    with pytest.raises(NotImplementedError, match=f"TRAIN.PRECISION.*{model}"):
        pretrain.train_precision(_cfg("bf16", model=model))
    with pytest.raises(NotImplementedError, match=f"TRAIN.PRECISION.*{model}"):
        pretrain.train_precision(_cfg("fp32", model=model), override="bf16")
    assert pretrain.train_precision(_cfg("fp32", model=model)) == "fp32"


@pytest.mark.parametrize("value", ["fp16", "fp8", 16, None])
def test_any_other_value_is_a_value_error_naming_the_key(value):
    from alphapose import pretrain
    with pytest.raises(ValueError, match="TRAIN.PRECISION"):
        pretrain.train_precision(_cfg(value))


def test_an_unknown_override_is_a_value_error_too():
    from alphapose import pretrain
    with pytest.raises(ValueError, match="TRAIN.PRECISION"):
        pretrain.train_precision(_cfg("bf16"), override="fp16")
    with pytest.raises(ValueError, match="TRAIN.PRECISION"):
        pretrain.train_epoch(None, [], None, precision="fp16")                   # refused before the model is looked at


def test_flag_overrides_the_yaml_key_and_an_absent_flag_leaves_it(tmp_path):
    from alphapose import pretrain
    path = _yaml(tmp_path, _cfg("fp32"))
    opt = pretrain.parse_args(["--cfg", path, "--precision", "bf16"])
    assert opt.precision == "bf16"
    assert pretrain.train_precision(pretrain.load_config(path), opt.precision) == "bf16"
    opt = pretrain.parse_args(["--cfg", path])
    assert opt.precision is None
    assert pretrain.train_precision(pretrain.load_config(path), opt.precision) == "fp32"
    path = _yaml(tmp_path, _cfg("bf16"))
    assert pretrain.train_precision(pretrain.load_config(path), pretrain.parse_args(["--cfg", path]).precision) == "bf16"
    assert pretrain.train_precision(pretrain.load_config(path), pretrain.parse_args(["--cfg", path, "--precision", "fp32"]).precision) == "fp32"
    with pytest.raises(SystemExit):
        pretrain.parse_args(["--cfg", path, "--precision", "fp16"])


def test_main_refuses_before_a_data_set_is_built(tmp_path, monkeypatch):
    from alphapose import pretrain
    built = []
    monkeypatch.setattr(pretrain.builder, "build_dataset", lambda *a, **k: built.append(a) or (_ for _ in ()).throw(AssertionError("data set built")))
    monkeypatch.setattr(pretrain.builder, "build_sppe", lambda *a, **k: built.append(a) or (_ for _ in ()).throw(AssertionError("model built")))
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError, match="TRAIN.PRECISION.*FastPose"):
        pretrain.main(["--cfg", _yaml(tmp_path, _cfg(model="FastPose")), "--exp-id", "x", "--precision", "bf16"])
    with pytest.raises(ValueError, match="TRAIN.PRECISION"):
        pretrain.main(["--cfg", _yaml(tmp_path, _cfg("fp16")), "--exp-id", "x"])
    assert not built
    assert not (tmp_path / "exp").exists()                                       # no work dir, no log file either
