"""The host side of the opt-in graphed fine-tune step that needs no device: the ``RETRAIN.GRAPH`` key and the dependency key of a
captured step (alphapose/models/hip_train_graph.py)."""
import types

import pytest


def _cfg(**retrain):
    from alphapose.utils.config import edict
    return edict({
        "DATASET": {"TRAIN": {"TYPE": "SyntheticVideo", "NUM_ITEMS": 24, "TRACKS": 2}, "EVAL": {"TYPE": "SyntheticVideo", "NUM_ITEMS": 24, "TRACKS": 2}},
        "DATA_PRESET": {"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]},
        "MODEL": {"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50},
        "LOSS": {"TYPE": "MSELoss"},
        "AE": {"Z_DIM": 4, "INPUT_DIM": 42, "PRETRAINED": "", "EPOCH": 2, "LR": 1e-3},
        "RETRAIN": dict({"BATCH_SIZE": 8, "BASE": 1, "OPTIMIZER": "AdamW", "LR": 2.5e-4, "ALPHA": 2, "WEIGHT_DECAY": 0.7, "LR_GAMMA": 0.99}, **retrain),
        "VAL": {"BATCH_SIZE": 10, "W_UNC": 0.01, "UNC_LAMBDA": 0.01, "QUERY_RATIO": [0.25, 0.5, 1.0]},
    })


def test_retrain_graph_parsing():
    from active_learning.ActiveLearning import retrain_graph
    from alphapose.utils.config import edict
    assert retrain_graph(_cfg()) is False                              # absent -> today's loop
    assert retrain_graph(edict({"MODEL": {"TYPE": "SimplePose"}})) is False
    assert retrain_graph(_cfg(GRAPH=False)) is False
    assert retrain_graph(_cfg(GRAPH=True)) is True
    assert retrain_graph(_cfg(GRAPH="auto")) == "auto"


@pytest.mark.parametrize("bad", [1.5, "yes", None])
def test_retrain_graph_rejects_other_values(bad):
    from active_learning.ActiveLearning import retrain_graph
    with pytest.raises(ValueError, match="RETRAIN.GRAPH"):
        retrain_graph(_cfg(GRAPH=bad))


def test_constructor_rejects_a_bad_key_before_it_touches_the_device(monkeypatch):
    """No GPU here: any device call would raise something else.  To be sure, the first things the constructor does after parsing the
    keys — joining / starting worker ranks and asking for the current device — are made to fail loudly."""
    import torch

    from active_learning import ActiveLearning
    from active_learning import distributed as D

    def touched(*a, **k):
        raise AssertionError("the constructor went past the key parsers")
    monkeypatch.setattr(D, "ensure_workers", touched)
    monkeypatch.setattr(torch.cuda, "current_device", touched)
    opt = types.SimpleNamespace(uncertainty="HP", representativeness="None", filter="None", strategy="HP", video_id="syn", get_prenext=True,
                                from_scratch=True, continual=True, num_gpu=1, onebyone=False, retrain_thresh=1, THCvsWPU="const")
    with pytest.raises(ValueError, match="RETRAIN.GRAPH"):
        ActiveLearning(_cfg(GRAPH="yes"), opt, eval_dataset=object(), train_dataset=object())


# ------------------------------------------------------------------------------------------------------------------ the dependency key
BASE = dict(ptrs=(0x7000, 0x7400, 0x9000), trainable=(True, True), training=True, device="cuda:0", shape=(3, 3, 64, 64), dtype="torch.float32",
            constants=(True, True, False, 128, 128, True, True, True, None))
# one change per item of the list a captured step depends on
CHANGES = {
    "a parameter's storage": dict(ptrs=(0x7000, 0x7800, 0x9000)),
    "a buffer's storage": dict(ptrs=(0x7000, 0x7400, 0x9400)),
    "the trainable set": dict(trainable=(True, False)),
    "the train flag": dict(training=False),
    "the device": dict(device="cuda:1"),
    "the input shape": dict(shape=(2, 3, 64, 64)),
    "the input dtype": dict(dtype="torch.float64"),
    **{f"route constant {i}": dict(constants=tuple((not v if isinstance(v, bool) else (True if v is None else v + 1)) if j == i else v
                                                   for j, v in enumerate(BASE["constants"])))
       for i in range(len(BASE["constants"]))},
}


def test_dependency_key_is_a_pure_function_of_its_arguments():
    from alphapose.models.hip_train_graph import dependency_key
    k0 = dependency_key(**BASE)
    hash(k0)
    assert dependency_key(**BASE) == k0
    # the same facts in other containers / spellings are the same key: nothing else (identity of the lists, a torch.Size, ...) enters it
    import torch
    same = dict(BASE, ptrs=list(BASE["ptrs"]), trainable=list(BASE["trainable"]), shape=torch.Size(BASE["shape"]), dtype=torch.float32, training=1,
                constants=list(BASE["constants"]))
    assert dependency_key(**same) == k0


@pytest.mark.parametrize("what", list(CHANGES))
def test_dependency_key_changes_with_every_item_a_graph_depends_on(what):
    from alphapose.models.hip_train_graph import dependency_key
    assert dependency_key(**dict(BASE, **CHANGES[what])) != dependency_key(**BASE), what


def test_route_constants_name_every_constant_of_the_issue():
    """``route_constants`` reads the module attributes the trainers read; flipping each moves exactly its own entry."""
    from alphapose.models import hip_train, hip_train_graph, hip_train_h16
    names = [(hip_train, "_FUSE_BN_BWD"), (hip_train, "_WINOGRAD"), (hip_train, "_WINOGRAD_F4"), (hip_train, "_WINOGRAD_WGRAD_MIN_C"),
             (hip_train, "_FUSE_BN_MIN_C"), (hip_train, "_USE_PACK_PLAN"), (hip_train._side, "enabled"), (hip_train_graph, "SIDE_STREAM_IN_GRAPH"),
             (hip_train_h16, "_USE_PACK_PLAN")]
    base = hip_train_graph.route_constants("bf16")
    assert len(base) == len(names) == len(BASE["constants"])
    assert hip_train_graph.route_constants("fp32") == base[:-1] + (None,)      # the fp32 trainers never read the bf16 plan switch
    for i, (mod, attr) in enumerate(names):
        keep = getattr(mod, attr)
        setattr(mod, attr, (not keep) if isinstance(keep, bool) else keep + 1)
        try:
            now = hip_train_graph.route_constants("bf16")
        finally:
            setattr(mod, attr, keep)
        assert [j for j in range(len(base)) if now[j] != base[j]] == [i], attr
    assert hip_train_graph.route_constants("bf16") == base
