"""The opt-in graphed fine-tune step (alphapose/models/hip_train_graph.py, ``cfg.RETRAIN.GRAPH``): a captured and replayed step gives the
eager step's bits — loss, heat-maps, every gradient, every parameter after the optimiser, every BatchNorm buffer — on the smallest shapes
of tests/train_step_cases.py / tests/train_tape_cases.py.  What can go wrong here is wiring (a stale pointer, a missed host-side version
bump, a dropped fork / join), not arithmetic: every step gets another batch, so a replay that ignored its inputs fails."""
import sys
import types

import numpy as np
import pytest
import torch

from oracle import synth
from tests import train_step_cases, train_tape_cases
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu

# name -> (network of train_step_cases, (B, H, W) of the crops, precision, optimiser)
CASES = {
    "simplepose": ("simplepose", (3, 64, 64), "fp32", "adamw3"),
    "fastpose": ("fastpose", (2, 128, 96), "fp32", "adamw"),
    "hrnet": ("hrnet", (2, 128, 96), "fp32", "sgd"),
    "simplepose_bf16": ("simplepose", train_tape_cases.SHAPES[0], "bf16", "adamw3"),
}


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


_batches = {}


def _batch(shape, k, precision="fp32"):
    """Batch ``k`` of a shape: seeded, computed once, never written."""
    key = (shape, k, precision)
    if key not in _batches:
        b, h, w = shape
        hm = train_tape_cases.heatmap_hw(h, w) if precision == "bf16" else (h // 4, w // 4)
        x = synth.crops(b, seed=161 + k, hw=(h, w))
        labels, masks = synth.gaussian_targets(b, seed=262 + k, hw=hm)
        _batches[key] = tuple(torch.from_numpy(np.ascontiguousarray(t)).float().to(dev()) for t in (x, labels, masks))
    return _batches[key]


def _optimiser(m, which):
    from active_learning.optim import SGD, AdamW
    if which == "adamw3":                               # the three groups the active-learning loop builds for SimplePose
        groups = [{"params": getattr(m, a).parameters(), "lr": 2.5e-4 * f} for a, f in (("final_layer", 10), ("preact", 1), ("deconv_layers", 5))]
        return AdamW(params=groups, weight_decay=0.7)
    if which == "adamw":
        return AdamW(m.parameters(), lr=2.5e-4, weight_decay=0.7)
    return SGD(m.parameters(), lr=2.5e-4, momentum=0.9, weight_decay=5e-4)


class Twins:
    """Two models from one seed with an optimiser each: ``e`` takes the eager sequence, ``g`` the graphed step.  ``step(batch)`` runs
    one optimiser step on both and demands equal bits everywhere."""

    def __init__(self, vh, kind, precision, optimiser):
        from alphapose.models import hip_train, hip_train_graph
        self.vh, self.precision = vh, precision
        self.e, self.g = train_step_cases.model(kind, dev()), train_step_cases.model(kind, dev())
        for a, b in zip(self.e.state_dict().values(), self.g.state_dict().values()):
            assert torch.equal(a, b)
        self.oe, self.og = _optimiser(self.e, optimiser), _optimiser(self.g, optimiser)
        self.graphed = hip_train_graph.graphed_step_for(self.g, precision)
        assert hip_train_graph.graphed_step_for(self.g, precision) is self.graphed                   # cached on the model
        self.arena = hip_train.arena_for
        self.steps = 0

    def _eager(self, x, labels, masks):
        from alphapose.models import hip_train
        if self.precision == "bf16":
            from alphapose.models import hip_train_h16
            tr = hip_train_h16.trainer_for_h16(self.e)
        else:
            tr = hip_train.trainer_for(self.e)
        arena = hip_train.arena_for(self.e)
        with torch.no_grad():
            out = tr.forward(x)
            loss, dout = self.vh.masked_mse_fwd_bwd(out, labels, masks)
            arena.begin()
            tr.backward(dout, arena=arena, overlap=True)
            arena.finish()
        return out, loss

    def step(self, batch):
        x, labels, masks = batch
        oe, le = self._eager(x, labels, masks)
        og, lg = self.graphed(x, labels, masks)
        path = self.graphed.path
        self.steps += 1
        what = f"step {self.steps} ({path})"
        assert lg.dim() == 0 and torch.equal(lg, le.reshape(())), what
        assert torch.equal(og, oe), what
        ae, ag = self.arena(self.e), self.arena(self.g)
        assert torch.equal(ag.flat, ae.flat), what
        ae.attach(); ag.attach()
        self.oe.step(); self.og.step()
        for (k, a), b in zip(self.e.named_parameters(), self.g.parameters()):
            assert torch.equal(a, b), (what, k)
        for (k, a), b in zip(self.e.named_buffers(), self.g.buffers()):                      # num_batches_tracked included
            assert torch.equal(a, b), (what, k)
        return path


@pytest.mark.parametrize("side", [True, False], ids=["forked", "linear"])
@pytest.mark.parametrize("case", list(CASES))
def test_replay_equals_eager_and_the_inference_plans_see_it(vh, case, side, monkeypatch):
    """Four optimiser steps, each on another batch: eager warm-up, capture + replay, replay, replay — with the weight gradients forked
    onto the side stream inside the graph and as a linear graph.  Then both models go to eval(): the inference plans, which key their
    packed weights and folded BatchNorm statistics on version counters, must see the replayed steps like eager ones."""
    from alphapose.models import hip_engine, hip_train_graph
    kind, shape, precision, optimiser = CASES[case]
    monkeypatch.setattr(hip_train_graph, "SIDE_STREAM_IN_GRAPH", side)
    t = Twins(vh, kind, precision, optimiser)
    bn_e = next(m for m in t.e.modules() if isinstance(m, torch.nn.BatchNorm2d))
    bn_g = next(m for m in t.g.modules() if isinstance(m, torch.nn.BatchNorm2d))
    v_e, v_g = bn_e.running_mean._version, bn_g.running_mean._version
    paths = [t.step(_batch(shape, k, precision)) for k in range(4)]
    print(case, "forked" if side else "linear", paths, t.graphed.stats)
    assert paths == ["eager:warm", "captured", "replayed", "replayed"], paths
    assert t.graphed.stats == {"eager": 1, "captured": 1, "replayed": 2}
    assert bn_e.running_mean._version - v_e == 4 and bn_g.running_mean._version - v_g == 4
    t.e.eval(); t.g.eval()
    x = _batch(shape, 0, precision)[0]
    hm = _batch(shape, 0, precision)[1].shape
    with torch.no_grad():
        he = hip_engine.forward_into(t.e, x, torch.empty(hm, device=x.device))
        hg = hip_engine.forward_into(t.g, x, torch.empty(hm, device=x.device))
    assert torch.equal(he, hg) and bool(torch.isfinite(hg).all())


def _until_captured(t, shape, k0, limit=4):
    """Steps on batch shape ``shape`` until one is captured -> the paths (a changed route may want one more eager step than a fresh
    model: the pack plan re-records when it meets a layout or a storage it had not seen)."""
    paths = []
    for k in range(limit):
        paths.append(t.step(_batch(shape, k0 + k)))
        if paths[-1] == "captured":
            return paths
    raise AssertionError(paths)


def test_shapes_and_invalidation(vh):
    """Two batch shapes keep two graphs; a parameter that moved to other storage, and a changed route constant, start the life cycle
    again; an in-place load_state_dict keeps the graph.  Equal bits to the eager twin, run under the same settings, throughout."""
    from alphapose.models import hip_train
    t = Twins(vh, "simplepose", "fp32", "adamw3")
    big, small = (3, 64, 64), (2, 64, 64)
    paths = [t.step(_batch(s, k)) for k, s in enumerate((big, small, big, small, big))]
    assert paths == ["eager:warm", "eager:warm", "captured", "captured", "replayed"], paths
    assert t.step(_batch(small, 5)) == "replayed"
    # storage of one parameter replaced (both models alike): the graph's pointers are stale
    for m in (t.e, t.g):
        p = m.final_layer.weight
        p.data = p.data.clone()
    assert t.step(_batch(big, 6)) == "eager:warm"
    assert _until_captured(t, big, 7)[:-1] in ([], ["eager:warm"])
    assert t.step(_batch(big, 11)) == "replayed"
    # values replaced in place: same storage, the graph stays
    for m in (t.e, t.g):
        sd = {k: (v * 1.001 if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()}
        m.load_state_dict(sd)
    assert t.step(_batch(big, 12)) == "replayed"
    # a route constant the trainer reads
    keep = hip_train._FUSE_BN_BWD
    hip_train._FUSE_BN_BWD = False
    try:
        assert t.step(_batch(big, 13)) == "eager:warm"
        assert _until_captured(t, big, 14)[:-1] in ([], ["eager:warm"])
        assert t.step(_batch(big, 18)) == "replayed"
    finally:
        hip_train._FUSE_BN_BWD = keep
    assert t.step(_batch(big, 19)) == "eager:warm"                                         # ... and back
    assert not t.graphed.reasons


@pytest.mark.parametrize("why", ["relu_tap", "streamk", "dcn"])
def test_cases_that_stay_eager(vh, why, monkeypatch):
    """What a graph does not cover runs eagerly, says so, is never captured — and gives the eager twin's bits."""
    from alphapose.models import hip_train
    kind, shape = ("fastpose_dcn", (2, 128, 96)) if why == "dcn" else ("simplepose", (3, 64, 64))
    keep = vh.deform_deterministic_mode()
    try:
        if why == "relu_tap":
            monkeypatch.setattr(hip_train, "_relu_tap", [])
        elif why == "streamk":
            monkeypatch.setattr(vh, "STREAMK_IN_TRAINING", True)
        else:
            from alphapose.models.layers import dcn
            dcn.set_deterministic(True)                                                    # the bit-reproducible deformable backward
        t = Twins(vh, kind, "fp32", "adamw")
        paths = [t.step(_batch(shape, k)) for k in range(3)]
    finally:
        vh.set_deform_deterministic(keep)
    print(why, paths)
    assert all(p.startswith("eager:") and p != "eager:warm" for p in paths), paths
    assert t.graphed.stats == {"eager": 3, "captured": 0, "replayed": 0} and t.graphed.reasons == [paths[0]]


def _one_cycle(graph):
    """eval_and_query -> outcome -> eval_and_query of the synthetic set-up of tests/test_gpu_al.py, ``RETRAIN.GRAPH`` absent or as given."""
    from active_learning import ActiveLearning
    from tests.test_gpu_al import _cfg
    cfg = _cfg()
    cfg.RETRAIN.ALPHA = 5                                  # int(5 * (1 - mOKS of the queried items)) epochs of one 6-crop step: warm, capture, replays
    if graph is not None:
        cfg.RETRAIN.GRAPH = graph
    opt = types.SimpleNamespace(uncertainty="THC_L1", representativeness="None", filter="None", strategy="THC_L1", video_id="syn", get_prenext=True,
                                from_scratch=True, continual=True, num_gpu=1, onebyone=False, retrain_thresh=1, THCvsWPU="const", fixed_lambda=False)
    torch.manual_seed(0); np.random.seed(0)
    al = ActiveLearning(cfg, opt)
    al.eval_and_query()
    assert al.outcome() is None
    al.eval_and_query()
    return al


def test_active_learning_cycle_with_graphed_steps():
    name = "alphapose.models.hip_train_graph"
    loaded = sys.modules.pop(name, None)                   # (earlier tests of this file imported it)
    try:
        plain = _one_cycle(None)
        assert name not in sys.modules and not hasattr(plain, "retrain_graph")
    finally:
        if loaded is not None:
            sys.modules[name] = loaded
    graphed = _one_cycle(True)
    print("retrain_graph:", graphed.retrain_graph, "epochs:", graphed.retrain_epoch)
    assert graphed.retrain_epoch == plain.retrain_epoch >= 3
    assert graphed.retrain_graph["replayed"] > 0 and graphed.retrain_graph["captured"] == 1 and graphed.retrain_graph["reasons"] == []
    assert graphed.retrain_graph["replayed"] + graphed.retrain_graph["captured"] + graphed.retrain_graph["eager"] == graphed.retrain_epoch
    assert graphed.last_train_loss == plain.last_train_loss and graphed.last_train_acc == plain.last_train_acc
    assert graphed.query_list_list == plain.query_list_list and len(plain.query_list_list) == 2
    sp, sg = plain.model.state_dict(), graphed.model.state_dict()
    assert list(sp) == list(sg)
    for k in sp:
        assert torch.equal(sp[k], sg[k]), k
