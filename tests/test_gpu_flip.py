"""Opt-in flip testing on the device: csrc/flip.hip against the reference's own outputs (tests/golden/flip_test.npz, cases and numpy
model in tests/flip_cases.py), `hip_engine_flip.flip_forward_into` against the same thing built from the existing public calls, and the
two products that can switch it on (`cfg.VAL.FLIP_TEST` of ActiveLearning, `--flip-test` of alphapose.pretrain).

"Composition" below is always

    (forward(x) + flip_heatmap(forward(flip(x)), joint_pairs, shift=True)) / 2

with `flip` / `flip_heatmap` of alphapose/utils/transforms.py (the restatement of the reference's helpers as torch indexing) and `forward`
an entry point that exists without this feature.  The networks run on 256x192 crops: 64x48 heat-maps, the product's size.
"""
import functools
import json
import types

import numpy as np
import pytest
import torch

from tests import flip_cases as FC
from tests.gpu_util import dev, to_dev
from tests.test_gpu_widepin import _build

pytestmark = pytest.mark.gpu

COCO = [list(p) for p in FC.COCO_PAIRS]


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


@pytest.fixture(scope="module")
def golden():
    return np.load(FC.GOLDEN)


def _stored(golden, key, a):
    want = golden[key]
    a = a.cpu().numpy()
    if want.dtype.kind == "U":
        return FC.digest(a) == str(want)
    return FC.same_bits(a, want)


def _misaligned(a):
    """The same values in a contiguous device tensor that starts 4 bytes past a 16-byte boundary: the thread-per-pixel kernels."""
    buf = torch.empty(a.size + 4, device=dev())
    assert buf.data_ptr() % 16 == 0
    t = buf[1:1 + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    return t


# ------------------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_flip_nchw_mirrors_every_case(vh, golden, name):
    hm, _ = FC.inputs(name)
    for x in (to_dev(hm), _misaligned(hm)):
        y = vh.flip_nchw(x)
        assert y.shape == x.shape and y.dtype == torch.float32 and y.data_ptr() != x.data_ptr()
        assert torch.equal(y.view(torch.int32), x.flip(-1).view(torch.int32))
        assert _stored(golden, f"{name}.flip", y)
        out = torch.empty_like(x)
        assert vh.flip_nchw(x, out=out) is out and torch.equal(out.view(torch.int32), y.view(torch.int32))
    if name == "special":                                 # bits are moved: NaN payloads survive
        bits = torch.tensor([[0x7FC12345, 0x7F800001, -0x3FEDCBB, 5], [1, 2, 3, 4]], dtype=torch.int32, device=dev())
        assert torch.equal(vh.flip_nchw(bits.view(torch.float32)).view(torch.int32), bits.flip(-1))


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_flip_merge_has_the_references_bits(vh, golden, name, shift):
    pairs = FC.TABLES[FC.CASES[name][4]]
    hm, fl = FC.inputs(name)
    for a, b in ((to_dev(hm), to_dev(fl)), (_misaligned(hm), to_dev(fl)), (to_dev(hm), _misaligned(fl))):
        keep = b.clone()
        assert vh.flip_merge(a, b, pairs, shift=bool(shift)) is a
        assert _stored(golden, f"{name}.m{shift}", a), (name, shift)
        assert torch.equal(b.view(torch.int32), keep.view(torch.int32))          # hm_flip is only read


def test_flip_merge_defaults_to_the_shift(vh, golden):
    hm, fl = FC.inputs("w48")
    assert _stored(golden, "w48.m1", vh.flip_merge(to_dev(hm), to_dev(fl), FC.COCO_PAIRS))


def test_refusals(vh):
    hm, fl = (torch.zeros((2, 17, 4, 8), device=dev()) for _ in range(2))
    both = torch.zeros((3, 17, 4, 8), device=dev())
    for a, b in ((hm, hm), (both[:2], both[1:]), (both[1:], both[:2])):            # the same tensor, and partial overlaps either way
        with pytest.raises(vh.VatlError, match="overlap"):
            vh.flip_merge(a, b, COCO)
    for pairs in ([[0, 17]], [[-1, 3]]):
        with pytest.raises(vh.VatlError, match="outside"):
            vh.flip_merge(hm, fl, pairs)
    wide = torch.zeros((2, 17, 4, 16), device=dev())
    for a, b in ((wide[..., :8], fl), (hm, wide[..., :8]), (hm.cpu(), fl), (hm, fl.cpu()), (hm, fl[:1]), (hm.double(), fl.double()), (hm[0], fl[0])):
        with pytest.raises(vh.VatlError):
            vh.flip_merge(a, b, COCO)
    assert not hm.any() and not fl.any()
    with pytest.raises(vh.VatlError, match="out of place"):
        vh.flip_nchw(hm, out=hm)
    for x, out in ((wide[..., :8], None), (hm.cpu(), None), (hm, fl[:1]), (hm, fl.cpu()), (hm.double(), None)):
        with pytest.raises(vh.VatlError):
            vh.flip_nchw(x, out=out)


def test_decode_of_the_merged_planes_gives_the_references_hms_flip_coordinates(vh, golden):
    """heatmap_to_coord_simple(hms, bbox, hms_flip) of the reference, under the criterion of tests/test_gpu_scorers.py::test_decode_golden: the maxima
    are copied values (bit-exact), the coordinates go through the float64 crop affine (1e-4)."""
    name = FC.DECODE_CASE
    hm, fl = FC.inputs(name)
    merged = vh.flip_merge(to_dev(hm), to_dev(fl), FC.TABLES[FC.CASES[name][4]], shift=True)
    coords, maxv, _ = vh.decode(merged, to_dev(FC.boxes(hm.shape[0])))
    assert np.array_equal(maxv.cpu().numpy(), golden["decode.maxvals"][..., 0])
    np.testing.assert_allclose(coords.cpu().numpy(), golden["decode.coords"], rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------------------------------- engine
@functools.lru_cache(maxsize=None)
def _net(name):
    """Per network, built once and shared: the model, 4 seeded crops, and the heat-maps of the crops and of their mirror images."""
    from alphapose.models import hip_engine
    from alphapose.utils.transforms import flip
    m = _build(name)
    x = to_dev(np.random.RandomState(77).standard_normal((4, 3, 256, 192)).astype(np.float32) * 0.25)
    a, b = (torch.empty((4, 17, 64, 48), device=dev()) for _ in range(2))
    with torch.no_grad():
        hip_engine.forward_into(m, x, a)
        hip_engine.forward_into(m, flip(x).contiguous(), b)
    return m, x, a, b


def _compose(a, b, pairs=COCO, shift=True):
    from alphapose.utils.transforms import flip_heatmap
    return (a + flip_heatmap(b, pairs, shift=shift)) / 2


@pytest.mark.parametrize("name", ["simplepose_r50", "fastpose_r50"])
def test_engine_equals_the_composition_bit_for_bit(vh, name):
    from alphapose.models import hip_engine, hip_engine_flip
    m, x, a, b = _net(name)
    want = _compose(a, b)
    assert not torch.equal(want, a)                        # the mirrored pass changes something
    out = torch.full((4, 17, 64, 48), float("nan"), device=dev())
    with torch.no_grad():
        assert hip_engine_flip.flip_forward_into(m, x, out, COCO) is out
    assert torch.equal(out, want)
    # with the embeddings: those of the un-mirrored pass, with forward_with_embedding's bits; the maps are the same
    hm_ref, emb_ref = torch.empty_like(a), torch.empty((4, 2048), device=dev())
    out2, emb = torch.empty_like(a), torch.full((4, 2048), float("nan"), device=dev())
    with torch.no_grad():
        hip_engine.forward_with_embedding(m, x, hm_ref, emb_ref)
        hip_engine_flip.flip_forward_into(m, x, out2, COCO, emb=emb)
    assert torch.equal(emb, emb_ref) and torch.equal(out2, want)
    # shift off, and another table
    jrdb = [list(p) for p in FC.JRDB_PAIRS]
    with torch.no_grad():
        hip_engine_flip.flip_forward_into(m, x, out, jrdb, shift=False)
    assert torch.equal(out, _compose(a, b, jrdb, shift=False))


@pytest.mark.parametrize("name", ["simplepose_r50", "fastpose_r50"])
def test_engine_on_the_bf16_route(vh, name):
    from alphapose.models import hip_engine_flip, hip_engine_h16
    from alphapose.utils.transforms import flip
    m, x, _, _ = _net(name)
    a, b, hm_ref = (torch.empty((4, 17, 64, 48), device=dev()) for _ in range(3))
    emb_ref, emb = (torch.empty((4, 2048), device=dev()) for _ in range(2))
    out = torch.empty_like(a)
    with torch.no_grad():
        hip_engine_h16.forward_h16(m, x, a, dtype=torch.bfloat16)
        hip_engine_h16.forward_h16(m, flip(x).contiguous(), b, dtype=torch.bfloat16)
        hip_engine_h16.forward_with_embedding_h16(m, x, hm_ref, emb_ref, dtype=torch.bfloat16)
        hip_engine_flip.flip_forward_into(m, x, out, COCO, emb=emb, dtype=torch.bfloat16)
    assert torch.equal(out, _compose(a, b)) and torch.equal(emb, emb_ref)
    assert not torch.equal(a, _net(name)[2])               # it really was the 16-bit route
    with pytest.raises(vh.VatlError, match="dtype"):
        hip_engine_flip.flip_forward_into(m, x, out, COCO, dtype=torch.float64)


def test_engine_is_exactly_equivariant(vh):
    """shift off, COCO pairs (an involution): the flip test of the mirrored crops is the flipped flip test of the crops — the two sums have
    the same terms in swapped order.  A mirrored index, a wrong joint source or a one-sided average cannot pass this."""
    from alphapose.models import hip_engine_flip
    from alphapose.utils.transforms import flip, flip_heatmap
    m, x, a, _ = _net("simplepose_r50")
    left, right = torch.empty_like(a), torch.empty_like(a)
    with torch.no_grad():
        hip_engine_flip.flip_forward_into(m, flip(x).contiguous(), left, COCO, shift=False)
        hip_engine_flip.flip_forward_into(m, x, right, COCO, shift=False)
    assert torch.equal(left, flip_heatmap(right, COCO, shift=False))
    assert not torch.equal(left, right)


def test_engine_cuts_the_batch_as_the_engine_does(vh, monkeypatch):
    """Chunks of 2 and 1 crops: the scratch of the first chunk serves the later, smaller one; results do not depend on the cut."""
    from alphapose.models import hip_engine, hip_engine_flip
    m, x, a, b = _net("simplepose_r50")
    monkeypatch.setattr(hip_engine, "MAX_CHUNK", 2)
    assert hip_engine._chunks(3, (256, 192)) == [(0, 2), (2, 3)]
    out, emb, emb_ref, hm_ref = torch.empty_like(a), torch.empty((4, 2048), device=dev()), torch.empty((4, 2048), device=dev()), torch.empty_like(a)
    with torch.no_grad():
        hip_engine_flip.flip_forward_into(m, x[:3], out[:3], COCO, emb=emb[:3])
        hip_engine.forward_with_embedding(m, x[:3], hm_ref[:3], emb_ref[:3])
    assert torch.equal(out[:3], _compose(a, b)[:3]) and torch.equal(emb[:3], emb_ref[:3])


def test_engine_refuses_what_the_entry_points_refuse(vh):
    from alphapose.models import hip_engine_flip
    m, x, a, _ = _net("simplepose_r50")
    out = torch.empty_like(a)
    with pytest.raises(vh.VatlError, match="MI355X only"):
        hip_engine_flip.flip_forward_into(m, x.cpu(), out, COCO)
    with pytest.raises(vh.VatlError, match="outside"):
        hip_engine_flip.flip_forward_into(m, x, out, [[3, 17]])
    m.train()
    try:
        for dt in (None, torch.bfloat16):
            with pytest.raises(vh.VatlError, match="eval"):
                hip_engine_flip.flip_forward_into(m, x, out, COCO, dtype=dt)
    finally:
        m.eval()


# ------------------------------------------------------------------------------------------------------------------ ActiveLearning
def _cfg(loss="MSELoss", **val):
    from alphapose.utils.config import edict
    return edict({
        "DATASET": {"TRAIN": {"TYPE": "SyntheticVideo", "NUM_ITEMS": 24, "TRACKS": 2}, "EVAL": {"TYPE": "SyntheticVideo", "NUM_ITEMS": 24, "TRACKS": 2}},
        "DATA_PRESET": {"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]},
        "MODEL": {"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50},
        "LOSS": {"TYPE": loss} if loss == "MSELoss" else {"TYPE": loss, "NORM_TYPE": "sigmoid"},
        "AE": {"Z_DIM": 4, "INPUT_DIM": 42, "PRETRAINED": "", "EPOCH": 2, "LR": 1e-3},
        "RETRAIN": {"BATCH_SIZE": 8, "BASE": 1, "OPTIMIZER": "AdamW", "LR": 2.5e-4, "ALPHA": 2, "WEIGHT_DECAY": 0.7, "LR_GAMMA": 0.99},
        "VAL": dict({"BATCH_SIZE": 10, "W_UNC": 0.01, "UNC_LAMBDA": 0.01, "QUERY_RATIO": [0.25, 0.5, 1.0]}, **val),
    })


def _opt():
    return types.SimpleNamespace(work_dir=None, uncertainty="THC_L1", representativeness="None", filter="None", strategy="THC_L1", video_id="syn",
                                 get_prenext=True, from_scratch=True, continual=True, num_gpu=1, onebyone=False, retrain_thresh=1, THCvsWPU="const")


def _first_round(**val):
    from active_learning import ActiveLearning
    torch.manual_seed(0)
    np.random.seed(0)
    al = ActiveLearning(_cfg(**val), _opt())
    al.eval_and_query()
    return al


def _composition_rows(vh, al, forward):
    """Key-point rows of the composition over the round's own loader batches."""
    from alphapose.utils.transforms import flip
    ds = al.eval_dataset
    rows = []
    for lo in range(0, len(ds), al.eval_loader.batch_size):
        idx = range(lo, min(lo + al.eval_loader.batch_size, len(ds)))
        x = torch.stack([ds._crop(i) for i in idx]).to(dev())
        a, b = (torch.empty((len(idx), 17, 64, 48), device=dev()) for _ in range(2))
        with torch.no_grad():
            forward(al.model, x, a)
            forward(al.model, flip(x).contiguous(), b)
        rows.append(vh.decode_pose(_compose(a, b, ds.joint_pairs), to_dev(ds.bbox[list(idx)]))[0].reshape(len(idx), -1).cpu().numpy())
    return np.concatenate(rows)


def test_a_round_with_the_key_on_scores_the_merged_maps(vh):
    from alphapose.models import hip_engine
    al = _first_round(FLIP_TEST=True)
    assert al.flip_test is True and al.dedup
    assert np.array_equal(al.keypoints, _composition_rows(vh, al, hip_engine.forward_into))
    assert al.performance[0]["flip_test"] is True and 0.0 <= al.performance[0]["mOKS"] <= 1.0
    u = al.uncertainty_dict["Round0"]
    assert all(np.isfinite(np.asarray(u[i], np.float64)).all() for i in range(24)) and len(al.query_list_list["Round0"]) == 6
    al.close()


def test_a_round_with_the_key_on_and_a_16_bit_evaluation_pass(vh):
    from alphapose.models import hip_engine_h16
    al = _first_round(FLIP_TEST=True, PRECISION="bf16")
    rows = _composition_rows(vh, al, lambda m, x, out: hip_engine_h16.forward_h16(m, x, out, dtype=torch.bfloat16))
    assert np.array_equal(al.keypoints, rows)
    assert al.performance[0]["flip_test"] is True and al.performance[0]["precision"] == "bf16"
    al.close()


def test_an_absent_key_and_false_are_the_same_run_and_differ_from_true(vh):
    from alphapose.models import hip_engine
    a, b = _first_round(), _first_round(FLIP_TEST=False)
    assert a.flip_test is False and b.flip_test is False
    assert np.array_equal(a.keypoints, b.keypoints) and np.array_equal(a.oks, b.oks)
    ua, ub = a.uncertainty_dict["Round0"], b.uncertainty_dict["Round0"]
    assert sorted(ua) == sorted(ub) and all(np.array_equal(np.asarray(ua[k]), np.asarray(ub[k])) for k in ua)
    assert a.query_list_list["Round0"] == b.query_list_list["Round0"]
    assert "flip_test" not in a.performance[0] and a.performance[0] == b.performance[0]
    # ... and are the plain stream: one forward per crop, decoded
    ds = a.eval_dataset
    x = torch.stack([ds._crop(i) for i in range(10)]).to(dev())
    hm = torch.empty((10, 17, 64, 48), device=dev())
    with torch.no_grad():
        hip_engine.forward_into(a.model, x, hm)
    assert np.array_equal(a.keypoints[:10], vh.decode_pose(hm, to_dev(ds.bbox[:10]))[0].reshape(10, -1).cpu().numpy())
    a.close(); b.close()


def test_the_three_forwards_path_flips_the_neighbours_too(vh):
    """A data set that does not declare an id-sorted stream hands over [current, previous, next] crops: each of the three forwards of
    `_heatmaps` is followed by its mirrored pass and merge."""
    from active_learning import ActiveLearning
    from alphapose.datasets.synthetic import SyntheticVideo
    from alphapose.models import hip_engine
    from alphapose.utils.transforms import flip

    class Unsorted(SyntheticVideo):
        ID_SORTED_STREAM = False

    preset = {"IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48], "SIGMA": 2, "NUM_JOINTS": 17}
    ds = Unsorted(train=False, get_prenext=True, PRESET=preset, NUM_ITEMS=8, TRACKS=2)
    torch.manual_seed(0)
    al = ActiveLearning(_cfg(FLIP_TEST=True), _opt(), eval_dataset=ds, train_dataset=SyntheticVideo(train=True, get_prenext=False, PRESET=preset, NUM_ITEMS=8))
    assert not al.dedup and al.get_prenext
    al.model.eval()
    inps = ds.my_collate_fn([ds[i] for i in range(1, 4)])[1]
    got = al._heatmaps(inps)
    for k in range(3):
        x = inps[:, k].to(dev())
        a, b = (torch.empty((3, 17, 64, 48), device=dev()) for _ in range(2))
        with torch.no_grad():
            hip_engine.forward_into(al.model, x, a)
            hip_engine.forward_into(al.model, flip(x).contiguous(), b)
        assert torch.equal(got[k], _compose(a, b, ds.joint_pairs)), k
    al.close()


def test_the_constructor_refuses_a_bad_key_and_another_decoder():
    from active_learning import ActiveLearning
    for bad in ("true", 1):
        with pytest.raises(ValueError, match="VAL.FLIP_TEST"):
            ActiveLearning(_cfg(FLIP_TEST=bad), _opt())
    with pytest.raises(NotImplementedError, match="heatmap_to_coord_simple_regress"):
        ActiveLearning(_cfg("L1JointRegression", FLIP_TEST=True), _opt())


# ------------------------------------------------------------------------------------------------------- pre-training validation
def test_pretrain_validate_with_the_flag_writes_the_compositions_records(vh, tmp_path):
    from alphapose import pretrain
    from alphapose.models import builder, hip_engine
    from alphapose.utils.transforms import flip, flip_heatmap, heatmap_to_coord_simple
    from oracle import synth
    from tests.test_gpu_pose_pretrain import _fresh_simplepose, _posetrack_cfg
    ann, frames, kept = synth.write_coco_video(str(tmp_path), n_frames=3, tracks=2)
    cfg = _posetrack_cfg(tmp_path, ann)
    ds = builder.build_dataset(cfg.DATASET.VAL, preset_cfg=cfg.DATA_PRESET, train=False)
    m = _fresh_simplepose(5)
    m.load_state_dict(synth.state_dict_for(m), strict=True)
    m = m.to(dev())

    def keypoints(**kw):
        res = pretrain.validate(m, cfg, ds, str(tmp_path / "work"), **kw)
        recs = json.load(open(tmp_path / "work" / "predicted_kpt.json"))
        assert res["records"] == len(recs) == len(ds) == 6
        return [r["keypoints"] for r in recs]
    plain, flagged = keypoints(), keypoints(flip_test=True)
    cfg.VAL["FLIP_TEST"] = True
    assert keypoints() == flagged and flagged != plain                       # the yaml key does what the flag does
    cfg.VAL["FLIP_TEST"] = False
    assert keypoints() == plain and keypoints(flip_test=True) == flagged
    for i in range(len(ds)):
        _, inp, _, _, _, _, _, bb_crop, _, _, _ = ds[i]
        x = inp[0][None].to(dev())
        a, b = (torch.empty((1, 17, 64, 48), device=dev()) for _ in range(2))
        with torch.no_grad():
            hip_engine.forward_into(m, x, a)
            hip_engine.forward_into(m, flip(x).contiguous(), b)
        box = bb_crop.cpu().numpy().tolist()
        coords, scores = heatmap_to_coord_simple(a[0][ds.EVAL_JOINTS], box, hms_flip=flip_heatmap(b, ds.joint_pairs, shift=True)[0][ds.EVAL_JOINTS])
        assert flagged[i] == np.concatenate((coords, scores), axis=1).reshape(-1).tolist()
        coords, scores = heatmap_to_coord_simple(a[0][ds.EVAL_JOINTS], box)
        assert plain[i] == np.concatenate((coords, scores), axis=1).reshape(-1).tolist()
    cfg.VAL["FLIP_TEST"] = "yes"
    with pytest.raises(ValueError, match="VAL.FLIP_TEST"):
        pretrain.validate(m, cfg, ds, str(tmp_path / "work"))
