"""Host side of the opt-in flip testing (cfg.VAL.FLIP_TEST): the yaml key, the joint permutation, and the numpy model of csrc/flip.hip
against the reference's own outputs (tests/golden/flip_test.npz, written by tools/make_flip_golden.py).  No GPU."""
import numpy as np
import pytest

from tests import flip_cases as FC


@pytest.fixture(scope="module")
def golden():
    return np.load(FC.GOLDEN)


def _stored(golden, key, a):
    """The fixture keeps arrays of more than DIGEST_ABOVE words as their SHA-256."""
    want = golden[key]
    if want.dtype.kind == "U":
        assert a.size > FC.DIGEST_ABOVE
        return FC.digest(np.ascontiguousarray(a, np.float32)) == str(want)
    return FC.same_bits(a, want)


def _cfg(loss="MSELoss", **val):
    from alphapose.utils.config import edict
    return edict({"DATA_PRESET": {"TYPE": "simple"}, "LOSS": {"TYPE": loss, "NORM_TYPE": "sigmoid"}, "VAL": dict({"BATCH_SIZE": 4}, **val)})


def test_the_key_is_a_bool_and_off_by_default():
    from active_learning.ActiveLearning import flip_test
    from alphapose.utils.config import edict
    assert flip_test(_cfg()) is False and flip_test(_cfg(FLIP_TEST=False)) is False and flip_test(_cfg(FLIP_TEST=True)) is True
    assert flip_test(edict({"DATA_PRESET": {"TYPE": "simple"}, "LOSS": {"TYPE": "MSELoss"}})) is False          # no VAL section at all
    for bad in ("true", "on", 1, 0, None, 1.0, [True]):
        with pytest.raises(ValueError, match="VAL.FLIP_TEST"):
            flip_test(_cfg(FLIP_TEST=bad))
    # alphapose.pretrain's --flip-test stands in for the key
    assert flip_test(_cfg(), True) is True and flip_test(_cfg(FLIP_TEST=True), None) is True and flip_test(_cfg(FLIP_TEST=False), True) is True


@pytest.mark.parametrize("loss, name", [("L1JointRegression", "heatmap_to_coord_simple_regress"), ("Combined", "heatmap_to_coord_simple_regress")])
def test_another_decoder_is_refused_by_name(loss, name):
    from active_learning.ActiveLearning import flip_test
    assert flip_test(_cfg(loss)) is False and flip_test(_cfg(loss, FLIP_TEST=False)) is False                    # off: nothing to refuse
    with pytest.raises(NotImplementedError, match=name):
        flip_test(_cfg(loss, FLIP_TEST=True))
    with pytest.raises(NotImplementedError, match=name):
        flip_test(_cfg(loss), True)


def test_the_constructor_refuses_before_it_touches_the_device():
    """No GPU here: a constructor that went on to build anything would fail differently."""
    import types

    from active_learning import ActiveLearning
    opt = types.SimpleNamespace(uncertainty="THC_L1", representativeness="None", filter="None", num_gpu=1)
    cfg = _cfg(FLIP_TEST="yes")
    cfg["DATASET"] = {"EVAL": {"TYPE": "SyntheticVideo"}, "TRAIN": {"TYPE": "SyntheticVideo"}}
    cfg["RETRAIN"] = {}
    with pytest.raises(ValueError, match="VAL.FLIP_TEST"):
        ActiveLearning(cfg, opt, eval_dataset=object(), train_dataset=object())
    cfg = _cfg("L1JointRegression", FLIP_TEST=True)
    cfg["DATASET"] = {"EVAL": {"TYPE": "SyntheticVideo"}, "TRAIN": {"TYPE": "SyntheticVideo"}}
    cfg["RETRAIN"] = {}
    with pytest.raises(NotImplementedError, match="heatmap_to_coord_simple_regress"):
        ActiveLearning(cfg, opt, eval_dataset=object(), train_dataset=object())


def test_pretrain_has_the_flag():
    from alphapose import pretrain
    assert pretrain.parse_args(["--cfg", "x.yaml"]).flip_test is False
    assert pretrain.parse_args(["--cfg", "x.yaml", "--flip-test"]).flip_test is True


@pytest.mark.parametrize("table", sorted(FC.TABLES))
def test_swaps_composed_in_list_order_give_the_references_joint_order(golden, table):
    import vatl_hip as vh
    pairs = [tuple(p) for p in golden[f"pairs.{table}"].tolist()]
    assert pairs == list(FC.TABLES[table])
    order = golden[f"order.{table}"].tolist()
    assert vh.flip_src_joints(pairs, len(order)) == order == FC.src_joints(pairs, len(order))
    if table == "jrdb":                                   # the list repeats joints: neither an involution nor what swapping "all at once" gives
        assert [order[k] for k in order] != list(range(17))
        once = list(range(17))
        for a, b in pairs:
            once[a], once[b] = b, a
        assert once != order
        from alphapose.datasets.coco_video import JRDB2022
        assert [tuple(p) for p in JRDB2022.joint_pairs] == pairs


def test_a_pair_outside_the_joints_is_refused():
    import vatl_hip as vh
    for pairs in ([(0, 17)], [(-1, 2)], [(1, 2), (17, 3)]):
        with pytest.raises(vh.VatlError, match="outside"):
            vh.flip_src_joints(pairs, 17)


@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_the_numpy_model_reproduces_the_fixture(golden, name):
    """tests/test_gpu_flip.py holds the kernels to the fixture; this holds the model that states their formula to it, so the two cannot drift."""
    n, j, h, w, table, _ = FC.CASES[name]
    pairs = FC.TABLES[table]
    hm, fl = FC.inputs(name)
    assert hm.shape == fl.shape == (n, j, h, w)
    assert FC.digest(hm) == str(golden[f"{name}.hm_sha"]) and FC.digest(fl) == str(golden[f"{name}.fl_sha"])
    assert _stored(golden, f"{name}.flip", hm[..., ::-1])
    for s in (0, 1):
        assert _stored(golden, f"{name}.fh{s}", FC.flip_heatmap_model(fl, pairs, s)), s
        assert _stored(golden, f"{name}.m{s}", FC.merge_model(hm, fl, pairs, s)), s
    if name == "special":
        m = golden["special.m0"]
        assert np.isnan(m).sum() >= 5 and np.isinf(m).sum() >= 4 and np.isnan(m[0, 1, 0, 0])          # inf + -inf met where inputs() says


def test_the_cases_cover_what_their_docstring_says(golden):
    shapes = list(FC.CASES.values())
    assert {c[3] for c in shapes} == {1, 2, 5, 48} and {c[2] for c in shapes} == {1, 3, 64} and {c[1] for c in shapes} == {1, 15, 17}
    assert {c[4] for c in shapes} == set(FC.TABLES)
    n, j = FC.CASES[FC.DECODE_CASE][:2]
    assert golden["decode.coords"].shape == (n, j, 2) and golden["decode.maxvals"].shape == (n, j, 1)
    import os
    assert os.path.getsize(FC.GOLDEN) < 200 * 1024
