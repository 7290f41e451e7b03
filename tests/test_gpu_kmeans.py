"""K-Means / weighted query filters on the device against scikit-learn's seeded run (tests/golden/kmeans.npz, written by
tools/make_kmeans_golden.py; inputs regenerated from the cases' seeds).  Labels, iteration counts, seeding indices and
representatives are integers and must be EQUAL; centres and inertia are bounded by 100 x the error of an independent float64
numpy restatement on the same case (stored in the fixture): rounding grows with the summation length D = 2048, not with the
device."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import kmeans_cases as KC
from tests.gpu_util import dev, record

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def golden():
    return KC.Golden()


def _dev_inputs(case):
    x, w = KC.case_inputs(case)
    return x, w, torch.from_numpy(x).to(dev())


@pytest.mark.parametrize("case", KC.DEVICE_CASES, ids=KC.case_id)
def test_seeding_alone(golden, case):
    from active_learning import query as Q
    x, w, xd = _dev_inputs(case)
    idx, tied = Q.kmeans_seeding(xd, case[1], w)
    print("seeding", case, idx.tolist(), "tie flag", tied)
    assert not tied
    assert idx.tolist() == golden.get(case, "init").tolist()


@pytest.mark.parametrize("case", KC.DEVICE_CASES, ids=KC.case_id)
def test_lloyd_alone_from_fixture_indices(golden, case):
    from active_learning import query as Q
    x, w, xd = _dev_inputs(case)
    n, k = case[:2]
    res = Q.kmeans_fit(xd, k, w, init_indices=golden.get(case, "init"))
    assert res.path == "device", res.reason
    labels = golden.get(case, "labels")
    x64 = x.astype(np.float64)
    mean = x64.mean(axis=0)
    ref = KC.member_means(x64 - mean, labels, k, w) + mean
    fig = float(golden.get(case, "restatement_centre_err"))
    same = np.array_equal(res.labels, labels)
    err = float(np.abs(res.centers - ref).max()) if same else float("nan")
    inertia = float(golden.get(case, "inertia"))
    rel_inertia = abs(res.inertia - inertia) / inertia if inertia else abs(res.inertia)
    print("lloyd", case, "labels equal", same, "n_iter", res.n_iter, int(golden.get(case, "n_iter")), "centre err %.3e" % err, "restatement %.3e" % fig,
          "inertia rel err %.3e" % rel_inertia)
    record("kmeans_lloyd", case=list(case), centre_err=err, restatement_err=fig, inertia_rel_err=rel_inertia, n_iter=res.n_iter)
    assert same and res.n_iter == int(golden.get(case, "n_iter"))
    assert err <= 100 * fig
    if golden.has(case, "centres"):                              # the small cases: scikit-learn's own centres are in the fixture
        err_sk = float(np.abs(res.centers - golden.get(case, "centres")).max())
        print("lloyd", case, "centre err against cluster_centers_ %.3e" % err_sk)
        assert err_sk <= 100 * fig
    # inertia: scikit-learn adds each point's D = 2048 squared differences one after the other, so its own rounding is up to D * eps
    # relative (4.5e-13); the centres' error enters in second order only (they are the clusters' means)
    assert rel_inertia <= 2048 * EPS


@pytest.mark.parametrize("case", KC.DEVICE_CASES, ids=KC.case_id)
def test_end_to_end_representatives(golden, case):
    from active_learning import query as Q
    x, w, xd = _dev_inputs(case)
    cand = list(range(1000, 1000 + case[0]))
    res = Q.kmeans_queries(xd, cand, case[1], w)
    query, picks = res
    assert res.path == "device", res.reason
    assert res.n_iter == int(golden.get(case, "n_iter"))
    want, tied = golden.get(case, "reps"), golden.get(case, "tied")
    assert len(picks) == len(want) and query == [cand[i] for i in picks]
    for j, (got, exp) in enumerate(zip(picks, want)):
        if tied[j]:
            assert got == min(golden.tied_members(case, j)), (j, got, golden.tied_members(case, j))
        else:
            assert got == int(exp), (j, got, exp)


def test_two_runs_give_the_same_bits():
    from active_learning import query as Q
    case = (1024, 51, 3, True)
    x, w, xd = _dev_inputs(case)
    a, b = Q.kmeans_fit(xd, 51, w), Q.kmeans_fit(xd, 51, w)
    assert a.path == b.path == "device"
    assert np.array_equal(a.centers.view(np.int64), b.centers.view(np.int64)) and np.array_equal(a.labels, b.labels)
    assert a.inertia == b.inertia and a.representatives == b.representatives


@pytest.mark.parametrize("which", ["degenerate", "tie"])
def test_handed_back_to_the_host(which):
    """Where scikit-learn's answer hangs on its rounding (empty cluster, tied seeding candidates) the device path stops and
    scikit-learn runs on the host exactly as before."""
    from active_learning import query as Q
    if which == "degenerate":
        x, k = KC.degenerate(), 16
    else:
        x, k = KC.case_inputs(KC.TIE_CASE)[0], KC.TIE_CASE[1]
    cand = list(range(len(x)))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                          # scikit-learn warns about the duplicate points
        got = Q.kmeans_queries(torch.from_numpy(x).to(dev()), cand, k)
        want = Q.kmeans_queries(x.astype(np.float64), cand, k)
    print(which, "reason:", got.reason)
    assert got.path == "host" and got.reason in ("empty cluster", "tied seeding candidates")
    if which == "tie":
        assert got.reason == "tied seeding candidates"
    assert list(got[0]) == list(want[0]) and [int(i) for i in got[1]] == [int(i) for i in want[1]]
    if which == "degenerate":                                    # the Lloyd stage's own trigger: duplicate centres leave clusters empty
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = Q.kmeans_fit(torch.from_numpy(x).to(dev()), k, init_indices=np.arange(16))
        assert res.path == "host" and res.reason == "empty cluster"


def test_duplicate_removal_matches_numpy_unique():
    from active_learning import query as Q
    x = KC.emb(300, seed=21)
    r = np.random.RandomState(5)
    x[r.randint(0, 300, 40)] = x[r.randint(0, 300, 40)]
    x[[7, 8, 9]] = x[250]
    uniq, first = Q.unique_rows(torch.from_numpy(x).to(dev()))
    want_rows, want_first = np.unique(x.astype(np.float64), axis=0, return_index=True)
    assert len(want_first) < 300
    assert np.array_equal(first, want_first)
    assert np.array_equal(uniq.double().cpu().numpy(), want_rows)


def test_argument_checks_through_the_c_abi():
    import vatl_hip as vh
    lib = vh.lib()
    n, d, k = 32, 64, 4
    f64 = lambda *s: torch.zeros(*s, device=dev(), dtype=torch.float64)
    xc, w, cen, st, ws = f64(n, d), f64(n), f64(k, d), f64(4), f64(4096)
    emb = torch.zeros(n, d, device=dev())
    lab = torch.zeros(n, device=dev(), dtype=torch.int32)
    idx = torch.zeros(k + 1, device=dev(), dtype=torch.int32)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    bad = [
        lambda: lib.vatl_kmeans_prepare(None, n, d, P(xc), P(w), P(st), P(ws), None),
        lambda: lib.vatl_kmeans_prepare(P(emb), n, 0, P(xc), P(w), P(st), P(ws), None),
        lambda: lib.vatl_kmeans_seed(P(xc), P(w), n, d, n + 1, 0, P(ws), 3, P(idx), P(idx), P(ws), None),        # k > n
        lambda: lib.vatl_kmeans_seed(P(xc), None, n, d, k, 0, P(ws), 3, P(idx), P(idx), P(ws), None),
        lambda: lib.vatl_kmeans_seed(P(xc), P(w), n, d, k, n, P(ws), 3, P(idx), P(idx), P(ws), None),            # first index out of range
        lambda: lib.vatl_kmeans_seed(P(xc), P(w), n, d, k, 0, P(ws), 17, P(idx), P(idx), P(ws), None),           # too many trials
        lambda: lib.vatl_kmeans_assign(P(xc), P(cen), n, d, n + 1, None, P(lab), P(st), P(ws), None),
        lambda: lib.vatl_kmeans_assign(P(xc), P(cen), n, -1, k, None, P(lab), P(st), P(ws), None),
        lambda: lib.vatl_kmeans_assign(P(xc), P(cen), n, 24, k, None, P(lab), P(st), P(ws), None),               # D not a multiple of 16
        lambda: lib.vatl_kmeans_assign(P(xc), None, n, d, k, None, P(lab), P(st), P(ws), None),
        lambda: lib.vatl_kmeans_update(P(xc), P(w), None, P(cen), n, d, k, P(cen), P(st), P(ws), None),
        lambda: lib.vatl_kmeans_update(P(xc), P(w), P(lab), P(cen), n, d, n + 1, P(cen), P(st), P(ws), None),
        lambda: lib.vatl_kmeans_finish(P(emb), P(xc), P(w), P(w), P(cen), P(lab), n, 0, k, P(idx), P(st), P(ws), None),
        lambda: lib.vatl_kmeans_finish(P(emb), P(xc), P(w), P(w), P(cen), P(lab), n, d, k, None, P(st), P(ws), None),
    ]
    for i, call in enumerate(bad):
        assert call() != 0, i
        assert b"kmeans" in lib.vatl_last_error(), i
    torch.cuda.synchronize()
    assert float(st.abs().sum()) == 0 and int(lab.abs().sum()) == 0 and int(idx.abs().sum()) == 0          # nothing was launched
    assert lib.vatl_kmeans_seed_workspace_doubles(100, 3) == 5 * 100 + 8 and lib.vatl_kmeans_seed_workspace_doubles(100, 17) == 0
    with pytest.raises(ValueError):
        from active_learning import query as Q
        Q.kmeans_fit(emb[:3], 4)


def _cfg():
    from alphapose.utils.config import edict
    return edict({
        "DATASET": {"TRAIN": {"TYPE": "SyntheticVideo", "NUM_ITEMS": 120, "TRACKS": 2}, "EVAL": {"TYPE": "SyntheticVideo", "NUM_ITEMS": 120, "TRACKS": 2}},
        "DATA_PRESET": {"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]},
        "MODEL": {"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50},
        "LOSS": {"TYPE": "MSELoss"},
        "AE": {"Z_DIM": 4, "INPUT_DIM": 42, "PRETRAINED": "", "EPOCH": 2, "LR": 1e-3},
        "RETRAIN": {"BATCH_SIZE": 8, "BASE": 1, "OPTIMIZER": "AdamW", "LR": 2.5e-4, "ALPHA": 2, "WEIGHT_DECAY": 0.7, "LR_GAMMA": 0.99},
        "VAL": {"BATCH_SIZE": 10, "W_UNC": 0.01, "UNC_LAMBDA": 0.01, "QUERY_RATIO": [0.1, 0.5, 1.0]},
    })


@pytest.mark.parametrize("rep,flt", [("Influence", "weighted"), ("None", "K-Means")])
def test_product_round_selects_what_the_host_path_selects(rep, flt, monkeypatch):
    """ActiveLearning on SyntheticVideo (120 items, first query ratio 0.1: k = 12 = n / 10): Round0's queries equal what the host
    path selects from the rows, candidates and weights the round handed to kmeans_queries, and the round ran on the device."""
    from active_learning import ActiveLearning
    from active_learning import query as Q
    calls = []
    real = Q.kmeans_queries

    def spy(emb, cand, k, weight=None):
        out = real(emb, cand, k, weight)
        calls.append((emb, list(cand), k, None if weight is None else np.array(weight), out))
        return out
    monkeypatch.setattr(Q, "kmeans_queries", spy)
    deduped = []
    real_unique = Q.unique_rows
    monkeypatch.setattr(Q, "unique_rows", lambda e: (deduped.append(e), real_unique(e))[1])
    opt = types.SimpleNamespace(uncertainty="THC_L1", representativeness=rep, filter=flt, strategy="THC_L1", video_id="syn", get_prenext=True,
                                from_scratch=True, continual=True, num_gpu=1, onebyone=False, retrain_thresh=1, THCvsWPU="const", fixed_lambda=False)
    torch.manual_seed(0); np.random.seed(0)
    al = ActiveLearning(_cfg(), opt)
    al.eval_and_query()
    assert len(calls) == 1
    emb, cand, k, weight, out = calls[0]
    assert emb.is_cuda and k == 12 and (weight is not None) == (flt == "weighted")
    rows = emb.double().cpu().numpy()
    print(flt, "rows", rows.shape, "distinct", len(np.unique(rows, axis=0)), "path", al.query_path["Round0"])
    if flt == "weighted":
        # the reference's own sequence from the round's candidate rows (ActiveLearning.py:593-600): np.unique drops duplicates and
        # re-orders the rows, candidates and weights follow its first-occurrence indices
        assert len(deduped) == 1 and deduped[0].shape[0] == 120
        all_rows = deduped[0].double().cpu().numpy()
        unc, inf, cw = al.uncertainty_dict["Round0"], al.influence_dict["Round0"], al.combine_weight[0]
        u = al._total_score(np.array([[unc[i], 0.0] for i in range(120)]))
        total = cw * u + (1 - cw) * np.array([inf[i] for i in range(120)])
        _, first = np.unique(all_rows, axis=0, return_index=True)
        assert not np.array_equal(first, np.arange(len(first)))                  # the rows really are re-ordered
        assert cand == [int(i) for i in first] and np.array_equal(rows, all_rows[first])
        np.testing.assert_allclose(weight, (1 + al.w_unc * cw * total)[first], rtol=1e-12, atol=0)
        rows, cand, weight = all_rows[first], [int(i) for i in first], (1 + al.w_unc * cw * total)[first]
    want, _ = real(rows, cand, k, weight)
    assert al.query_path["Round0"]["path"] == "device", al.query_path["Round0"]
    assert al.query_list_list["Round0"] == want and len(set(want)) == 12
