"""CPU checks around the K-Means fixture (tests/golden/kmeans.npz): it loads as plain data, the installed scikit-learn still
computes what it holds, the host path of kmeans_queries returns its representatives, and the random draws the device path makes
on the host are RandomState(318)'s sequence in scikit-learn's order."""
import numpy as np
import pytest

from tests import kmeans_cases as KC


@pytest.fixture(scope="module")
def golden():
    return KC.Golden()


def test_fixture_holds_the_fifteen_cases_and_only_data(golden):
    assert golden.cases == KC.ALL_CASES and len(golden.cases) == 15
    assert all(golden.z[name].dtype != object for name in golden.z.files)
    assert str(golden.z["sklearn_version"]).startswith("1.7") and str(golden.z["numpy_version"])
    for case in KC.ALL_CASES:
        n, k, _, _ = case
        labels, reps, init = golden.get(case, "labels"), golden.get(case, "reps"), golden.get(case, "init")
        assert labels.shape == (n,) and labels.min() == 0 and labels.max() == k - 1
        assert init.shape == (k,) and 0 <= init.min() and init.max() < n
        assert len(reps) == len(np.unique(labels)) and all(labels[r] == j for j, r in enumerate(reps))
        assert golden.get(case, "tied").shape == (len(reps),) and 1 <= int(golden.get(case, "n_iter")) <= 300
    # the claim's conditions: no tied cluster in the main cases; of the small shapes only (24, 6, 7) has one, of two members
    assert not any(golden.get(c, "tied").any() for c in KC.MAIN_CASES)
    assert [int(golden.get(c, "tied").sum()) for c in KC.SMALL_CASES] == [1, 0, 0, 0, 0]
    j = int(np.flatnonzero(golden.get(KC.SMALL_CASES[0], "tied"))[0])
    assert len(golden.tied_members(KC.SMALL_CASES[0], j)) == 2
    assert max(float(golden.get(c, "restatement_centre_err")) for c in KC.DEVICE_CASES) < 2e-15
    assert [c for c in KC.ALL_CASES if golden.has(c, "centres")] == [KC.MAIN_CASES[0]] + KC.SMALL_CASES
    for c in KC.SMALL_CASES:                                     # and the member means recomputed from the labels are those centres
        x, w = KC.case_inputs(c)
        mean = x.astype(np.float64).mean(axis=0)
        np.testing.assert_allclose(KC.member_means(x.astype(np.float64) - mean, golden.get(c, "labels"), c[1], w) + mean, golden.get(c, "centres"),
                                   rtol=0, atol=max(float(golden.get(c, "restatement_centre_err")), 1e-300))


def _sklearn():
    sklearn = pytest.importorskip("sklearn")
    if tuple(int(v) for v in sklearn.__version__.split(".")[:2]) < (1, 4):
        pytest.skip("scikit-learn >= 1.4 needed (n_init='auto', sample_weight in k-means++)")
    return sklearn


@pytest.mark.parametrize("case", KC.ALL_CASES, ids=KC.case_id)
def test_installed_sklearn_reproduces_the_fixture(golden, case):
    """A scikit-learn upgrade that changes the algorithm is noticed here, not blamed on the kernels."""
    _sklearn()
    from sklearn.cluster import KMeans
    x, w = KC.case_inputs(case)
    km = KMeans(n_clusters=case[1], random_state=318)
    labels = km.fit_predict(x.astype(np.float64), sample_weight=w)
    assert np.array_equal(labels, golden.get(case, "labels")) and km.n_iter_ == int(golden.get(case, "n_iter"))
    np.testing.assert_allclose(km.inertia_, float(golden.get(case, "inertia")), rtol=1e-12)


@pytest.mark.parametrize("case", KC.ALL_CASES, ids=KC.case_id)
def test_host_kmeans_queries_returns_the_fixture_representatives(golden, case):
    _sklearn()
    from active_learning import query as Q
    x, w = KC.case_inputs(case)
    cand = list(range(1000, 1000 + case[0]))
    res = Q.kmeans_queries(x.astype(np.float64), cand, case[1], w)
    query, picks = res
    assert res.path == "host" and query == [cand[i] for i in picks]
    want, tied = golden.get(case, "reps"), golden.get(case, "tied")
    assert len(picks) == len(want)
    for j, (got, exp) in enumerate(zip(picks, want)):
        assert int(got) in (golden.tied_members(case, j) if tied[j] else [int(exp)]), (j, got, exp)


@pytest.mark.parametrize("n,k,weighted", [(257, 13, True), (1024, 154, False)])
def test_host_draws_are_randomstate_318_in_sklearn_order(n, k, weighted):
    from active_learning import query as Q
    w = KC.weights(n, 1) if weighted else None
    first, draws = Q.kmeans_draws(n, k, w)
    rs = np.random.RandomState(318)
    p = np.ones(n) / n if w is None else w / w.sum()
    assert first == rs.choice(n, p=p)
    trials = 2 + int(np.log(k))
    assert draws.shape == (k - 1, trials) and draws.dtype == np.float64
    for c in range(k - 1):
        assert np.array_equal(draws[c], rs.uniform(size=trials))
    assert Q.kmeans_draws(5, 1)[1].shape == (0, 2)
