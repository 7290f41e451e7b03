"""The query-selection cases and their float64 restatement (tests/query_cases.py) against the reference's own scikit-learn calls
(oracle/query.py), on the host: what tests/test_gpu_query.py holds the kernels to is right, and every case has one right answer."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import query as OQ
from tests import query_cases as QC


@pytest.mark.parametrize("case", QC.ROWSUM_CASES, ids=QC.rowsum_id)
def test_cosine_restatement_matches_sklearn(case):
    x = QC.rowsum_case(case)
    n = case[0]
    got, want = QC.cosine_sums_ref(x), OQ.cosine_distance_sums(x)
    print(f"{QC.rowsum_id(case)}: max |restatement - sklearn| = {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)        # measured: 3.5e-13 at most (float64 sums of up to 1030 terms of size <= 2)
    if n > 3:
        assert got[2] == n - 1 and want[2] == n - 1                  # the zero row
        assert got[n - 1] == got[1]                                  # the duplicate row


def test_cosine_restatement_single_row():
    """n = 1 is outside scikit-learn's reach (n_neighbors = 0): 0 for a non-zero row (1 - u.u) and 0 for a zero row (n - 1)."""
    assert abs(QC.cosine_sums_ref(QC.emb_case(1, 1, 65, "signed"))[0]) <= 1e-15
    assert QC.cosine_sums_ref(np.zeros((1, 65), np.float32))[0] == 0.0


def test_zero_row_formula_differs_from_sklearn():
    """n - u_i . s gives n for a zero row; scikit-learn, whose diagonal is zero, gives n - 1."""
    x = QC.emb_case(3, 7, 5, "signed")
    x[3] = 0
    want = OQ.cosine_distance_sums(x)
    assert want[3] == 6.0 and QC.cosine_sums_ref(x)[3] == 6.0
    xd = x.astype(np.float64)
    u = xd / np.where(np.arange(7) == 3, 1.0, np.sqrt((xd * xd).sum(axis=1)))[:, None]
    assert (7 - u @ u.sum(axis=0))[3] == 7.0


@pytest.mark.parametrize("name", QC.CORESET_NAMES)
def test_coreset_restatement_matches_oracle(name):
    x, labeled, unc, q, mode, moks, lam = QC.coreset_case(name)
    want = OQ.coreset_selection(x, labeled, unc.copy(), q, mode, moks, lam, rng=np.random.RandomState(QC.RNG_SEED))
    got, gaps = QC.coreset_ref(x, labeled, unc.copy(), q, mode, moks, lam, rng=np.random.RandomState(QC.RNG_SEED))
    h = QC.held(name, q)
    print(f"{name}: picks {got}, smallest held gap {min(gaps[:h]):.3e}")
    assert got[:h] == want[:h]
    assert got[h:] == [0] * (q - h)                                  # exhausted pool: every score is exactly 0, the first arg-max is 0
    assert all(g == 0.0 for g in gaps[h:])
    assert len(set(got[:h])) == h and not set(got[:h]) & set(labeled.tolist())


def test_every_coreset_step_has_one_answer():
    """The relative gap between the best and the second-best score is at least 1e-6 at every step held to the oracle: seven orders above
    the 2.3e-13 a float64 sum of 2048 terms can be off by, so the pick does not hang on the order of summation."""
    smallest = {}
    for name in QC.CORESET_NAMES:
        x, labeled, unc, q, mode, moks, lam = QC.coreset_case(name)
        _, gaps = QC.coreset_ref(x, labeled, unc, q, mode, moks, lam, rng=np.random.RandomState(QC.RNG_SEED))
        smallest[name] = min(gaps[:QC.held(name, q)])
    print(smallest)
    assert len(smallest) == 9
    assert all(g >= QC.MIN_GAP for g in smallest.values()), smallest


def test_argmax_ref_is_np_argmax():
    r = np.random.RandomState(0)
    for _ in range(200):
        v = r.randint(0, 4, r.randint(1, 9)).astype(np.float64)
        v[r.random_sample(len(v)) < 0.15] = np.nan
        v[r.random_sample(len(v)) < 0.15] = -np.inf
        assert QC.argmax_ref(v)[0] == int(np.argmax(v)), v
    assert QC.argmax_ref([1.0, np.nan, 2.0, np.nan])[0] == 1
    assert QC.argmax_ref([-np.inf] * 5)[0] == 0 and QC.argmax_ref([np.nan] * 5)[0] == 0


def test_fused_pair_ties_in_numpy_and_splits_when_contracted():
    a, b, md, unc = QC.FUSED_A, QC.FUSED_B, QC.FUSED_MIN_DIST, QC.FUSED_UNC
    score = a * md + b * unc
    assert score[0] == score[1] == QC.FUSED_SCORE
    assert int(np.argmax(score)) == 0 and QC.pick_ref(md, unc, a, b) == (0, 0.0)

    def rounded(fr):                                                 # Fraction -> nearest double (int / int division rounds correctly)
        return fr.numerator / fr.denominator

    F = Fraction
    two_roundings = [rounded(F(rounded(F(a) * F(float(m)))) + F(rounded(F(b) * F(float(u))))) for m, u in zip(md, unc)]
    assert two_roundings == score.tolist()
    contracted = [rounded(F(a) * F(float(m)) + F(rounded(F(b) * F(float(u))))) for m, u in zip(md, unc)]   # fma(a, md, fl(b * unc))
    assert contracted[0] == QC.FUSED_SCORE
    assert contracted[1] == math.nextafter(QC.FUSED_SCORE, 1.0)
    assert int(np.argmax(contracted)) == 1
