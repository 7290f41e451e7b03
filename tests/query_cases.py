"""Query selection (csrc/query.hip): the seeded cases of tests/test_query_cpu.py and tests/test_gpu_query.py, and a plain numpy float64
restatement of what the kernels are meant to compute.

    cosine row sums   u_i = x_i / ||x_i|| (0 for a zero row), out_i = n - u_i . sum_j u_j; a zero row gives n - 1 (distance 1 to every
                      other row, 0 to itself: scikit-learn zeroes the diagonal)
    k-center update   min_dist_i = min(min_dist_i, sqrt(sum_d (x_id - x_cd)^2)) with direct differences: a centre is at exactly 0
    pick              score_i = fl(a * min_dist_i) + fl(b * unc_i), both products rounded as numpy rounds them; the first arg-max, a
                      NaN counting as the maximum (np.argmax)

The restatement also returns, per greedy step, the relative gap between the best and the second-best score: a case whose gap is far above
the arithmetic's error has one right answer, whichever way the distances were summed.
"""
import numpy as np

# a pair that tells a contracted score (mul + fma) from numpy's: numpy's two scores tie bit for bit, so np.argmax returns 0; with the
# first product left unrounded item 1 comes out one ulp larger
FUSED_A, FUSED_B = 0.4, 0.6
FUSED_MIN_DIST = np.array([0.0, float.fromhex("0x1.4e8bdfb2607a2p-1")])
FUSED_UNC = np.array([float.fromhex("0x1.fca53864960bap-1"), float.fromhex("0x1.1d9d4dedab0fap-1")])
FUSED_SCORE = float.fromhex("0x1.312feea2c06d6p-1")

ROWSUM_SHAPES = [(2, 1), (2, 4), (3, 63), (5, 64), (6, 65), (7, 255), (9, 256), (10, 257), (13, 2048), (257, 100), (1030, 48)]
KINDS = ("clustered", "signed")
# (n, d, kind, seed)
ROWSUM_CASES = [(n, d, kind, 500 + i) for i, (n, d) in enumerate(ROWSUM_SHAPES) for kind in KINDS]

# (name, n, D, kind, n_labeled, q, mode, moks, lambda); `held` picks are compared with the oracle (all of them unless stated)
CORESET_CASES = [
    ("tiny_d3", 5, 3, "signed", 1, 3, "kcenter", 0.0, 1.0),
    ("odd_37x65", 37, 65, "clustered", 3, 8, "moks", 0.6, 1.0),
    ("empty_pool_130x100", 130, 100, "clustered", 0, 6, "moks", 0.5, 1.0),
    ("empty_kcenter_50x20", 50, 20, "signed", 0, 5, "kcenter", 0.0, 1.0),
    ("wide_1500x48", 1500, 48, "clustered", 200, 10, "fixed", 0.0, 0.5),
    ("emb_257x2048", 257, 2048, "clustered", 40, 12, "kcenter", 0.0, 1.0),
    ("moks1_66x130", 66, 130, "clustered", 5, 7, "moks", 1.0, 2.0),
    ("moks0_66x130", 66, 130, "clustered", 5, 7, "moks", 0.0, 2.0),
    ("exhausted_6x16", 6, 16, "signed", 3, 5, "fixed", 0.0, 1.0),
]
CORESET_NAMES = [c[0] for c in CORESET_CASES]
HELD = {"exhausted_6x16": 3}              # the pool is empty after three picks: the rest is the arg-max of an all-zero score, index 0
MIN_GAP = 1e-6
RNG_SEED = 9


def emb_case(seed, n, d, kind):
    r = np.random.RandomState(seed)
    if kind == "clustered":                                          # non-negative like ReLU + GAP features
        k = max(2, min(12, n // 3))
        base = np.abs(r.standard_normal((k, d)))
        x = base[r.randint(0, k, n)] + 0.3 * np.abs(r.standard_normal((n, d)))
    elif kind == "signed":
        x = r.standard_normal((n, d))
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def rowsum_case(case):
    """Embeddings of a row-sum case: for n > 3, row 2 is zero and row n-1 repeats row 1."""
    n, d, kind, seed = case
    x = emb_case(seed, n, d, kind)
    if n > 3:
        x[2] = 0
        x[n - 1] = x[1]
    return x


def rowsum_id(case):
    return f"{case[0]}x{case[1]}-{case[2]}"


def coreset_case(name):
    """(embeddings, labeled, uncertainty, q, mode, moks, lambda) of a core-set case."""
    i = CORESET_NAMES.index(name)
    _, n, d, kind, n_labeled, q, mode, moks, lam = CORESET_CASES[i]
    x = emb_case(700 + i, n, d, kind)
    r = np.random.RandomState(800 + i)
    labeled = np.sort(r.choice(n, n_labeled, replace=False))
    unc = r.random_sample(n)
    unc[labeled] = 0.0
    return x, labeled, unc, q, mode, moks, lam


def held(name, q):
    return HELD.get(name, q)


# ---- the restatement -------------------------------------------------------------------------------------------------------------

def cosine_sums_ref(emb):
    x = np.asarray(emb, np.float64)
    n = x.shape[0]
    norm = np.sqrt((x * x).sum(axis=1))
    zero = norm == 0
    u = x / np.where(zero, 1.0, norm)[:, None]
    out = n - (u * u.sum(axis=0)).sum(axis=1)                        # row by row: equal rows get equal sums
    out[zero] = n - 1
    return out


def center_distances_ref(emb, centers):
    """(n,) distance of every row to the nearest of ``centers``, from direct differences."""
    x = np.asarray(emb, np.float64)
    best = np.full(x.shape[0], np.inf)
    for c in np.asarray(centers, np.int64).reshape(-1):
        diff = x - x[c]
        best = np.minimum(best, np.sqrt((diff * diff).sum(axis=1)))
    return best


def update_ref(emb, centers, prev=None):
    d = center_distances_ref(emb, centers)
    return d if prev is None else np.minimum(np.asarray(prev, np.float64), d)


def score_ref(min_dist, unc, a, b, n=None):
    """fl(a * md) + fl(b * unc), element-wise like numpy: a missing array counts as zeros."""
    n = n if n is not None else len(min_dist if min_dist is not None else unc)
    md = np.zeros(n) if min_dist is None else np.asarray(min_dist, np.float64)[:n]
    u = np.zeros(n) if unc is None else np.asarray(unc, np.float64)[:n]
    with np.errstate(all="ignore"):
        return np.float64(a) * md + np.float64(b) * u


def argmax_ref(score):
    """First arg-max with NaN counted as the maximum, written out (np.argmax behaves the same), and the relative gap to the runner-up."""
    score = np.asarray(score, np.float64)
    nan = np.isnan(score)
    if nan.any():
        return int(np.flatnonzero(nan)[0]), 0.0 if nan.sum() > 1 else np.inf
    best = int(np.flatnonzero(score == score.max())[0])
    if len(score) == 1:
        return best, np.inf
    second = np.delete(score, best).max()
    with np.errstate(all="ignore"):
        gap = (score[best] - second) / abs(score[best]) if score[best] != second else 0.0
    return best, float(gap)


def pick_ref(min_dist, unc, a, b, n=None):
    return argmax_ref(score_ref(min_dist, unc, a, b, n))


def mode_weights(mode, moks, lam):
    return {"kcenter": (1.0, 0.0), "fixed": (1.0, float(lam)), "moks": (1.0 - float(moks), float(lam) * float(moks))}[mode]


def coreset_ref(emb, labeled, uncertainty, q, mode="moks", moks=0.0, lam=1.0, rng=np.random):
    """ActiveLearning.py:798-850 on the restated pieces.  Returns (picks, per-step relative gaps; inf where the step is a random draw)."""
    x = np.asarray(emb, np.float64)
    unc = np.array(uncertainty, np.float64)
    labeled = np.asarray(labeled, np.int64).reshape(-1)
    a, b = mode_weights(mode, moks, lam)
    md = update_ref(x, labeled) if labeled.size else None
    picks, gaps = [], []
    for _ in range(q):
        if md is None:
            i, gap = (int(rng.choice(np.arange(x.shape[0]))), np.inf) if mode == "kcenter" else argmax_ref(unc)
        else:
            i, gap = pick_ref(md, unc, a, b)
        md = update_ref(x, [i], md)
        unc[i] = 0.0
        picks.append(i)
        gaps.append(gap)
    return picks, gaps
