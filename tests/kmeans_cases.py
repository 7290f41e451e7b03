"""Inputs of the K-Means fixture (tests/golden/kmeans.npz, tools/make_kmeans_golden.py): every case's embeddings and weights
come from a seed (numpy freezes RandomState streams), so the fixture holds expected outputs only."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmeans.npz")

# (n, k, seed, weighted)
MAIN_CASES = [(64, 4, 0, False), (257, 13, 1, False), (257, 13, 1, True), (600, 30, 2, True), (1024, 51, 3, False), (1024, 51, 3, True),
              (1024, 154, 4, True), (333, 50, 5, True), (1500, 75, 6, True)]
SMALL_CASES = [(24, 6, 7, False), (18, 6, 7, True), (5, 5, 8, True), (40, 1, 9, False), (2, 2, 10, False)]
TIE_CASE = (17, 16, 12, False)
DEVICE_CASES = MAIN_CASES + SMALL_CASES
ALL_CASES = DEVICE_CASES + [TIE_CASE]
TIE_REL = 1e-9


def emb(n, d=2048, seed=0, tracks=6):
    r = np.random.RandomState(seed)
    base = np.abs(r.standard_normal((tracks, d)))
    t = np.repeat(np.arange(tracks), n // tracks + 1)[:n]
    drift = np.cumsum(r.standard_normal((n, d)) * 0.02, axis=0)
    return np.maximum(base[t] + drift + 0.05 * r.standard_normal((n, d)), 0).astype(np.float32)


def weights(n, seed):
    return 1 + 3 * 0.7 * np.random.RandomState(seed + 100).rand(n)


def case_inputs(case):
    n, k, seed, weighted = case
    return emb(n, seed=seed), (weights(n, seed) if weighted else None)


def case_id(case):
    return f"{case[0]}-{case[1]}-{case[2]}-{'w' if case[3] else 'p'}"


def degenerate():
    """Ten distinct rows, four times: k = 16 leaves clusters empty."""
    return np.concatenate([emb(40, seed=9)[:10]] * 4)


def member_means(x, labels, k, weight=None):
    """Centres recomputed from labels: the weighted mean of each cluster's members in float64 (the fixture holds scikit-learn's
    centres for the small cases only: all fifteen would be 7.8 MB of float64)."""
    x = np.asarray(x, np.float64)
    w = np.ones(len(x)) if weight is None else np.asarray(weight, np.float64)
    c = np.zeros((k, x.shape[1]))
    np.add.at(c, labels, x * w[:, None])
    return c / np.bincount(labels, weights=w, minlength=k)[:, None]


class Golden:
    def __init__(self, path=GOLDEN):
        self.z = np.load(path, allow_pickle=False)
        self.cases = [tuple(int(v) for v in row[:3]) + (bool(row[3]),) for row in self.z["cases"]]

    def get(self, case, name):
        return self.z[f"c{self.cases.index(tuple(case))}_{name}"]

    def has(self, case, name):
        return f"c{self.cases.index(tuple(case))}_{name}" in self.z.files

    def tied_members(self, case, cluster):
        off = self.get(case, "tied_offsets")
        return [int(i) for i in self.get(case, "tied_members")[off[cluster]:off[cluster + 1]]]
