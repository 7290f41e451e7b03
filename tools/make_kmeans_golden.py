"""Writes tests/golden/kmeans.npz: what the installed scikit-learn answers on the K-Means cases of tests/kmeans_cases.py.

    python tools/make_kmeans_golden.py

Per case: labels, n_iter_, inertia_, the representatives the reference picks (ActiveLearning.py:573-576), the seeding indices
of the public sklearn.cluster.kmeans_plusplus on the centred rows with the same seed, per cluster a `tied` flag with the tied
members, cluster_centers_ where they are small (k x 2048 float64 of all fifteen cases would be 7.8 MB next to 35 KB of the rest), and two float64 figures for the centre bound of tests/test_gpu_kmeans.py: how far an independent numpy restatement
of the algorithm lands from scikit-learn's centres, and how far the weighted member means recomputed from the labels do.
The tool checks itself: KMeans started from the stored seeding indices must reproduce the seeded run's labels, or nothing is
written.  Inputs are not stored: they come from the cases' seeds."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.kmeans_cases import ALL_CASES, GOLDEN, TIE_REL, case_inputs, member_means  # noqa: E402

SEED = 318
CENTRES_MAX_BYTES = 128 << 10            # cluster_centers_ are stored for the cases where k x D float64 stays below this


def d2(a, b):
    """Squared distances by direct differences (scikit-learn expands |x|^2 - 2xc + |c|^2: another rounding)."""
    out = np.empty((a.shape[0], b.shape[0]))
    for i in range(a.shape[0]):
        out[i] = ((b - a[i]) ** 2).sum(1)
    return out


def restate_lloyd(xc, k, w, idx, tol, max_iter=300):
    c = xc[idx].copy()
    labels_old = np.full(len(xc), -1)
    strict = False
    for it in range(max_iter):
        labels = d2(xc, c).argmin(1)
        wc = np.bincount(labels, weights=w, minlength=k)
        if (wc == 0).any():
            return None
        cn = np.zeros_like(c)
        np.add.at(cn, labels, xc * w[:, None])
        cn /= wc[:, None]
        shift = ((cn - c) ** 2).sum()
        c = cn
        if np.array_equal(labels, labels_old):
            strict = True
            break
        if shift <= tol:
            break
        labels_old = labels
    if not strict:
        labels = d2(xc, c).argmin(1)
    return labels, c, it + 1


def main():
    import sklearn
    from sklearn.cluster import KMeans, kmeans_plusplus
    out = {"cases": np.array([[n, k, s, int(wt)] for n, k, s, wt in ALL_CASES], np.int64),
           "sklearn_version": np.array(sklearn.__version__), "numpy_version": np.array(np.__version__)}
    for ci, case in enumerate(ALL_CASES):
        n, k, seed, weighted = case
        x32, w = case_inputs(case)
        x = x32.astype(np.float64)
        km = KMeans(n_clusters=k, random_state=SEED)
        labels = km.fit_predict(x, sample_weight=w)
        mean = x.mean(axis=0)
        xc = x - mean
        _, idx = kmeans_plusplus(xc, k, sample_weight=w, random_state=SEED)
        km2 = KMeans(n_clusters=k, init=x[idx], n_init=1, random_state=SEED).fit(x, sample_weight=w)
        if not (np.array_equal(km2.labels_, labels) and km2.n_iter_ == km.n_iter_):
            raise SystemExit(f"case {case}: KMeans from the kmeans_plusplus indices does not reproduce the seeded run; nothing written")
        centres = km.cluster_centers_
        dis = ((x - centres[labels]) ** 2).sum(axis=1)
        reps, tied, members, offsets = [], [], [], [0]
        for j in range(len(np.unique(labels))):
            mem = np.arange(n)[labels == j]
            rep = mem[dis[mem].argmin()]
            near = mem[dis[mem] <= dis[rep] * (1 + TIE_REL)]
            reps.append(rep)
            tied.append(len(near) > 1)
            members.extend(near.tolist() if len(near) > 1 else [])
            offsets.append(len(members))
        p = f"c{ci}_"
        out[p + "labels"] = labels.astype(np.int32)
        out[p + "n_iter"] = np.array(km.n_iter_, np.int64)
        out[p + "inertia"] = np.array(km.inertia_, np.float64)
        if centres.nbytes <= CENTRES_MAX_BYTES:
            out[p + "centres"] = centres
        out[p + "reps"] = np.array(reps, np.int32)
        out[p + "init"] = np.asarray(idx, np.int32)
        out[p + "tied"] = np.array(tied, bool)
        out[p + "tied_members"] = np.array(members, np.int32)
        out[p + "tied_offsets"] = np.array(offsets, np.int32)
        ww = np.ones(n) if w is None else w
        rs = restate_lloyd(xc, k, ww, idx, np.mean(np.var(xc, axis=0)) * 1e-4)
        same = rs is not None and np.array_equal(rs[0], labels) and rs[2] == km.n_iter_
        out[p + "restatement_centre_err"] = np.array(np.abs(rs[1] + mean - centres).max() if same else np.nan, np.float64)
        full = len(np.unique(labels)) == k
        out[p + "recompute_centre_err"] = np.array(np.abs(member_means(xc, labels, k, w) + mean - centres).max() if full else np.nan, np.float64)
        print(case, "iters", km.n_iter_, "tied clusters", int(np.sum(tied)), "restatement same", same, "centre err %.2e" % out[p + "restatement_centre_err"],
              "recompute err %.2e" % out[p + "recompute_centre_err"], flush=True)
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
