"""Query selection on the device embeddings (reference: ActiveLearning.py:467-617, 798-850).

What the reference computes with sklearn on a host float64 ``fvecs_matrix`` after every evaluation pass:

  influence / diversity   row sums of the all-pairs cosine-distance matrix        -> ``vatl_cosine_rowsum``
  core-set                k-center greedy over Euclidean distances (+ uncertainty) -> ``vatl_kcenter_update`` / ``_pick``
  K-Means / weighted      sklearn ``KMeans(n_clusters=query_size, random_state=318)``     -> ``vatl_kmeans_*`` (``kmeans_fit``)

The embeddings never leave the GPU; the greedy loop chains pick -> update launches on the stream without host round
trips and copies the selected indices back once.

K-Means restates scikit-learn 1.7's seeded run (k-means++ seeding, one Lloyd run, float64) so that it selects the same
items: the random draws depend on the seed, n, k and the weights only and are made on the host in scikit-learn's order, the
seeding steps are chained on the stream, and each Lloyd iteration reads four scalars back for the stop rule.  Where
scikit-learn's own answer hangs on its rounding (an empty cluster, tied seeding candidates) the call is handed back to
scikit-learn on the host, and the result says so.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

import vatl_hip as vh


def minmax(v: np.ndarray) -> np.ndarray:
    """(v - min) / (max - min) exactly as the reference writes it (nan when all values are equal, like numpy)."""
    v = np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        return (v - np.min(v)) / (np.max(v) - np.min(v))


def cosine_distance_sums(emb: torch.Tensor) -> np.ndarray:
    """(n, D) device embeddings -> (n,) float64: np.sum(KNeighborsTransformer(mode='distance', metric='cosine',
    n_neighbors=n-1).fit_transform(emb), axis=1)   (ActiveLearning.py:471-473, 585-587)."""
    return vh.cosine_rowsum(emb.float().contiguous()).cpu().numpy()


def influence_scores(emb: torch.Tensor) -> np.ndarray:
    """Normalised influence score of the unlabeled items (ActiveLearning.py:467-476)."""
    n = emb.shape[0]
    if n in (0, 1):
        return np.zeros(n)
    return minmax(cosine_distance_sums(emb))


def diversity_queries(emb: torch.Tensor, candidate_list, query_size: int):
    """filter == 'Diversity' (ActiveLearning.py:583-592): candidates with the SMALLEST distance sums first."""
    score = cosine_distance_sums(emb)
    order = np.argsort(score, kind="stable")                     # sorted(dict.items(), key=score) is stable too
    return [int(candidate_list[i]) for i in order[:query_size]]


def coreset_selection(emb: torch.Tensor, labeled_idx, uncertainty: np.ndarray, query_size: int, mode: str = "moks", moks: float = 0.0,
                      unc_lambda: float = 1.0, rng=np.random):
    """k-center greedy (ActiveLearning.py:798-850).  ``emb`` (N, D) covers the whole pool, ``uncertainty`` (N,) is 0 on
    labeled items.  mode: 'kcenter' (no uncertainty term), 'fixed' (min_dist + lambda*unc), 'moks'
    ((1-moks)*min_dist + lambda*moks*unc).  Returns the selected pool indices in selection order."""
    emb = emb.float().contiguous()
    n = emb.shape[0]
    dev = emb.device
    labeled = np.asarray(labeled_idx, np.int64).reshape(-1)
    a, b = {"kcenter": (1.0, 0.0), "fixed": (1.0, float(unc_lambda)), "moks": (1.0 - float(moks), float(unc_lambda) * float(moks))}[mode]
    unc = torch.as_tensor(np.asarray(uncertainty, np.float64), device=dev).contiguous()
    min_dist = torch.empty(n, device=dev, dtype=torch.float64)
    sel = torch.zeros(max(query_size, 1), device=dev, dtype=torch.int32)
    have = labeled.size > 0
    if have:
        vh.kcenter_update(emb, torch.as_tensor(labeled, dtype=torch.int32, device=dev), min_dist, first=True)
    for step in range(query_size):
        if not have:                                             # no labeled item yet (reference: len(labeled_idx) == 0)
            if mode == "kcenter":
                sel[step] = int(rng.choice(np.arange(n)))
                unc[int(sel[step])] = 0.0
            else:
                vh.kcenter_pick(None, unc, 0.0, 1.0, sel, step, n)       # np.argmax(uncertainty)
        else:
            vh.kcenter_pick(min_dist, unc, a, b, sel, step, n)
        vh.kcenter_update(emb, sel[step:step + 1], min_dist, first=not have)
        have = True
    return [int(i) for i in sel[:query_size].cpu().numpy()]


KMEANS_SEED = 318                                                # the reference's random_state (ActiveLearning.py:556, 596)
KMEANS_MAX_ITER, KMEANS_MAX_TRIALS = 300, 16


@dataclasses.dataclass
class KMeansResult:
    """What ``kmeans_fit`` returns.  path: "device" or "host"; reason: why the host ran (None on the device path)."""
    labels: np.ndarray                                           # (n,) int32
    centers: np.ndarray                                          # (k, D) float64, uncentred like ``cluster_centers_``
    n_iter: int
    inertia: float
    init_indices: np.ndarray | None                              # (k,) seeding indices (None when scikit-learn seeded)
    path: str
    reason: str | None = None
    representatives: list | None = None                          # per cluster with members, in label order: the member nearest its centre


class KMeansQueries(tuple):
    """``(queried candidates, picked rows)`` of ``kmeans_queries``, plus which path ran: .path, .reason, .n_iter."""
    def __new__(cls, query, picks, path, reason=None, n_iter=None):
        self = super().__new__(cls, (query, picks))
        self.path, self.reason, self.n_iter = path, reason, n_iter
        return self


def kmeans_draws(n: int, k: int, weight=None, seed: int = KMEANS_SEED):
    """Every random number of scikit-learn's k-means++ (``_kmeans_plusplus``), in its order: the first centre, then per
    further centre ``2 + int(log(k))`` uniform draws.  They depend on the seed, n, k and the weights only.
    Returns (first index, (k-1, trials) float64)."""
    rs = np.random.RandomState(seed)
    w = np.ones(n) if weight is None else np.asarray(weight, np.float64)
    trials = 2 + int(np.log(k))
    first = int(rs.choice(n, p=w / w.sum()))
    draws = np.stack([rs.uniform(size=trials) for _ in range(k - 1)]) if k > 1 else np.zeros((0, trials))
    return first, draws


def _host_kmeans(emb_np, k, weight, seed):
    try:
        from sklearn.cluster import KMeans
    except ImportError as e:                                     # pragma: no cover
        raise ValueError("Filter type is not supported (K-Means needs scikit-learn on the host)") from e
    learner = KMeans(n_clusters=k, random_state=seed)
    labels = learner.fit_predict(emb_np, sample_weight=weight) if weight is not None else learner.fit_predict(emb_np)
    return learner, labels


def _host_picks(emb_np, labels, centers):
    cluster_num = len(np.unique(labels))
    dis = ((emb_np - centers[labels]) ** 2).sum(axis=1)
    return [np.arange(emb_np.shape[0])[labels == i][dis[labels == i].argmin()] for i in range(cluster_num)]


def _host_fit(emb: torch.Tensor, k, weight, seed, reason) -> KMeansResult:
    emb_np = emb.double().cpu().numpy()
    learner, labels = _host_kmeans(emb_np, k, weight, seed)
    return KMeansResult(labels.astype(np.int32), learner.cluster_centers_, int(learner.n_iter_), float(learner.inertia_), None, "host", reason,
                        [int(i) for i in _host_picks(emb_np, labels, learner.cluster_centers_)])


def _device_seeding(xc, w, w_np, k, seed):
    n = xc.shape[0]
    first, draws = kmeans_draws(n, k, w_np, seed)
    if draws.shape[1] > KMEANS_MAX_TRIALS:
        raise ValueError("K-Means: too many clusters")
    return vh.kmeans_seed(xc, w, k, first, vh.upload(draws.reshape(-1), xc.device) if k > 1 else None, draws.shape[1])


def kmeans_seeding(emb: torch.Tensor, k: int, weight=None, seed: int = KMEANS_SEED):
    """The k-means++ stage alone: (k seeding indices, tie flag) of (n, D) device embeddings."""
    emb = emb.float().contiguous()
    w_np = None if weight is None else np.ascontiguousarray(weight, np.float64)
    w = torch.ones(emb.shape[0], device=emb.device, dtype=torch.float64) if w_np is None else vh.upload(w_np, emb.device)
    out = _device_seeding(vh.kmeans_prepare(emb)[0], w, w_np, int(k), seed).cpu().numpy()
    return out[:k].copy(), bool(out[k])


def kmeans_fit(emb: torch.Tensor, k: int, weight=None, seed: int = KMEANS_SEED, init_indices=None) -> KMeansResult:
    """scikit-learn's ``KMeans(n_clusters=k, random_state=seed).fit(emb, sample_weight=weight)`` on (n, D) device embeddings.
    ``init_indices`` (k rows of ``emb``) replaces the k-means++ seeding.  D must be a multiple of 16 (the MFMA assignment's
    column step; the embeddings are 2048 wide): any other width raises ``VatlError``, it is not handed back."""
    return _kmeans_fit(emb, k, weight, seed, init_indices, True)


def _kmeans_fit(emb, k, weight, seed, init_indices, readback) -> KMeansResult:
    """``readback=False`` leaves labels and centres on the device (``labels`` / ``centers`` None, ``inertia`` nan): the filters
    need the representatives only."""
    emb = emb.float().contiguous()
    n, d = emb.shape
    k = int(k)
    if not 1 <= k <= n:
        raise ValueError(f"n_samples={n} should be >= n_clusters={k}.")
    dev = emb.device
    w_np = None if weight is None else np.ascontiguousarray(weight, np.float64)
    w = torch.ones(n, device=dev, dtype=torch.float64) if w_np is None else vh.upload(w_np, dev)
    xc, mean, tol = vh.kmeans_prepare(emb)
    if init_indices is None:
        seeded = _device_seeding(xc, w, w_np, k, seed)
        seeded_np = seeded.cpu().numpy()                         # the indices and the tie flag: one read-back
        if seeded_np[k]:
            return _host_fit(emb, k, w_np, seed, "tied seeding candidates")
        idx = seeded[:k].long()
        init_np = seeded_np[:k].copy()
    else:
        init_np = np.asarray(init_indices, np.int32).reshape(-1)
        if init_np.size != k or init_np.min() < 0 or init_np.max() >= n:
            raise ValueError("init_indices: need k row indices")
        idx = torch.as_tensor(init_np, device=dev).long()
    centers, centers_new = xc[idx].contiguous(), torch.empty((k, d), device=dev, dtype=torch.float64)
    labels, labels_old = torch.empty(n, device=dev, dtype=torch.int32), torch.empty(n, device=dev, dtype=torch.int32)
    status = torch.zeros(4, device=dev, dtype=torch.float64)     # changed, total squared shift, empty cluster, tol
    status[3:] = tol
    ws = torch.empty(max(k, vh.kmeans_update_workspace_doubles(d, k)), device=dev, dtype=torch.float64)
    strict, n_iter = False, 0
    for it in range(KMEANS_MAX_ITER):
        vh.kmeans_assign(xc, centers, labels_old if it else None, labels, status, ws)
        vh.kmeans_update(xc, w, labels, centers, centers_new, status, ws)
        changed, shift, empty, tol_abs = status.tolist()         # the iteration's one read-back
        if empty:
            return _host_fit(emb, k, w_np, seed, "empty cluster")
        centers, centers_new = centers_new, centers
        n_iter = it + 1
        if not changed:
            strict = True
            break
        if shift <= tol_abs:
            break
        labels, labels_old = labels_old, labels
    if not strict:
        vh.kmeans_assign(xc, centers, None, labels, status, ws)
    reps, inertia = vh.kmeans_finish(emb, xc, mean, w, centers, labels)
    reps_np = reps.cpu().numpy()
    if (reps_np < 0).any():                                      # the last assignment left a cluster without members
        return _host_fit(emb, k, w_np, seed, "empty cluster")
    return KMeansResult(labels.cpu().numpy() if readback else None, (centers + mean).cpu().numpy() if readback else None, n_iter,
                        float(inertia.item()) if readback else float("nan"), init_np, "device", None, [int(i) for i in reps_np])


def unique_rows(emb: torch.Tensor):
    """``np.unique(emb, axis=0, return_index=True)`` on the device: the distinct rows in lexicographic order and, on the host,
    the index of each one's first occurrence."""
    uniq, inverse = torch.unique(emb, dim=0, return_inverse=True)
    n = emb.shape[0]
    first = torch.full((uniq.shape[0],), n, device=emb.device, dtype=torch.long)
    first.scatter_reduce_(0, inverse, torch.arange(n, device=emb.device), reduce="amin")
    return uniq, first.cpu().numpy()


def kmeans_queries(emb, candidate_list, query_size: int, weight=None):
    """filters 'K-Means' / 'weighted' (ActiveLearning.py:553-582, 595-611): cluster, then the member closest to its
    centre represents each cluster.  A device tensor takes ``kmeans_fit``; numpy rows run sklearn on the host exactly as
    the reference does.  Returns ``(queried candidates, picked rows)`` as a ``KMeansQueries``."""
    if isinstance(emb, torch.Tensor) and emb.is_cuda:
        res = _kmeans_fit(emb, query_size, weight, KMEANS_SEED, None, False)
        picks = res.representatives
        return KMeansQueries([int(candidate_list[i]) for i in picks], picks, res.path, res.reason, res.n_iter)
    emb_np = np.asarray(emb, np.float64)
    learner, cluster_idxs = _host_kmeans(emb_np, query_size, weight, KMEANS_SEED)
    picks = _host_picks(emb_np, cluster_idxs, learner.cluster_centers_)
    return KMeansQueries([int(candidate_list[i]) for i in picks], picks, "host", "numpy input", int(learner.n_iter_))
