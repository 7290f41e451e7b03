"""kmeans_fit's host side without a GPU: the stop rule, the buffer hand-over between iterations and the two hand-backs, driven
with numpy stand-ins for the vatl_kmeans_* entry points (each restates what include/vatl_hip.h says the entry point computes).
The kernels themselves are checked on the device in tests/test_gpu_kmeans.py."""
import warnings

import numpy as np
import pytest
import torch

from tests import kmeans_cases as KC


def _d2(a, b):
    return np.stack([((b - a[i]) ** 2).sum(1) for i in range(len(a))])


def _prepare(emb):
    x = emb.double().numpy()
    m = x.mean(0)
    xc = x - m
    return torch.from_numpy(xc), torch.from_numpy(m), torch.tensor([np.mean(np.var(xc, axis=0)) * 1e-4], dtype=torch.float64)


def _seed(xc, w, k, first, draws, trials):
    xc, ww = xc.numpy(), w.numpy()
    n = len(xc)
    dr = draws.numpy().reshape(-1, trials) if draws is not None else None
    idx, closest, flag = [first], _d2(xc[[first]], xc)[0], 0
    pot = closest @ ww
    for c in range(1, k):
        cand = np.minimum(np.searchsorted(np.cumsum(ww * closest), dr[c - 1] * pot), n - 1)
        dc = np.minimum(closest, _d2(xc[cand], xc))
        pots = dc @ ww
        b = int(np.argmin(pots))
        if any(cand[t] != cand[b] and (pots[b] == 0 or pots[t] - pots[b] <= KC.TIE_REL * pots[b]) for t in range(len(cand))):
            flag = 1
        pot, closest = pots[b], dc[b]
        idx.append(int(cand[b]))
    return torch.tensor(idx + [flag], dtype=torch.int32)


def _assign(xc, c, prev, labels, status, ws):
    x, cc = xc.numpy(), c.numpy()
    lab = ((cc ** 2).sum(1)[None] - 2 * x @ cc.T).argmin(1).astype(np.int32)
    status[0] = 1.0 if prev is None or not np.array_equal(prev.numpy(), lab) else 0.0
    status[2] = 0.0
    labels.copy_(torch.from_numpy(lab))


def _update(xc, w, labels, c, cn, status, ws):
    x, ww, lab, k = xc.numpy(), w.numpy(), labels.numpy(), c.shape[0]
    wc = np.bincount(lab, weights=ww, minlength=k)
    new = np.zeros((k, x.shape[1]))
    np.add.at(new, lab, x * ww[:, None])
    empty = wc == 0
    new = new * (1 / np.where(empty, 1, wc))[:, None]
    new[empty] = c.numpy()[empty]
    status[1] = ((new - c.numpy()) ** 2).sum()
    status[2] = 1.0 if empty.any() else 0.0
    cn.copy_(torch.from_numpy(new))


def _finish(emb, xc, mean, w, c, labels):
    x, lab, cc = xc.numpy(), labels.numpy(), c.numpy()
    inertia = (w.numpy() * ((x - cc[lab]) ** 2).sum(1)).sum()
    dis = ((emb.double().numpy() - (cc + mean.numpy())[lab]) ** 2).sum(1)
    reps = []
    for j in range(len(cc)):
        mem = np.flatnonzero(lab == j)
        reps.append(-1 if len(mem) == 0 else int(mem[dis[mem] <= dis[mem].min() * (1 + KC.TIE_REL)].min()))
    return torch.tensor(reps, dtype=torch.int32), torch.tensor([inertia], dtype=torch.float64)


@pytest.fixture
def Q(monkeypatch):
    import vatl_hip as vh
    from active_learning import query
    for name, fn in (("kmeans_prepare", _prepare), ("kmeans_seed", _seed), ("kmeans_assign", _assign), ("kmeans_update", _update),
                     ("kmeans_finish", _finish), ("upload", lambda h, d, **kw: torch.as_tensor(h)),
                     ("kmeans_update_workspace_doubles", lambda d, k: 8 * k)):
        monkeypatch.setattr(vh, name, fn)
    return query


@pytest.mark.parametrize("case", [c for c in KC.DEVICE_CASES if c[0] <= 600], ids=KC.case_id)
def test_flow_reproduces_the_fixture(Q, case):
    golden = KC.Golden()
    x, w = KC.case_inputs(case)
    for init in (None, golden.get(case, "init")):
        res = Q.kmeans_fit(torch.from_numpy(x), case[1], w, init_indices=init)
        assert res.path == "device" and res.reason is None
        assert np.array_equal(res.init_indices, golden.get(case, "init"))
        assert np.array_equal(res.labels, golden.get(case, "labels")) and res.n_iter == int(golden.get(case, "n_iter"))
        np.testing.assert_allclose(res.inertia, float(golden.get(case, "inertia")), rtol=2048 * np.finfo(np.float64).eps, atol=0)
        tied, want = golden.get(case, "tied"), golden.get(case, "reps")
        assert res.representatives == [min(golden.tied_members(case, j)) if tied[j] else int(want[j]) for j in range(len(want))]


def test_flow_hands_back(Q):
    pytest.importorskip("sklearn")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x = KC.case_inputs(KC.TIE_CASE)[0]
        res = Q.kmeans_fit(torch.from_numpy(x), 16)
        assert (res.path, res.reason) == ("host", "tied seeding candidates") and res.init_indices is None
        assert np.array_equal(res.labels, KC.Golden().get(KC.TIE_CASE, "labels"))
        deg = torch.from_numpy(KC.degenerate())
        assert Q.kmeans_fit(deg, 16).path == "host"
        res = Q.kmeans_fit(deg, 16, init_indices=np.arange(16))
        assert (res.path, res.reason) == ("host", "empty cluster")
    with pytest.raises(ValueError):
        Q.kmeans_fit(deg[:3], 4)
