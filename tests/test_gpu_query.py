"""The query-selection kernels (csrc/query.hip: cosine row sums, k-center update and pick) at their edges: row and lane tails, more
than one block, the strided loop and the tie-break of the pick, zero / duplicate rows, NaN and -inf scores.  Row sums and whole
selections are held to the reference's scikit-learn calls (oracle/query.py), the single kernels to the float64 restatement of
tests/query_cases.py (which tests/test_query_cpu.py holds to the same oracle)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import query as OQ
from tests import query_cases as QC
from tests.gpu_util import dev, record

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


def f64(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float64)).to(dev())


def i32(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.int32)).to(dev())


def bits(t):
    return t.detach().cpu().numpy().view(np.int64)


# ---- cosine row sums ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", QC.ROWSUM_CASES, ids=QC.rowsum_id)
def test_cosine_rowsum_matches_sklearn(case):
    import vatl_hip as vh
    from active_learning import query as Q
    n = case[0]
    x = QC.rowsum_case(case)
    e = torch.from_numpy(x).to(dev())
    want = OQ.cosine_distance_sums(x)
    got = vh.cosine_rowsum(e)
    again = vh.cosine_rowsum(e)
    via_q = Q.cosine_distance_sums(e)
    got_np = got.cpu().numpy()
    diff = float(np.abs(got_np - want).max())
    print(f"cosine_rowsum {QC.rowsum_id(case)}: max |device - sklearn| = {diff:.3e}" + (f", sums {got_np.tolist()}" if n == 2 else ""))
    record("query_cosine_rowsum", case=QC.rowsum_id(case), max_abs_diff=diff, **({"sums": got_np.tolist(), "minmax": Q.minmax(got_np).tolist()} if n == 2 else {}))
    assert got.dtype == torch.float64 and got.shape == (n,)
    np.testing.assert_allclose(got_np, want, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(via_q, want, rtol=1e-9, atol=1e-9)
    assert np.array_equal(bits(got), bits(again)) and np.array_equal(got_np.view(np.int64), via_q.view(np.int64))
    if n > 3:
        assert got_np[2] == n - 1, got_np[2]                         # the zero row: exactly n - 1
        assert got_np[n - 1] == got_np[1]                            # equal rows, equal sums


@pytest.mark.parametrize("d", [1, 65, 2048])
def test_cosine_rowsum_single_row(d):
    import vatl_hip as vh
    x = QC.emb_case(40 + d, 1, d, "signed")
    got = float(vh.cosine_rowsum(torch.from_numpy(x).to(dev()))[0])
    zero = float(vh.cosine_rowsum(torch.zeros(1, d, device=dev()))[0])
    print(f"cosine_rowsum n=1 D={d}: {got!r}, zero row {zero!r}")
    assert abs(got) <= 1e-9 and zero == 0.0


def test_cosine_rowsum_counts_a_zero_row_once_for_the_others():
    """Every other row is at distance 1 from a zero row: their sums are those of the pool without it, plus 1."""
    import vatl_hip as vh
    x = QC.emb_case(41, 9, 65, "clustered")
    with_zero = np.insert(x, 4, 0, axis=0)
    got = vh.cosine_rowsum(torch.from_numpy(with_zero).to(dev())).cpu().numpy()
    base = QC.cosine_sums_ref(x)
    assert got[4] == 9.0
    np.testing.assert_allclose(np.delete(got, 4), base + 1, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("kind", QC.KINDS)
def test_diversity_order_with_duplicate_rows(kind):
    from active_learning import query as Q
    case = next(c for c in QC.ROWSUM_CASES if c[:3] == (257, 100, kind))
    x = QC.rowsum_case(case)
    cand = list(range(1000, 1257))
    want = np.argsort(OQ.cosine_distance_sums(x), kind="stable")     # rows 1 and 256 are equal: bit-equal sums, index order
    assert Q.diversity_queries(torch.from_numpy(x).to(dev()), cand, 257) == [cand[i] for i in want]


# ---- kcenter_update ----------------------------------------------------------------------------------------------------------------

UPDATE_REL = 1e-12       # a float64 sum of D <= 2048 non-negative terms is within (D-1) * 2^-53 = 2.3e-13 of exact in any order; sqrt halves it
SENTINEL = -12345.5


def _check_update(x, e, centers, prev, first, tag):
    import vatl_hip as vh
    n = x.shape[0]
    buf = torch.full((n + 5,), SENTINEL, device=dev(), dtype=torch.float64)
    buf[:n] = f64(np.full(n, NAN) if first else prev)
    vh.kcenter_update(e, i32(centers), buf[:n], first=first)
    out = buf.cpu().numpy()
    want = QC.update_ref(x, centers, None if first else prev)
    got = out[:n]
    assert np.all(out[n:] == SENTINEL), (tag, out[n:])
    assert np.all(np.isfinite(got)), (tag, got)
    err = float(np.max(np.abs(got - want) / np.where(want > 0, want, 1.0)))
    assert np.all(np.abs(got - want) <= UPDATE_REL * want), (tag, err)       # want == 0 (a centre, or an equal row) asks for exactly 0.0
    if first:
        assert np.all(got[np.asarray(centers)] == 0.0), tag
    return err


@pytest.mark.parametrize("d", [1, 63, 64, 65, 2048])
def test_kcenter_update_edges(d):
    worst = 0.0
    for n in (1, 3, 4, 5, 130):
        x = QC.emb_case(900 + d + n, n, d, QC.KINDS[(n + d) % 2])
        e = torch.from_numpy(x).to(dev())
        r = np.random.RandomState(n * 7 + d)
        one = [int(r.randint(0, n))]
        seven = r.randint(0, n, 7)                                   # in range by construction; repeats allowed (n < 7)
        scale = float(np.median(QC.center_distances_ref(x, seven))) or 1.0
        prev = scale * (0.5 + r.random_sample(n))                    # some earlier values survive, some are replaced
        for centers, first in ((one, True), (seven, True), (one, False), (seven, False)):
            worst = max(worst, _check_update(x, e, centers, prev, first, (n, d, len(centers), first)))
    print(f"kcenter_update D={d}: max relative error {worst:.3e}")
    record("query_kcenter_update", d=d, max_rel_err=worst)


def test_kcenter_update_200_centres():
    n, d = 1500, 48
    x = QC.emb_case(990, n, d, "clustered")
    e = torch.from_numpy(x).to(dev())
    r = np.random.RandomState(991)
    centers = np.sort(r.choice(n, 200, replace=False))
    prev = 2.0 * r.random_sample(n)
    worst = max(_check_update(x, e, centers, prev, True, "200 first"), _check_update(x, e, centers, prev, False, "200 min"))
    print(f"kcenter_update 1500x48, 200 centres: max relative error {worst:.3e}")
    record("query_kcenter_update", d=d, n=n, centres=200, max_rel_err=worst)


# ---- kcenter_pick ------------------------------------------------------------------------------------------------------------------

def _pick(md, unc, a, b, n=None, step=2):
    """Run one pick over copies; checks the side effects and returns the picked index."""
    import vatl_hip as vh
    n = n if n is not None else len(md if md is not None else unc)
    md_t = None if md is None else f64(md)
    unc_t = None if unc is None else f64(unc)
    sel = torch.full((4,), -7, device=dev(), dtype=torch.int32)
    vh.kcenter_pick(md_t, unc_t, a, b, sel, step, n)
    out = sel.cpu().numpy()
    picked = int(out[step])
    assert np.all(np.delete(out, step) == -7), out                   # only sel[step] is written
    assert 0 <= picked < n
    if md is not None:
        assert np.array_equal(bits(md_t), np.ascontiguousarray(md, np.float64).view(np.int64))
    if unc is not None:
        after, before = unc_t.cpu().numpy(), np.array(unc, np.float64)
        assert after[picked] == 0.0 and not np.signbit(after[picked])
        before[picked] = 0.0
        assert np.array_equal(after.view(np.int64), before.view(np.int64))      # nothing else in unc changes
    return picked


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 1025, 5000])
def test_kcenter_pick_sizes_and_variants(n):
    r = np.random.RandomState(1200 + n)
    md, unc = 3.0 * r.random_sample(n + 3), r.random_sample(n + 3)   # three entries past n: larger than any score, never to be picked
    md[n:], unc[n:] = 100.0, 100.0
    for step, (m, u, a, b) in enumerate([(md, unc, 0.4, 0.6), (None, unc, 0.0, 1.0), (md, None, 1.0, 0.0), (md, unc, 0.0, 0.7), (md, unc, 0.3, 0.0),
                                         (md, unc, 1.0, 0.5), (None, unc, 0.4, 0.6), (md, None, 0.4, 0.6)]):
        want, gap = QC.pick_ref(m, u, a, b, n)
        assert gap > 1e-12 or n == 1, (n, step, gap)                 # random doubles: one maximum
        assert _pick(m, u, a, b, n, step % 4) == want, (n, step, a, b)


@pytest.mark.parametrize("lo,hi", [(70, 4097), (7, 1030), (100, 900), (0, 4999), (63, 64), (1023, 1024)])
def test_kcenter_pick_breaks_ties_towards_the_lower_index(lo, hi):
    """Equal maxima in two iterations of different threads (70, 4097), with the lower index in the higher lane (7, 1030), in different
    waves (100, 900), and across the wave / stride boundaries: np.argmax returns the first."""
    n = 5000
    md = np.random.RandomState(lo).random_sample(n)
    md[[lo, hi]] = 2.0
    assert QC.pick_ref(md, None, 1.0, 0.0)[0] == lo
    assert _pick(md, None, 1.0, 0.0) == lo
    unc = md.copy()
    assert _pick(None, unc, 0.0, 1.0) == lo
    assert _pick(md[::-1].copy(), None, 1.0, 0.0) == n - 1 - hi     # mirrored: the pair sits in other lanes and waves


@pytest.mark.parametrize("n", [1, 4, 65, 5000])
def test_kcenter_pick_all_minus_inf_and_all_nan(n):
    assert _pick(np.full(n, -INF), None, 1.0, 0.0) == 0
    assert _pick(np.full(n, NAN), None, 1.0, 0.0) == 0
    assert _pick(np.full(n, NAN), np.zeros(n), 1.0, 1.0) == 0


def test_kcenter_pick_nan_is_the_maximum():
    assert _pick(np.array([1.0, NAN, 2.0, NAN]), None, 1.0, 0.0) == 1
    assert _pick(None, np.array([1.0, NAN, 2.0, NAN]), 0.0, 1.0) == 1
    for nans, want in (((4097, 70), 70), ((3000,), 3000), ((900, 100, 4999), 100), ((1030, 7), 7), ((4999,), 4999)):
        md = np.random.RandomState(5).random_sample(5000)
        md[5] = 50.0                                                 # the largest finite score loses to any NaN
        md[list(nans)] = NAN
        assert int(np.argmax(md)) == want and QC.pick_ref(md, None, 1.0, 0.0)[0] == want
        assert _pick(md, None, 1.0, 0.0) == want, nans


def test_kcenter_pick_rounds_both_products():
    """numpy rounds a*md and b*unc before adding them; the two scores below then tie bit for bit and np.argmax returns 0.  A contracted
    mul + fma makes item 1 one ulp larger."""
    assert _pick(QC.FUSED_MIN_DIST, QC.FUSED_UNC, QC.FUSED_A, QC.FUSED_B) == 0
    md, unc = np.zeros(1500), np.zeros(1500)                         # the same pair in other lanes and waves of the strided loop
    md[[200, 1300]], unc[[200, 1300]] = QC.FUSED_MIN_DIST, QC.FUSED_UNC
    assert _pick(md, unc, QC.FUSED_A, QC.FUSED_B) == 200


# ---- the greedy loop ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", QC.CORESET_NAMES)
def test_coreset_selection_matches_oracle(name):
    from active_learning import query as Q
    x, labeled, unc, q, mode, moks, lam = QC.coreset_case(name)
    e = torch.from_numpy(x).to(dev())
    want = OQ.coreset_selection(x, labeled, unc.copy(), q, mode, moks, lam, rng=np.random.RandomState(QC.RNG_SEED))
    unc_in = unc.copy()
    got = Q.coreset_selection(e, labeled, unc_in, q, mode, moks, lam, rng=np.random.RandomState(QC.RNG_SEED))
    again = Q.coreset_selection(e, labeled.tolist(), unc.copy(), q, mode, moks, lam, rng=np.random.RandomState(QC.RNG_SEED))
    h = QC.held(name, q)
    _, gaps = QC.coreset_ref(x, labeled, unc, q, mode, moks, lam, rng=np.random.RandomState(QC.RNG_SEED))
    print(f"coreset {name}: {got}")
    record("query_coreset", case=name, picks=got, min_gap=float(min(gaps[:h])))
    assert got[:h] == want[:h], (name, got, want, gaps)
    assert got[h:] == [0] * (q - h), (name, got)                     # pool exhausted: arg-max of an all-zero score
    assert got == again
    assert np.array_equal(unc_in, unc)                               # the caller's uncertainty is not written


# ---- argument checks ---------------------------------------------------------------------------------------------------------------

def test_argument_checks_through_the_c_abi():
    import vatl_hip as vh
    lib = vh.lib()
    n, d = 9, 5
    emb = torch.ones(n, d, device=dev())
    out, ws, md, unc = (torch.full((m,), 3.0, device=dev(), dtype=torch.float64) for m in (n, n + d, n, n))
    cen = torch.zeros(2, device=dev(), dtype=torch.int32)
    sel = torch.full((4,), -7, device=dev(), dtype=torch.int32)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    bad = [
        lambda: lib.vatl_cosine_rowsum(None, n, d, P(out), P(ws), None),
        lambda: lib.vatl_cosine_rowsum(P(emb), n, d, None, P(ws), None),
        lambda: lib.vatl_cosine_rowsum(P(emb), n, d, P(out), None, None),
        lambda: lib.vatl_cosine_rowsum(P(emb), n, 0, P(out), P(ws), None),
        lambda: lib.vatl_cosine_rowsum(P(emb), n, -3, P(out), P(ws), None),
        lambda: lib.vatl_kcenter_update(None, n, d, P(cen), 2, P(md), 1, None),
        lambda: lib.vatl_kcenter_update(P(emb), n, d, None, 2, P(md), 1, None),
        lambda: lib.vatl_kcenter_update(P(emb), n, d, P(cen), 2, None, 1, None),
        lambda: lib.vatl_kcenter_update(P(emb), n, 0, P(cen), 2, P(md), 1, None),
        lambda: lib.vatl_kcenter_pick(P(md), P(unc), 1.0, 1.0, None, 0, n, None),
        lambda: lib.vatl_kcenter_pick(P(md), P(unc), 1.0, 1.0, P(sel), -1, n, None),
        lambda: lib.vatl_kcenter_pick(None, None, 1.0, 1.0, P(sel), 0, n, None),
        lambda: lib.vatl_kcenter_pick(P(md), P(unc), 1.0, 1.0, P(sel), 0, 0, None),       # an empty pool has no arg-max
    ]
    for i, call in enumerate(bad):
        assert call() == -1, i                                       # VATL_EINVAL
        assert b"cosine_rowsum" in lib.vatl_last_error() or b"kcenter" in lib.vatl_last_error(), i
    # n = 0 (and no centres) is a no-op for the two calls that allow it
    assert lib.vatl_cosine_rowsum(P(emb), 0, d, P(out), P(ws), None) == 0
    assert lib.vatl_kcenter_update(P(emb), 0, d, P(cen), 2, P(md), 1, None) == 0
    assert lib.vatl_kcenter_update(P(emb), n, d, P(cen), 0, P(md), 1, None) == 0
    torch.cuda.synchronize()
    for t in (out, ws, md, unc):                                     # nothing was launched
        assert bool((t == 3.0).all())
    assert bool((sel == -7).all()) and bool((cen == 0).all())


def test_argument_checks_through_the_wrappers():
    import vatl_hip as vh
    n, d = 9, 5
    emb = torch.ones(n, d, device=dev())
    md, unc = (torch.full((n,), 3.0, device=dev(), dtype=torch.float64) for _ in range(2))
    cen = torch.zeros(2, device=dev(), dtype=torch.int32)
    sel = torch.full((4,), -7, device=dev(), dtype=torch.int32)
    wide = torch.ones(n, 2 * d, device=dev())
    bad = [
        lambda: vh.cosine_rowsum(emb.double()),
        lambda: vh.cosine_rowsum(emb[0]),
        lambda: vh.cosine_rowsum(wide[:, :d]),                                           # not contiguous
        lambda: vh.kcenter_update(emb.double(), cen, md, first=True),
        lambda: vh.kcenter_update(emb.reshape(-1), cen, md, first=True),
        lambda: vh.kcenter_update(wide[:, ::2], cen, md, first=True),
        lambda: vh.kcenter_update(emb, cen.long(), md, first=True),
        lambda: vh.kcenter_update(emb, cen, md[:n - 1], first=True),                     # min_dist shorter than n
        lambda: vh.kcenter_update(emb, cen, md.float(), first=True),
        lambda: vh.kcenter_pick(md[:n - 1], unc, 1.0, 1.0, sel, 0, n),
        lambda: vh.kcenter_pick(md, unc[:n - 1], 1.0, 1.0, sel, 0, n),
        lambda: vh.kcenter_pick(md, unc, 1.0, 1.0, sel, 4, n),                           # step past the end of selected
        lambda: vh.kcenter_pick(md, unc, 1.0, 1.0, sel, -1, n),
        lambda: vh.kcenter_pick(md, unc, 1.0, 1.0, sel.long(), 0, n),
        lambda: vh.kcenter_pick(None, None, 1.0, 1.0, sel, 0, n),
        lambda: vh.kcenter_pick(md, unc, 1.0, 1.0, sel, 0, 0),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            raise AssertionError(f"call {i} was accepted")
    torch.cuda.synchronize()
    assert bool((md == 3.0).all()) and bool((unc == 3.0).all()) and bool((sel == -7).all())    # nothing was launched
    # n = 0 is a no-op where it is allowed
    assert vh.cosine_rowsum(torch.empty(0, d, device=dev())).shape == (0,)
    vh.kcenter_update(torch.empty(0, d, device=dev()), cen, md, first=True)
    vh.kcenter_update(emb, cen[:0], md, first=False)                                     # no centres: min_dist stays
    torch.cuda.synchronize()
    assert bool((md == 3.0).all())
