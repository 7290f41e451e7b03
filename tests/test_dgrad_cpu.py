"""tests/dgrad_cases.py before anything trusts it (no GPU): the host model of conv2d_fwd_ex on the host-stated filter packing, assembled as
hip_train._igemm_dgrad assembles it, is float64 autograd; the impulse expectation is autograd of the impulse; the integer regime cannot round; the
claims of the case comments follow from the restated dispatch rules; the restated launch logic is the trainer's, line for line."""
import ast
import os

import numpy as np
import pytest

from tests import dgrad_cases as D

IDS = [D.case_id(c) for c in D.CASES]
SMALL = [c for c in D.CASES if c.route != D.STREAMK]                      # the two stream-K cases cost seconds per host reference: once each
SMALL_IDS = [D.case_id(c) for c in SMALL]


def test_case_names_are_unique_and_every_route_is_covered():
    assert len(set(IDS)) == len(IDS) and len(set(D.CASES)) == len(D.CASES) and set(D.CLAIMS) == set(D.CASES)
    assert len({D.seed(c) for c in D.CASES}) == len(D.CASES)
    assert {c.route for c in D.CASES} == {D.IGEMM, D.PERSISTENT, D.RING, D.STREAMK, D.WINO, D.WINO_2H, D.WINO_PERSIST}
    assert all(c.coutk % 32 == 0 and c.coutk >= c.cout for c in D.CASES if not D.is_winograd(c))
    assert all(c.cout % 16 == 0 and c.cin % 16 == 0 and (c.cout % 32 or c.cin % 32) for c in D.CASES if D.is_winograd(c))


def _forms(case):
    """The forms of a case: (residual?, launches to issue)."""
    n = len(D.launches(case))
    forms = [(False, None), (True, None)]
    if n == 4:
        forms += [(True, (i,)) for i in range(4)]
    return forms


# (the two large cases are held to autograd once, in the exact regime)
MODEL_RUNS = [(c, "integer") for c in D.CASES] + [(c, "random") for c in SMALL]


@pytest.mark.parametrize("case,regime", MODEL_RUNS, ids=[f"{D.case_id(c)}-{r}" for c, r in MODEL_RUNS])
def test_host_model_on_the_host_packing_is_autograd(case, regime):
    dz, w, res = D.inputs(case, regime)
    assert dz.dtype == w.dtype == res.dtype == np.float32 and not dz[..., case.cout:].any() and dz[..., :case.cout].any()
    ref = D.reference(case, dz, w)
    assert ref.dtype == np.float64 and ref.shape == (case.n, case.h, case.w, case.cin)
    for with_res, only in _forms(case):
        got = D.dgrad_model(case, dz, w, res if with_res else None, only)
        want = ref + res if with_res else ref
        if only is not None:                                                # one phase: its pixels, and nothing else written
            L = D.launches(case)[only[0]]
            mask = np.zeros((case.h, case.w), bool)
            mask[L.ooy::L.osy, L.oox::L.osx] = True
            assert np.isnan(got[:, ~mask]).all()
            got, want = got[:, mask], want[:, mask]
        elif case.stride == 2 and case.k == 1:                              # odd pixels: exactly 0, or the residual bit for bit
            odd = np.ones((case.h, case.w), bool)
            odd[0::2, 0::2] = False
            assert np.array_equal(got[:, odd], res[:, odd].astype(np.float64) if with_res else np.zeros_like(got[:, odd]))
        assert not np.isnan(got).any()
        if regime == "integer":
            assert np.array_equal(got, want), (with_res, only)
        else:
            s = D.abs_sum(case, dz, w, res if with_res else None)
            if only is not None:
                s = s[:, mask]
            assert (np.abs(got - want) <= 4 * (case.k * case.k * case.cout + 2) * 2.0 ** -53 * s).all(), (with_res, only)


@pytest.mark.parametrize("case", SMALL + [c for c in D.CASES if c.route == D.STREAMK and c.k == 1], ids=lambda c: D.case_id(c))
def test_impulse_expectation_is_autograd_of_the_impulse(case):
    w = D.impulse_weights(case)
    sites = D.impulse_sites(case)
    ho, wo = D.out_size(case)
    assert len(set(sites)) == len(sites) and {s[0] for s in sites} == {0, case.n - 1} and {s[1] for s in sites} == {0, case.cout - 1}
    pix = {(oy, ox) for _, _, oy, ox in sites}
    assert {(0, 0), (0, wo - 1), (ho - 1, 0), (ho - 1, wo - 1), (0, wo // 2), (ho - 1, wo // 2), (ho // 2, 0), (ho // 2, wo - 1), (ho // 2, wo // 2)} == pix
    if case.route in (D.STREAMK, D.WINO_PERSIST):                                       # the large cases: four of the sites
        sites = sites[:2] + sites[-2:]
    for site in sites:
        dz = D.impulse_dz(case, site)
        assert dz.sum() == 1.0 and np.count_nonzero(dz) == 1
        want = D.impulse_expectation(case, site, w)
        assert np.array_equal(D.reference(case, dz, w), want), site                     # one non-zero term: exact
        assert np.array_equal(D.dgrad_model(case, dz, w), want), site
        assert len(D.impulse_footprint(case, *site[2:])) == np.count_nonzero(want.any(axis=-1))
    if case.pad > 0:                                                                    # some tap of some impulse leaves the image
        assert any(len(D.impulse_footprint(case, oy, ox)) < case.k * case.k for _, _, oy, ox in sites)


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_integer_regime_cannot_round(case):
    assert D.exact_headroom(case) < 2 ** 24
    dz, w, res = D.inputs(case, "integer")
    for a in (dz, w, res):
        assert np.array_equal(a, np.rint(a)) and a.min() == -2 and a.max() == 2
    if case.route != D.STREAMK:
        ref = D.reference(case, dz, w) + res
        assert np.array_equal(ref, ref.astype(np.float32)) and np.abs(ref).max() <= D.exact_headroom(case)


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_claims_of_the_comments_follow_from_the_dispatch_rules(case):
    q, claim = D.plan(case), D.CLAIMS[case]
    assert claim and {k: q[k] for k in claim} == claim
    assert case.route in q["routes"] and (sum(q["routes"].values()) == len(D.launches(case)) or not q["direct"])
    if case.route == D.WINO_PERSIST:
        assert q["routes"] == {D.WINO_PERSIST: 1, D.WINO: 1} and 0 < q["persist_images"] < case.n      # and the remainder on the plain kernel
        assert D.plan(case._replace(n=q["persist_images"] - 1))["persist_images"] == 0                  # the smallest batch the gate admits
    elif case.route != D.STREAMK:
        assert q["routes"] == {case.route: len(D.launches(case)) if q["direct"] else 1}
    if not case.knobs:
        return
    default = D.plan(case._replace(knobs=()))                                           # the knob is what takes the case there
    assert default.get("tile") != q.get("tile") or default["routes"] != q["routes"]


def test_the_listed_branches_are_all_present():
    direct = [(c, D.plan(c)) for c in D.CASES if not D.is_winograd(c)]
    assert {q["tile"] for _, q in direct} == {(128, 32), (64, 64), (64, 128), (128, 64), (128, 128)}
    assert {v for _, q in direct if q["var"] for v in q["var"]} == {0, 4}
    for tile in ((64, 64), (64, 128)):                                                  # full and ragged output channels
        widths = {c.cin % tile[1] == 0 for c, q in direct if q["tile"] == tile}
        assert widths == {True, False}, tile
    assert {48, 96, 192} <= {c.cin for c, _ in direct}
    for tile in ((128, 64), (128, 128)):                                                # M below one tile, and no multiple of 64
        ms = {m for c, q in direct if q["tile"] == tile and q["routes"] == {D.IGEMM: len(q["launches"])} for m, _, _ in q["launches"]}
        assert any(m < 64 for m in ms) and any(m > 128 and m % 64 for m in ms), (tile, ms)
    forms = {(c.k, c.stride) for c, _ in direct}
    assert {(1, 1), (3, 1), (1, 2), (3, 2)} <= forms
    assert {D.out_size(c) for c, _ in direct if (c.k, c.stride) == (3, 2)} >= {(1, 1), (3, 2), (8, 6)}
    assert {(c.cout, c.coutk) for c, _ in direct if c.coutk != c.cout} == {(17, 32), (27, 32)}
    sk = [q for c, q in direct if c.route == D.STREAMK]
    assert [q["routes"] for q in sk] == [{D.STREAMK: 1}, {D.IGEMM: 3, D.STREAMK: 1}]
    assert [q["launches"][-1][2] for q in sk] == [D.STREAMK, D.STREAMK]                 # the scattered one is the four-tap (odd, odd) phase
    for c, q in direct:                                                                 # smallest shapes the stream-K gate admits
        if c.route == D.STREAMK:
            m, kt, _ = q["launches"][-1]
            assert -(-m // 64) * (D.cout_pad(c.cin) // 128) * kt == 6 * 768
    wino = [c for c in D.CASES if D.is_winograd(c)]
    assert {D.plan(c)["halves"] for c in wino} == {1, 2}
    assert any(c.h % 2 and c.w % 2 for c in wino) and any(c.h % 2 == 0 and c.w % 2 == 0 for c in wino)


def test_elementwise_bound_is_the_stated_formula():
    case = D.CASES[1]
    n = 9 * 64 + 1
    assert D.elementwise_bound(case, 2.0) == 2.0 * (n * 2.0 ** -24 / (1 - n * 2.0 ** -24)) * 2.0


def test_pack_layout_pads_with_zeros():
    w = np.arange(1, 1 + 17 * 40 * 9, dtype=np.float32).reshape(17, 40, 3, 3)
    p = D.expect_dgrad_pack(w, [(2, 0), (0, 1)], 32)
    assert p.shape == (64, 2, 32) and not p[40:].any() and not p[:, :, 17:].any() and (p[:40, :, :17] != 0).all()
    assert p[3, 0, 5] == w[5, 3, 2, 0] and p[39, 1, 16] == w[16, 39, 0, 1]
    assert [D.cout_pad(c) for c in (1, 32, 33, 64, 65, 128, 129, 192)] == [32, 32, 64, 64, 128, 128, 256, 256]


def test_the_restated_launch_logic_is_the_trainers():
    """The parts of hip_train.py this module restates, compared as source: the parity -> taps lists of _igemm_dgrad — the one place that
    assembles an implicit-GEMM data gradient, for every layer class — and _flipped_taps.  A change there must be made here as well, where
    autograd judges it.  And the BatchNorm backward's three-way choice and its fusion gate are each written in one function."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vatl4pose-wacv2024_amd", "alphapose", "models", "hip_train.py")
    tree = ast.parse(open(path).read())

    def phase_lists(root):
        found = {"rows": [], "cols": []}
        for node in ast.walk(root):
            if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name) and node.targets[0].id in found and isinstance(node.value, ast.IfExp):
                found[node.targets[0].id].append((ast.literal_eval(node.value.body), ast.literal_eval(node.value.orelse)))
        return found
    want = (D.PHASE_TAPS[0], D.PHASE_TAPS[1])
    dgrad = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "_igemm_dgrad")
    assert phase_lists(tree) == phase_lists(dgrad) == {"rows": [want], "cols": [want]}

    readers = {}                                                             # name -> [function that reads it (outermost def, Class.method for methods)]

    def visit(node, where):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, ast.ClassDef) and where is None:
                visit(child, child.name + ".")
            elif isinstance(child, ast.FunctionDef) and (where is None or where.endswith(".")):
                visit(child, (where or "") + child.name)
            else:
                name = child.attr if isinstance(child, ast.Attribute) else child.id if isinstance(child, ast.Name) else None
                if name is not None and isinstance(child.ctx, ast.Load):
                    readers.setdefault(name, []).append(where)
                visit(child, where)
    visit(tree, None)
    for name in ("pack_dgrad_weight", "conv2d_fwd_ex"):                      # the data-gradient launches: _igemm_dgrad alone
        assert set(readers[name]) == {"_igemm_dgrad"}, (name, readers[name])
    # ... and the transposed conv's 4x4 / stride-2 conv on the forward packing, a geometry of its own
    assert sorted(readers["conv2d_fwd_ex_bnbwd"]) == ["_DeconvBN.backward", "_igemm_dgrad"], readers["conv2d_fwd_ex_bnbwd"]
    for name in ("bn_bwd_from_stats", "bn_train_bwd_relu", "bn_train_bwd", "_FUSE_BN_MIN_C", "_FUSE_BN_BWD"):
        assert len(set(readers[name])) == 1 and None not in readers[name], (name, readers[name])
    assert set(readers["bn_bwd_from_stats"] + readers["bn_train_bwd_relu"] + readers["bn_train_bwd"]) == {"_bn_backward"}
    assert set(readers["_FUSE_BN_MIN_C"] + readers["_FUSE_BN_BWD"]) == {"_bn_spec"}

    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "_flipped_taps")
    ns = {}
    exec(compile(ast.Module([fn], []), path, "exec"), ns)
    for r, s in ((1, 1), (3, 3), (2, 3), (7, 7)):
        assert ns["_flipped_taps"](r, s) == D.flipped_taps(r, s)
