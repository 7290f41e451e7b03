"""The ordered dx of the deformable convolution without a GPU: the numpy float32 model of tests/dcn_ordered_cases.py — what
tests/test_gpu_dcn_ordered.py holds the kernel's bits to — against the float64 oracle, its independence of the order in which the
entries arrive, the list lengths the crafted cases promise, and how the process switch resolves."""
import numpy as np
import pytest
import torch

from tests import dcn_cases as D
from tests import dcn_ordered_cases as O

BAR = 2e-5          # normwise, the bar of tests/test_gpu_dcn.py


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def _smooth(spec):
    return D.smooth_offsets(D.make_case(*spec), 900 + D.ALL_CASES.index(spec))


def _model_vs_oracle(tag, c):
    g = O.grad_columns(c)
    got = O.model_dx(tag, c, g)
    want = O.oracle_dx(c, g).permute(0, 2, 3, 1).numpy()
    e = _rel(got, want)
    print(f"{tag}: model vs float64 {e:.3e}")
    assert got.dtype == np.float32 and got.shape == want.shape
    assert e <= BAR, (tag, e)
    return got


@pytest.mark.parametrize("spec", D.ALL_CASES, ids=[c[0] for c in D.ALL_CASES])
def test_model_vs_oracle_smooth_offsets(spec):
    _model_vs_oracle("smooth/" + spec[0], _smooth(spec))


@pytest.mark.parametrize("name", list(O.NEW_CASES))
def test_model_vs_oracle_new_cases(name):
    got = _model_vs_oracle(name, O.new_case(name))
    if name == "empty":
        assert not got.any() and not np.signbit(got).any()              # +0.0 everywhere


def test_crafted_cases_have_the_lists_they_promise():
    n = O.list_lengths(O.new_case("pileup_frac"))
    assert sorted(np.flatnonzero(n[0]).tolist()) == [3 * 5 + 2, 3 * 5 + 3, 4 * 5 + 2, 4 * 5 + 3] and set(n[0][n[0] > 0]) == {315}
    assert n[1].max() < 100 and np.count_nonzero(n[1]) > 20             # image 1 is random
    n = O.list_lengths(O.new_case("pileup_int"))
    assert np.flatnonzero(n[0]).tolist() == [3 * 5 + 2] and n[0][17] == 315          # the three corners of weight 0 are absent
    c = O.new_case("pileup_int")
    e = O.entries(c["offset"].numpy(), None, 7, 5, 1, 1)
    assert np.all(e["wk"][e["n"] == 0] == 1) and np.all(e["key"][e["n"] == 0] % 4 == 0)
    n = O.list_lengths(O.new_case("pileup_long"))
    assert np.count_nonzero(n[0]) == 4 and set(n[0][n[0] > 0]) == {3888}
    assert not O.list_lengths(O.new_case("empty")).any()
    n = O.list_lengths(O.new_case("dg4_s2"))
    assert n.shape == (3, 10 * 8 * 4) and n.max() > 1


@pytest.mark.parametrize("name", ["pileup_frac", "dg4_s2", "border_s1_dg2_v2"])
def test_order_of_arrival_does_not_matter(name):
    if name in O.NEW_CASES:
        c = O.new_case(name)
    else:
        c = D.case(next(s for s in D.ALL_CASES if s[0] == name))
    g = O.grad_columns(c)
    want = O.model_dx(name if name in O.NEW_CASES else "drawn/" + name, c, g)
    m = O.direct_mask(c)
    h, w = c["x"].shape[2:]
    for seed in (1, 2):
        got = O.ordered_dx(O.dcol_rows(g), c["offset"].numpy(), None if m is None else m.numpy(), h, w, c["stride"], c["dg"], shuffle_seed=seed)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # ... while the order of the SUM does: descending keys give other bits on a list of 315
    if name == "pileup_frac":
        rows, e = O.dcol_rows(g), O.entries(c["offset"].numpy(), None, h, w, 1, 1)
        sel = np.flatnonzero((e["n"] == 0) & (e["lst"] == 17))
        sel = sel[np.argsort(e["key"][sel])]
        terms = rows[0].reshape(35, 9, 16)[e["key"][sel] // 36, (e["key"][sel] // 4) % 9] * e["wk"][sel, None]
        up, down = np.zeros(16, np.float32), np.zeros(16, np.float32)
        for r in range(len(sel)):
            up, down = up + terms[r], down + terms[len(sel) - 1 - r]
        assert np.array_equal(up.view(np.uint32), want[0, 3, 2].view(np.uint32)) and not np.array_equal(up, down)


@pytest.fixture
def clean_switch():
    from alphapose.models.layers import dcn
    before = (dcn.vh.deform_deterministic_mode(), torch.are_deterministic_algorithms_enabled(), torch.backends.cudnn.deterministic)
    dcn.set_deterministic(None)
    torch.use_deterministic_algorithms(False)
    torch.backends.cudnn.deterministic = False
    yield dcn
    dcn.set_deterministic(before[0])
    torch.use_deterministic_algorithms(before[1])
    torch.backends.cudnn.deterministic = before[2]


def test_switch_resolution(clean_switch):
    dcn = clean_switch
    assert dcn.is_deterministic() is False                               # the default: off
    torch.use_deterministic_algorithms(True)
    assert dcn.is_deterministic() is True
    dcn.set_deterministic(False)                                         # an explicit False overrides torch
    assert dcn.is_deterministic() is False
    dcn.set_deterministic(None)
    torch.use_deterministic_algorithms(False)
    assert dcn.is_deterministic() is False
    torch.backends.cudnn.deterministic = True                            # what the driver's --seedfix sets
    assert dcn.is_deterministic() is True
    dcn.set_deterministic(False)
    assert dcn.is_deterministic() is False
    torch.backends.cudnn.deterministic = False
    dcn.set_deterministic(True)
    assert dcn.is_deterministic() is True
    with pytest.raises(ValueError):
        dcn.set_deterministic(1.5)
    assert dcn.is_deterministic() is True


def test_context_manager_restores_the_previous_state(clean_switch):
    dcn = clean_switch
    with dcn.deterministic():
        assert dcn.is_deterministic() is True
        with dcn.deterministic(False):
            assert dcn.is_deterministic() is False
        assert dcn.is_deterministic() is True
    assert dcn.vh.deform_deterministic_mode() is None and dcn.is_deterministic() is False
    dcn.set_deterministic(False)
    with pytest.raises(RuntimeError):
        with dcn.deterministic(True):
            raise RuntimeError("leaves the block")
    assert dcn.vh.deform_deterministic_mode() is False
    torch.backends.cudnn.deterministic = True
    with dcn.deterministic(None):                                        # None inside: follow torch
        assert dcn.is_deterministic() is True
    assert dcn.is_deterministic() is False
    assert {"set_deterministic", "is_deterministic", "deterministic"} <= set(dcn.__all__)
