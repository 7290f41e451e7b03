"""tests/wgrad_cases.py before anything trusts it (no GPU): the impulse expectation is the float64 reference of the impulse inputs bit
for bit, the pixel lists are inside the batch and complete, the claims of the case comments follow from the restated shape rules."""
import numpy as np
import pytest

from tests import wgrad_cases as W

IDS = [W.case_id(c) for c in W.CASES]


def test_case_names_are_unique_and_every_entry_is_covered():
    assert len(set(IDS)) == len(IDS)
    assert len(set(W.CASES)) == len(W.CASES) and set(W.CLAIMS) == set(W.CASES)
    assert {c[0] for c in W.CASES} == {W.DIRECT, W.DECONV, W.WINO, W.WINO_DECONV}
    assert len({W.seed(c) for c in W.CASES}) == len(W.CASES)


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_impulse_expectation_is_the_reference_of_the_impulse_inputs(case):
    g = W.geometry(case)
    plain, gathered, expected = W.impulse(case)
    assert plain.dtype == np.float32 and gathered.dtype == np.float32 and expected.shape == g["dw"]
    valid = plain[..., :g["Cn"]].reshape(g["M"], g["Cn"])
    assert ((valid == 0) | (valid == 1)).all() and (valid.sum(axis=0) == 1).all()              # one-hot per channel, channel Cn-1 included
    assert [int(valid[:, ch].argmax()) for ch in (0, g["Cn"] - 1)] == [W.impulse_pixel(case, 0), W.impulse_pixel(case, g["Cn"] - 1)]
    if g["Gs"] > g["Cn"]:
        assert (plain[..., g["Cn"]:] != 0).all()                                                # padding channels carry values to leave out
    ref = W.reference(case, (plain, gathered))
    assert ref.dtype == np.float64 and np.array_equal(ref, expected)                            # one non-zero term: exact
    inside = expected != 0
    assert inside.any() and (expected[inside] == expected[inside].astype(np.float32)).all()
    if g["pad"] > 0:
        assert not inside.all()                                                                 # some tap of some impulse leaves the image


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_pixel_list_is_inside_the_batch_and_complete(case):
    g, q = W.geometry(case), W.plan(case)
    n, ho, wo, m_all = g["N"], g["Ho"], g["Wo"], g["M"]
    px = W.pixels(case)
    kinds = dict(px)
    assert len(kinds) == len(px)                                                                # no kind listed twice
    assert all(isinstance(m, int) and 0 <= m < m_all for _, m in px)
    assert kinds["row0"] == 0 and kinds["last_row"] == m_all - 1
    for m in (31, 32):
        assert (f"row{m}" in kinds) == (m < m_all) and kinds.get(f"row{m}", m) == m
    assert ("split_end" in kinds) == ("split_start" in kinds) == (q["splits"] > 1)
    if q["splits"] > 1 and not W.is_winograd(case):
        assert kinds["split_end"] + 1 == kinds["split_start"] == q["kps"] * 32 < m_all
    if q["splits"] > 1 and W.is_winograd(case):                                                 # tile index of a pixel: (b, oy // mo, ox // mo)
        tile = lambda m: (m // (ho * wo)) * q["th"] * q["tw"] + (m // wo % ho) // q["mo"] * q["tw"] + (m % wo) // q["mo"]
        assert tile(kinds["split_end"]) == q["tps"] - 1 and tile(kinds["split_start"]) == q["tps"]
    for b in {0, n - 1}:
        corners = {m for k, m in px if k.startswith(f"corner_b{b}_")}
        assert corners == {(b * ho + oy) * wo + ox for oy in (0, ho - 1) for ox in (0, wo - 1)}
    assert kinds["last_column"] % wo == wo - 1 and kinds["last_line"] // wo % ho == ho - 1
    first_tile_images = min(n, -(-32 // (ho * wo)))
    assert [k for k in kinds if k.startswith("image")] == ([f"image{b}" for b in range(first_tile_images)] if ho * wo < 32 else [])
    assert all(kinds[f"image{b}"] // (ho * wo) == b for b in range(first_tile_images) if ho * wo < 32)
    distinct = {m for _, m in px}
    used = {W.impulse_pixel(case, ch) for ch in range(g["Cn"])}
    assert used <= distinct and (used == distinct or g["Cn"] < len(distinct))                   # every pixel is dealt while channels last
    assert W.impulse_pixel(case, g["Cn"] - 1) in distinct


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_claims_of_the_comments_follow_from_the_shape_rules(case):
    q, claim = W.plan(case), W.CLAIMS[case]
    assert {k: q[k] for k in claim} == claim


def test_the_listed_branches_are_all_present():
    direct = [W.direct_plan(c) for c in W.CASES if c[0] == W.DIRECT]
    assert {q["tile"] for q in direct} == {(128, 128), (128, 64), (64, 128), (64, 64), (32, 128), (64, 32)}
    assert {q["tpt"] for q in direct} == {1, 2, 4}
    assert {1, 3, 9, 48} <= {q["slices"] for q in direct}
    assert any(W.geometry(c)["M"] < 32 for c in W.CASES) and any(W.geometry(c)["Ho"] * W.geometry(c)["Wo"] == 1 for c in W.CASES)
    wino = [W.winograd_plan(c) for c in W.CASES if c[0] == W.WINO]
    assert {q["halves"] for q in wino} == {1, 2} and {q["table"] for q in wino} == {True, False}
    assert any(q["mtiles"] < 8 for q in wino) and any(q["mtiles"] % q["tps"] == 1 for q in wino)
    assert len(W.TWO_HALF_CASES) == 4


def test_elementwise_bound_is_the_stated_formula():
    case = W.CASES[0]
    m = W.geometry(case)["M"]
    n = m + 3 + 17
    assert W.elementwise_bound(case, 3, 2.0) == 2.0 * (n * 2.0 ** -24 / (1 - n * 2.0 ** -24)) * 2.0
