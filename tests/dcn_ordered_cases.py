"""The ordered (bit-reproducible) dx of the deformable convolution: a numpy float32 model of it, operation for operation, and the
cases of tests/test_dcn_ordered_cpu.py and tests/test_gpu_dcn_ordered.py that go beyond those of tests/dcn_cases.py.

The model states the arithmetic of csrc/deform_sample.h in ``np.float32`` (numpy rounds every operation once and fuses nothing):

    py = float32(y*s - 1 + i) + dy                      one add (px likewise)
    valid = py > -1 and px > -1 and py < H and px < W   (NaN and infinities fail)
    fy = floor(py); ly = py - fy; hy = 1 - ly           (lx, hx likewise)
    w[k] = wy[a] * wx[b], k = 2a + b, wy = (hy, ly), wx = (hx, lx), corner (fy + a, fx + b); a corner outside the image has w = 0
    wk = w[k] * m                                       one multiply; m = 1 for DCN v1, the modulation itself for v2

and the ordered sum of include/vatl_hip.h: the contributions to dx[n, y, x, c] are the (p, t, k) of image n whose corner k is (y, x)
with wk != 0; in ascending key = (p_local*9 + t)*4 + k:  acc = acc + (dcol[p, t, c] * wk), from +0.0, product and sum rounded once
each.  Mask logits (DCN v2 as the trainer calls it) go through the kernels' ``expf`` and are not modelled.
"""
import numpy as np
import torch

from tests import dcn_cases as D


def direct_mask(c):
    """The modulation itself (float64 tensor of float32 values) of a case: its ``mask``, else the sigmoid of its logits rounded to
    float32, else None (DCN v1)."""
    if c.get("mask") is not None:
        return c["mask"]
    return None if c["mask_logits"] is None else torch.sigmoid(c["mask_logits"]).float().double()


def entries(offset, mask, h, w, stride, dg):
    """Every contribution of the index, unsorted -> dict of flat arrays: image ``n``, list ``lst`` = (y*W + x)*dg + g inside the image,
    ``key``, ``wk`` (float32).  offset (B,18dg,Ho,Wo), mask (B,9dg,Ho,Wo) or None: arrays of float32 values."""
    f32 = np.float32
    off = np.asarray(offset, dtype=f32)
    b, _, ho, wo = off.shape
    o = off.reshape(b, dg, 9, 2, ho, wo)
    t = np.arange(9)
    base_y = (np.arange(ho)[None, :, None] * stride - 1 + (t // 3)[:, None, None]).astype(f32)       # (9, Ho, 1)
    base_x = (np.arange(wo)[None, None, :] * stride - 1 + (t % 3)[:, None, None]).astype(f32)        # (9, 1, Wo)
    with np.errstate(invalid="ignore"):
        py = base_y[None, None] + o[:, :, :, 0]                                                       # (B, dg, 9, Ho, Wo), one float32 add
        px = base_x[None, None] + o[:, :, :, 1]
        valid = (py > f32(-1)) & (px > f32(-1)) & (py < f32(h)) & (px < f32(w))
    py, px = np.where(valid, py, f32(0)), np.where(valid, px, f32(0))
    fy, fx = np.floor(py), np.floor(px)
    ly, lx = py - fy, px - fx
    hy, hx = f32(1) - ly, f32(1) - lx
    assert ly.dtype == f32 and hy.dtype == f32
    m = np.ones_like(py) if mask is None else np.asarray(mask, dtype=f32).reshape(b, dg, 9, ho, wo)
    n_i, g_i, t_i, y_i, x_i = np.meshgrid(np.arange(b), np.arange(dg), t, np.arange(ho), np.arange(wo), indexing="ij")
    out = {"n": [], "lst": [], "key": [], "wk": []}
    for a in (0, 1):
        for bb in (0, 1):
            k = 2 * a + bb
            ys, xs = fy.astype(np.int64) + a, fx.astype(np.int64) + bb
            inside = valid & (ys >= 0) & (ys <= h - 1) & (xs >= 0) & (xs <= w - 1)
            wgt = np.where(inside, (ly if a else hy) * (lx if bb else hx), f32(0))
            wk = wgt * m
            assert wk.dtype == f32
            with np.errstate(invalid="ignore"):
                counts = valid & (wk != 0)                             # the test of the kernels: a NaN modulation counts
            # a corner outside the image that still counts (w = 0 times a NaN or infinite modulation) sits at index 0, as in deform_sample.h
            pix = np.where(inside, ys * w + xs, 0)
            out["n"].append(n_i[counts]); out["lst"].append(pix[counts] * dg + g_i[counts])
            out["key"].append(((y_i * wo + x_i) * 9 + t_i)[counts] * 4 + k); out["wk"].append(wk[counts])
    return {k: np.concatenate(v) for k, v in out.items()}


def ordered_dx(dcol, offset, mask, h, w, stride, dg, shuffle_seed=None):
    """The model: dcol (B,Ho,Wo,9,C) float32 -> dx (B,H,W,C) float32, NHWC as the kernels hold it.  ``shuffle_seed``: the entries are
    shuffled before they are sorted (the arrival order of the kernels' cursors is not fixed; the result must not depend on it)."""
    f32 = np.float32
    dcol = np.asarray(dcol, dtype=f32)
    b, ho, wo, _, c = dcol.shape
    cg = c // dg
    e = entries(offset, mask, h, w, stride, dg)
    order = np.arange(e["key"].size)
    if shuffle_seed is not None:
        order = np.random.default_rng(shuffle_seed).permutation(order)
    glob = (e["n"] * (h * w * dg) + e["lst"])[order]                   # the list across the batch
    key, wk = e["key"][order], e["wk"][order]
    srt = np.lexsort((key, glob))                                      # by list, then ascending key
    glob, key, wk = glob[srt], key[srt], wk[srt]
    assert np.all((np.diff(glob) > 0) | (np.diff(key) > 0)), "keys inside a list are unique"
    first = np.searchsorted(glob, glob, side="left")
    rank = np.arange(glob.size) - first                                # position inside the own list
    rows = dcol.reshape(b, ho * wo, 9, dg, cg)
    acc = np.zeros((b * h * w * dg, cg), dtype=f32)                    # +0.0: an empty list keeps it
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.searchsorted(rank[by_rank], np.arange(rank.max() + 2 if rank.size else 1))
    for r in range(len(bounds) - 1):                                   # step r adds the r-th entry of every list that has one
        sel = by_rank[bounds[r]:bounds[r + 1]]
        li = glob[sel]
        img, g = li // (h * w * dg), li % dg
        term = rows[img, key[sel] // 36, (key[sel] // 4) % 9, g] * wk[sel, None]        # rounded once
        acc[li] = acc[li] + term                                                        # rounded once; each list at most once per step
    return acc.reshape(b, h, w, dg * cg)


def list_lengths(c):
    """Entries per (image, input pixel, group) of a case with its direct mask: (B, H*W*dg)."""
    b, _, h, w = c["x"].shape
    m = direct_mask(c)
    e = entries(c["offset"].numpy(), None if m is None else m.numpy(), h, w, c["stride"], c["dg"])
    return np.bincount(e["n"] * (h * w * c["dg"]) + e["lst"], minlength=b * h * w * c["dg"]).reshape(b, -1)


def _aim(c, image, py, px):
    """Every tap of every output pixel of ``image`` to the exact position (py, px)."""
    _, _, h, w = c["x"].shape
    ho, wo = D.out_hw(h, w, c["stride"])
    for g in range(c["dg"]):
        for t in range(9):
            for y in range(ho):
                for x in range(wo):
                    D._set_pos(c["offset"], h, w, c["stride"], image, g, t, y, x, py, px)
    c["offset"] = D._f32(c["offset"])
    return c


def _pileup_frac():
    return _aim(D.make_case("pileup_frac", 2, 7, 5, 16, 16, 1, 1, False, 401), 0, 3.25, 2.5)


def _pileup_int():
    return _aim(D.make_case("pileup_int", 2, 7, 5, 16, 16, 1, 1, False, 402), 0, 3.0, 2.0)


def _pileup_long():
    return _aim(D.make_case("pileup_long", 1, 24, 18, 16, 16, 1, 1, False, 403), 0, 10.25, 7.5)


def _empty():
    c = D.make_case("empty", 2, 7, 5, 16, 16, 1, 1, False, 404)
    bad = torch.tensor([1e4, -1e4, float("nan"), float("inf"), -float("inf")], dtype=torch.float64)
    n = c["offset"].numel()
    c["offset"] = bad[torch.arange(n) % 5].reshape(c["offset"].shape)          # every coordinate of every tap is one of them
    return c


def _dg4_s2():
    c = D.make_case("dg4_s2", 3, 10, 8, 32, 32, 2, 4, True, 405)
    c["mask"] = D._f32(torch.rand(c["mask_logits"].shape, generator=torch.Generator().manual_seed(406)) * 1.5)      # given directly
    c["mask_logits"] = None
    return c


NEW_CASES = {"pileup_frac": _pileup_frac, "pileup_int": _pileup_int, "pileup_long": _pileup_long, "empty": _empty, "dg4_s2": _dg4_s2}
_cache = {}


def new_case(name):
    """The (cached, never modified) new case ``name``: the keys of dcn_cases.make_case plus ``mask`` (the modulation given directly)."""
    if name not in _cache:
        _cache[name] = NEW_CASES[name]()
    return _cache[name]


def grad_columns(c, seed=6):
    """A seeded gradient of the column matrix in the oracle's layout (B, C, 9, Ho, Wo), float64 tensor of float32 values."""
    b, ch, h, w = c["x"].shape
    ho, wo = D.out_hw(h, w, c["stride"])
    return D._f32(torch.randn((b, ch, 9, ho, wo), generator=torch.Generator().manual_seed(seed)))


def dcol_rows(g):
    """(B, C, 9, Ho, Wo) -> the kernels' rows (B, Ho, Wo, 9, C), float32 numpy."""
    return np.ascontiguousarray(g.permute(0, 3, 4, 2, 1).float().numpy())


_model_cache = {}


def model_dx(tag, c, g):
    """ordered_dx of case ``c`` under the column gradient ``g``, computed once per ``tag``."""
    if tag not in _model_cache:
        b, _, h, w = c["x"].shape
        m = direct_mask(c)
        _model_cache[tag] = ordered_dx(dcol_rows(g), c["offset"].numpy(), None if m is None else m.numpy(), h, w, c["stride"], c["dg"])
    return _model_cache[tag]


def oracle_dx(c, g):
    """dx (B, C, H, W) float64: autograd of dcn_cases.deform_columns_ref under the column gradient ``g``."""
    x = c["x"].clone().requires_grad_()
    ref = D.deform_columns_ref(x, c["offset"], direct_mask(c), c["stride"], c["dg"])
    return torch.autograd.grad(ref, [x], g)[0]
