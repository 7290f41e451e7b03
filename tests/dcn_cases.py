"""Deformable convolution (DCN v1 / v2): the float64 oracle and the seeded cases of tests/test_dcn_cpu.py and tests/test_gpu_dcn.py.

The oracle is the published definition, written with index gathers so that autograd gives all four gradients:

    dy = offset[b, 18g + 2t, y, x], dx = offset[b, 18g + 2t + 1, y, x], m = mask[b, 9g + t, y, x] (1 without a mask)
    py = y*s - 1 + i + dy, px = x*s - 1 + j + dx                                  (g = c // (C/dg), t = 3i + j)
    out[b,o,y,x] = sum_c sum_t w[o,c,i,j] * m * S(x[b,c], py, px)
    S = 0 unless py > -1, px > -1, py < H, px < W (NaN / inf fail); else the bilinear blend of the four corners around
    (floor py, floor px), a corner outside [0,H-1] x [0,W-1] contributing 0.

Every tensor of a case holds float32-representable values (drawn in float32, kept in float64), so the oracle and the fp32 kernels read
the same numbers and differ in arithmetic only.
"""
import torch


def out_hw(h, w, stride):
    return (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1


def positions(offset, h, w, stride, dg):
    """(py, px), each (B, dg, 9, Ho, Wo), in the dtype of ``offset``."""
    b, _, ho, wo = offset.shape
    o = offset.view(b, dg, 9, 2, ho, wo)
    i = torch.arange(9).div(3, rounding_mode="floor").view(1, 1, 9, 1, 1).to(offset.dtype)
    j = (torch.arange(9) % 3).view(1, 1, 9, 1, 1).to(offset.dtype)
    ys = (torch.arange(ho) * stride - 1).view(1, 1, 1, ho, 1).to(offset.dtype)
    xs = (torch.arange(wo) * stride - 1).view(1, 1, 1, 1, wo).to(offset.dtype)
    return ys + i + o[:, :, :, 0], xs + j + o[:, :, :, 1]


def deform_columns_ref(x, offset, mask, stride, dg):
    """The sampled, mask-weighted values (B, C, 9, Ho, Wo)."""
    b, c, h, w = x.shape
    ho, wo = out_hw(h, w, stride)
    cg = c // dg
    py, px = positions(offset, h, w, stride, dg)
    valid = (py > -1) & (px > -1) & (py < h) & (px < w)                   # False for NaN and infinities
    zero = torch.zeros((), dtype=x.dtype)
    py, px = torch.where(valid, py, zero), torch.where(valid, px, zero)    # validity is decided before anything is floored or indexed
    y0, x0 = torch.floor(py).detach(), torch.floor(px).detach()
    ly, lx = py - y0, px - x0
    xg = x.reshape(b, dg, cg, h * w)
    s = 0
    for a in (0, 1):
        for bb in (0, 1):
            yy, xx = y0 + a, x0 + bb
            inb = valid & (yy >= 0) & (yy <= h - 1) & (xx >= 0) & (xx <= w - 1)
            idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).long().view(b, dg, 1, 9 * ho * wo).expand(b, dg, cg, 9 * ho * wo)
            v = torch.gather(xg, 3, idx).view(b, dg, cg, 9, ho, wo)
            wgt = (ly if a else 1 - ly) * (lx if bb else 1 - lx)
            s = s + torch.where(inb, wgt, zero).unsqueeze(2) * v
    if mask is not None:
        s = s * mask.view(b, dg, 1, 9, ho, wo)
    return s.reshape(b, c, 9, ho, wo)


def deform_conv_ref(x, w, offset, mask, stride, dg):
    """out (B, Co, Ho, Wo) in the dtype of the inputs (float64 for the oracle proper, float32 for 'the oracle's own fp32 distance')."""
    col = deform_columns_ref(x, offset, mask, stride, dg)
    return torch.einsum("bcthw,oct->bohw", col, w.reshape(w.shape[0], w.shape[1], 9))


def _f32(t):
    return t.float().double()


def _set_pos(off, h, w, stride, b, g, t, y, x, py=None, px=None):
    """Move tap t of output pixel (b, y, x), group g, to the exact position (py, px); None leaves a coordinate alone."""
    if py is not None:
        off[b, 18 * g + 2 * t, y, x] = py - (y * stride - 1 + t // 3)
    if px is not None:
        off[b, 18 * g + 2 * t + 1, y, x] = px - (x * stride - 1 + t % 3)


def make_case(name, b, h, w, c, co, stride, dg, masked, seed, crafted=False):
    """-> dict of float64 CPU tensors: x (B,C,H,W), w (Co,C,3,3), offset (B,18dg,Ho,Wo) ~ N(0, 2^2) so that most taps of these small
    images cross a border, mask_logits (B,9dg,Ho,Wo) or None.  ``crafted`` plants the border rows: positions inside (-1,0) and (H-1,H),
    exactly -1, 0, H-1 and H, integer offsets and taps at +-1e4."""
    gen = torch.Generator().manual_seed(seed)
    ho, wo = out_hw(h, w, stride)
    x = _f32(torch.randn(b, c, h, w, generator=gen))
    wt = _f32(torch.randn(co, c, 3, 3, generator=gen) / (9 * c) ** 0.5)
    off = _f32(2.0 * torch.randn(b, 18 * dg, ho, wo, generator=gen))
    ml = _f32(torch.randn(b, 9 * dg, ho, wo, generator=gen)) if masked else None
    if crafted:
        rows = [(-0.5, None), (None, -0.5), (h - 0.5, None), (None, w - 0.5), (-0.25, w - 0.25), (-1.0, None), (None, -1.0), (0.0, 0.0),
                (h - 1.0, w - 1.0), (float(h), None), (None, float(w)), (h - 1.0, None), (None, 0.0), (-1.0, -1.0), (float(h), float(w))]
        k = 0
        for py, px in rows:
            for g in range(dg):
                y, xx = (k // wo) % ho, k % wo
                _set_pos(off, h, w, stride, k % b, g, k % 9, y, xx, py, px)
                k += 1
        for g in range(dg):                                   # integer offsets, and taps far outside
            off[0, 18 * g + 0, ho - 1, wo - 1], off[0, 18 * g + 1, ho - 1, wo - 1] = 2.0, -1.0
            off[b - 1, 18 * g + 8, 0, 0], off[b - 1, 18 * g + 9, 0, 0] = -1.0, 1.0
            off[0, 18 * g + 4, 0, wo - 1] = 1e4
            off[b - 1, 18 * g + 7, ho - 1, 0] = -1e4
    return {"name": name, "x": x, "w": wt, "offset": off, "mask_logits": ml, "stride": stride, "dg": dg}


def smooth_offsets(case, seed):
    """The case with its offsets redrawn so that BOTH fractional parts of every sampling position lie in [0.15, 0.85] (the offset
    gradient is discontinuous at cell edges, where an fp32 position may land on the other side): integer shift in -3 .. 3 plus a
    fraction, by construction — nothing is filtered."""
    gen = torch.Generator().manual_seed(seed)
    shape = case["offset"].shape
    off = torch.randint(-3, 4, shape, generator=gen).double() + (0.15 + 0.7 * torch.rand(shape, generator=gen).double())
    out = dict(case)
    out["offset"] = _f32(off)
    return out


def fractional_parts_ok(case, lo=0.1, hi=0.9):
    h, w = case["x"].shape[2:]
    py, px = positions(case["offset"], h, w, case["stride"], case["dg"])
    fy, fx = py - torch.floor(py), px - torch.floor(px)
    return bool(((fy >= lo) & (fy <= hi) & (fx >= lo) & (fx <= hi)).all())


# (name, B, H, W, C, Co, stride, dg, masked, seed, crafted)
BORDER_CASES = [(f"border_s{s}_dg{dg}_{'v2' if m else 'v1'}", 2, 7, 5, 16, 16, s, dg, m, 100 + 10 * s + 2 * dg + int(m), True)
                for s in (1, 2) for dg in (1, 2) for m in (False, True)]
TILE_CASES = [("tile_162px", 3, 9, 6, 32, 48, 1, 1, True, 201, False), ("tile_1x1", 1, 1, 1, 16, 16, 1, 1, True, 202, False),
              ("tile_dg4", 1, 5, 4, 16, 32, 1, 4, True, 203, False)]
PRODUCT_CASES = [("layer2_0", 2, 16, 12, 128, 128, 2, 1, True, 301, False), ("layer3", 2, 8, 6, 256, 256, 1, 1, False, 302, False),
                 ("layer4_k4608", 2, 4, 3, 512, 512, 1, 2, True, 303, False)]
ALL_CASES = BORDER_CASES + TILE_CASES + PRODUCT_CASES

_cache = {}


def case(spec):
    """The (cached, never modified) case of a spec tuple with its float64 oracle output ``ref`` and the oracle's own fp32 distance."""
    if spec[0] not in _cache:
        c = make_case(*spec)
        m = None if c["mask_logits"] is None else torch.sigmoid(c["mask_logits"])
        c["ref"] = deform_conv_ref(c["x"], c["w"], c["offset"], m, c["stride"], c["dg"])
        f = lambda t: None if t is None else t.float()
        r32 = deform_conv_ref(f(c["x"]), f(c["w"]), f(c["offset"]), None if m is None else torch.sigmoid(f(c["mask_logits"])), c["stride"], c["dg"])
        c["fp32_oracle_err"] = float((r32.double() - c["ref"]).abs().max() / c["ref"].abs().max())
        _cache[spec[0]] = c
    return _cache[spec[0]]
