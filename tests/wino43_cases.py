"""Inputs and case list of the Winograd-inference bit fixture (tests/golden/wino43_bits.npz): what tools/make_scorer_bits.py records from the
parent commit's library (``--cases tests.wino43_cases``) and tests/test_gpu_scorer_bits.py replays.  Same protocol as tests/scorer_cases.py:
inputs are regenerated from the seeds, never stored; nothing here imports the library.  The kernels are the two F(4x3,2x2) kernels
(csrc/winograd_deconv43.hip, winograd_s2_43.hip) with their filter packs, which share csrc/winograd43.h, winograd_stage.h and tile_order.h, and
the host side of csrc/conv_winograd.hip, which takes its tile order and stage from the same headers.

Shapes (N, H, W, Cin, Cout) are the smallest that reach each branch:
  transposed conv   (1,4,3,16,64) one tile, one stage; (5,8,6,32,64) images straddle a block; (9,8,6,48,128) tail group, two filter tiles,
                    odd stage count; (2,16,12,64,192) an odd number of filter tiles, so the last group of the tile order is short
  stride-2 conv     (1,8,6,16,64); (5,16,12,32,64); (9,16,12,48,128); (2,32,24,64,192) interior tiles
                    each with scale / bias / ReLU, and each once more with none of them
  packed filters    (Cin, Cout) = (16,64) and (48,192) for both kernels
  conv_winograd     one F(2x2,3x3) and one F(3x3,2x2) layer per route counter it can take, at 8x6 with 32 / 64 input channels: plain blocks,
                    two-half blocks (vatl_tune_set(21, 3)) and, for F(2x2,3x3), the persistent walk with a plain launch for the remainder
                    (4101 images: 512 periods of 8 and 5 left over).  These store the launch counts of the three routes next to the output.
Outputs of more than 65536 words are stored as their SHA-256.
"""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino43_bits.npz")
DIGEST_ABOVE = 65536
DECONV_SHAPES = ((1, 4, 3, 16, 64), (5, 8, 6, 32, 64), (9, 8, 6, 48, 128), (2, 16, 12, 64, 192))
S2_SHAPES = ((1, 8, 6, 16, 64), (5, 16, 12, 32, 64), (9, 16, 12, 48, 128), (2, 32, 24, 64, 192))
PACK_SHAPES = ((16, 64), (48, 192))
ROUTES = ("winograd", "winograd_2h", "winograd_persist")


def _rand(seed, *shape):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def _put(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _affine(cout, on):
    return (_put(np.abs(_rand(3, cout)) + 0.5), _put(_rand(4, cout))) if on else (None, None)


def _deconv43(vh, shape, affine):
    n, h, w, cin, cout = shape
    x, wt = _put(_rand(1, n, h, w, cin)), _put(_rand(2, cin, cout, 4, 4) * 0.05)
    sc, bi = _affine(cout, affine)
    assert vh.deconv4x4s2_winograd43_supported(n, h, w, cin, cout)
    return (vh.deconv4x4s2_winograd_fwd(x, None, sc, bi, cout, affine, u43=vh.pack_winograd_deconv43_weight(wt)),)


def _s2_43(vh, shape, affine):
    n, h, w, cin, cout = shape
    x, wt = _put(_rand(5, n, h, w, cin)), _put(_rand(6, cout, cin, 3, 3) * 0.05)
    sc, bi = _affine(cout, affine)
    assert vh.conv3x3s2_winograd43_supported(n, h, w, cin, cout)
    return (vh.conv2d_fwd(x, None, sc, bi, cout, 3, 3, 2, 1, affine, u_s2=vh.pack_winograd_s2_43_weight(wt)),)


def _pack_deconv43(vh, cin, cout):
    return (vh.pack_winograd_deconv43_weight(_put(_rand(7, cin, cout, 4, 4))),)


def _pack_s2_43(vh, cin, cout):
    return (vh.pack_winograd_s2_43_weight(_put(_rand(8, cout, cin, 3, 3))),)


def _with_routes(vh, halves, fn):
    """fn() under vatl_tune_set(21, halves) -> (output, launches of ROUTES as int64)."""
    import torch
    vh.tune_set(21, halves)
    try:
        with vh.flop_meter() as fm:
            y = fn()
    finally:
        vh.tune_set(21, 2)
    return y, torch.tensor([fm.routes[r] for r in ROUTES], dtype=torch.int64)


def _f23(vh, n, cin, cout, halves):
    x, wt = _put(_rand(9, n, 8, 6, cin)), _put(_rand(10, cout, cin, 3, 3) * 0.05)
    sc, bi = _affine(cout, True)
    r = _put(_rand(11, n, 8, 6, cout))
    u = vh.pack_winograd_weight(wt)
    return _with_routes(vh, halves, lambda: vh.conv3x3_winograd_fwd(x, u, sc, bi, cout, True, residual=r))


def _f32(vh, n, cin, cout, halves):
    x, wt = _put(_rand(12, n, 8, 6, cin)), _put(_rand(13, cin, cout, 4, 4) * 0.05)
    sc, bi = _affine(cout, True)
    u = vh.pack_winograd_deconv_weight(wt)
    return _with_routes(vh, halves, lambda: vh.deconv4x4s2_winograd_fwd(x, u, sc, bi, cout, True))


def _case(fn, *args):
    return lambda vh: fn(vh, *args)


def _tag(shape):
    return "x".join(str(v) for v in shape)


CASES = {}
for _s in DECONV_SHAPES:
    CASES[f"deconv43_{_tag(_s)}"] = _case(_deconv43, _s, True)
    CASES[f"deconv43_{_tag(_s)}_plain"] = _case(_deconv43, _s, False)
for _s in S2_SHAPES:
    CASES[f"s2_43_{_tag(_s)}"] = _case(_s2_43, _s, True)
    CASES[f"s2_43_{_tag(_s)}_plain"] = _case(_s2_43, _s, False)
for _ci, _co in PACK_SHAPES:
    CASES[f"pack_deconv43_{_ci}_{_co}"] = _case(_pack_deconv43, _ci, _co)
    CASES[f"pack_s2_43_{_ci}_{_co}"] = _case(_pack_s2_43, _ci, _co)
CASES["f23_winograd_2x8x6_32_32"] = _case(_f23, 2, 32, 32, 2)
CASES["f23_winograd_2h_2x8x6_64_64"] = _case(_f23, 2, 64, 64, 3)
CASES["f23_winograd_persist_4101x8x6_32_32"] = _case(_f23, 4101, 32, 32, 2)
CASES["f32_winograd_2x8x6_32_64"] = _case(_f32, 2, 32, 64, 2)
CASES["f32_winograd_2h_2x8x6_64_64"] = _case(_f32, 2, 64, 64, 3)


def bits(t):
    """A device tensor as the fixture stores it: float32 as uint32 bit patterns, integers raw; anything over DIGEST_ABOVE words as the eight
    uint32 words of the SHA-256 of those bits."""
    a = t.detach().cpu().numpy()
    a = a.view(np.uint32) if a.dtype.kind == "f" else a
    if a.size > DIGEST_ABOVE:
        return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint32).copy()
    return a


def run(vh, name):
    """-> {fixture key: bits} of one case: its outputs in the order the case returns them."""
    import torch
    outs = CASES[name](vh)
    torch.cuda.synchronize()
    return {f"{name}.{k}": bits(t) for k, t in enumerate(outs)}
