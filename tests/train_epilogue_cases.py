"""Inputs and case list of the training-epilogue bit fixture (tests/golden/train_epilogue_bits.npz): what tools/make_scorer_bits.py records from the
parent commit's library (``--cases tests.train_epilogue_cases``) and tests/test_gpu_scorer_bits.py replays.  Same protocol as tests/wino43_cases.py:
inputs are regenerated from the seeds, never stored; nothing here imports the library.  The kernels are the convolutions whose write-out runs the
training-mode BatchNorm pieces of csrc/bn_epilogue.h — the forward statistics (sum, sum^2) and the BatchNorm-backward epilogue (ReLU mask, masked
gradient g, (sum g, sum g * xhat)) — in csrc/conv_igemm.h (conv_epilogue, shared by the implicit GEMM and its stream-K form), conv_winograd.hip
(winograd_body: F(2x2,3x3), F(3x3,2x2) and its gather form) and winograd_f4.hip (f4_body).

Every case stores the written tensor, the used part of the float64 partials stats[:blocks * C * 2], the block count and the launch counts of ROUTES
(the fixture fails when a case stops reaching its instantiation).  Shapes (N, H, W, Cin, Cout) are the smallest that reach each branch:
  implicit GEMM, statistics     1x1 (2,8,6,64,256); 3x3 stride 2 (3,8,6,32,64); 3x3 stride 1 on the 32-wide tile with M = 105 rows (3,7,5,32,32: the
                                implicit GEMM takes input channels in multiples of 32); transposed conv (2,4,3,32,64)
  implicit GEMM, BN backward    stride-1 data gradient of (3,7,5,32,16) (dz carried in 32 channels, 128x32 tile) and of (2,8,6,256,64) (64x128 tile); the
                                four parity launches of a stride-2 3x3 data gradient appending to one BnBwdSpec, dz (2,4,3,64) -> dx (2,8,6,32); each with
                                the mask recomputed from (scale, bias) / taken from a saved y / absent, with and without a residual.  The first shape once
                                more inside vh.streamk_scope (its 32-wide tile stays on the whole-tile kernel: the route counts say so) and the smallest
                                launch stream-K accepts — 65 tiles of 64x128, 72 k-tiles: (86,8,6,128,256) — which runs the stream-K BNB instantiation
                                the 64x64 tile (2,8,6,64,32) and the 128x128 tile, which a launch takes from 768 blocks on: (16,64,48,256,32)
  F(2x2,3x3)                    statistics at (3,8,6,32,32) (36 tiles: a full block and a tail), (3,7,5,16,48) (odd plane, Cout no multiple of 32) and
                                (2,8,6,64,64) under vatl_tune_set(21, 3) (two-half blocks); BN backward on the first and the third, masks x residual
  F(3x3,2x2)                    statistics of the transposed conv at (2,4,3,32,64) and (3,5,4,16,32); its data gradient with a spec (the gather
                                instantiation) dz (2,8,6,32) -> dx (2,4,3,32) and 64 -> 64 under knob 21 = 3, three mask kinds each
  F(4x4,3x3)                    statistics and BN backward (three mask kinds) at (17,4,4,64,128) (17 tiles: the 16-tile tail block), (5,16,12,64,64)
                                and (3,8,12,128,256)
The route counters do not tell one-half from two-half Winograd blocks with the BN-backward epilogue: the f23_bnbwd_2x8x6x64x64_* and f32_dgrad_2h_*
cases count `winograd_bnbwd` like their one-half neighbours, and reach the two-half instantiations only because knob 21 = 3 and a 64-channel output make
the launcher choose them today; the fixture would not notice if they stopped (the forward-statistics case f23_stats_2h_* does: `winograd_2h`).
Outputs of more than 4096 words are stored as their SHA-256.
"""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_epilogue_bits.npz")
DIGEST_ABOVE = 4096
ROUTES = ("igemm", "igemm_bnbwd", "streamk", "winograd", "winograd_2h", "winograd_bnbwd", "winograd_f4", "winograd_f4_bnbwd")
MASKS = ("recompute", "saved", "none")
F4_SHAPES = ((17, 4, 4, 64, 128), (5, 16, 12, 64, 64), (3, 8, 12, 128, 256))


def _rand(seed, *shape):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def _put(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _flipped_taps(r, s):
    return [(r - 1 - i, s - 1 - j) for i in range(r) for j in range(s)]


def _spec(vh, mask, shape):
    """BnBwdSpec of a consumer layer whose conv output has ``shape`` (N, H, W, C), with one of the three MASKS."""
    c = shape[-1]
    z, mean, invstd = _put(_rand(21, *shape)), _put(_rand(22, c) * 0.1), _put(np.abs(_rand(23, c)) + 0.5)
    if mask == "recompute":
        return vh.BnBwdSpec(z, mean, invstd, scale=_put(np.abs(_rand(24, c)) + 0.5), bias=_put(_rand(25, c) * 0.3))
    if mask == "saved":
        return vh.BnBwdSpec(z, mean, invstd, mask_y=_put(_rand(26, *shape)))
    return vh.BnBwdSpec(z, mean, invstd)


def _res(shape, on):
    return _put(_rand(27, *shape)) if on else None


def _of_spec(g, spec):
    c = g.shape[-1]
    return g, spec.stats[:spec.blocks * c * 2], spec.blocks


def _igemm_stats(vh, shape, k, stride):
    n, h, w, cin, cout = shape
    x, wp = _put(_rand(1, n, h, w, cin)), vh.pack_conv_weight(_put(_rand(2, cout, cin, k, k) * 0.05))
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    return vh._stats_fwd("vatl_conv2d_fwd_stats", x, wp, (n, ho, wo, cout), vh.lib().vatl_conv_stats_row_blocks(n * ho * wo, 1),
                         (n, h, w, cin, cout, wp.shape[0], k, k, stride, pad))


def _igemm_deconv_stats(vh, shape):
    n, h, w, cin, cout = shape
    x, wp = _put(_rand(3, n, h, w, cin)), vh.pack_deconv_weight(_put(_rand(4, cin, cout, 4, 4) * 0.05))
    return vh._stats_fwd("vatl_deconv4x4s2_fwd_stats", x, wp, (n, 2 * h, 2 * w, cout), vh.lib().vatl_conv_stats_row_blocks(n * h * w, 4),
                         (n, h, w, cin, cout, wp.shape[1]))


def _igemm_dgrad_s1(vh, shape, mask, res, streamk=False):
    """Data gradient of a 3x3 / stride 1 / pad 1 conv (Cin -> Cout): a 3x3 conv of dz with Cin output channels; dz is carried in a multiple of 32 channels."""
    import torch
    n, h, w, cin, cout = shape
    ck = (cout + 31) // 32 * 32
    dz, wt = _put(_rand(5, n, h, w, ck)), _put(_rand(6, cout, cin, 3, 3) * 0.05)
    wd = vh.pack_dgrad_weight(wt, _flipped_taps(3, 3), cout_k=ck)
    spec = _spec(vh, mask, (n, h, w, cin))

    def go():
        return vh.conv2d_fwd_ex_bnbwd(dz, wd, cin, 3, 3, 1, 1, 1, h, w, h, w, 1, 1, 0, 0, spec, residual=_res((n, h, w, cin), res))
    if streamk:
        with vh.streamk_scope(torch.device("cuda:0"), force=True):
            return _of_spec(go(), spec)
    return _of_spec(go(), spec)


def _igemm_dgrad_s2(vh, mask, res):
    """The four parity launches of the data gradient of a 3x3 / stride 2 / pad 1 conv 32 -> 64: dz (2,4,3,64) -> dx (2,8,6,32), one BnBwdSpec."""
    import torch
    n, h, w, cin, cout, ho, wo = 2, 8, 6, 32, 64, 4, 3
    dz, wt = _put(_rand(7, n, ho, wo, cout)), _put(_rand(8, cout, cin, 3, 3) * 0.05)
    spec, r = _spec(vh, mask, (n, h, w, cin)), _res((n, h, w, cin), res)
    dx = torch.empty((n, h, w, cin), device=dz.device, dtype=torch.float32)
    for py in (0, 1):
        rows = [1] if py == 0 else [2, 0]
        for px in (0, 1):
            cols = [1] if px == 0 else [2, 0]
            wd = vh.pack_dgrad_weight(wt, [(a, b) for a in rows for b in cols])
            vh.conv2d_fwd_ex_bnbwd(dz, wd, cin, len(rows), len(cols), 1, 0, 0, ho, wo, h, w, 2, 2, py, px, spec, out=dx, residual=r)
    return _of_spec(dx, spec)


def _f23_stats(vh, shape):
    n, h, w, cin, cout = shape
    x, wt = _put(_rand(9, n, h, w, cin)), _put(_rand(10, cout, cin, 3, 3) * 0.05)
    return vh.conv3x3_winograd_fwd_stats(x, vh.pack_winograd_weight(wt), cout)


def _f23_bnbwd(vh, shape, mask, res):
    """Data gradient of the 3x3 layer Cin -> Cout: dz (N,H,W,Cout) -> g (N,H,W,Cin)."""
    n, h, w, cin, cout = shape
    dz, wt = _put(_rand(11, n, h, w, cout)), _put(_rand(12, cout, cin, 3, 3) * 0.05)
    spec = _spec(vh, mask, (n, h, w, cin))
    g = vh.conv3x3_winograd_fwd_bnbwd(dz, vh.pack_winograd_weight(wt, data_gradient=True), cin, spec, residual=_res((n, h, w, cin), res))
    return _of_spec(g, spec)


def _f32_stats(vh, shape):
    n, h, w, cin, cout = shape
    x, wt = _put(_rand(13, n, h, w, cin)), _put(_rand(14, cin, cout, 4, 4) * 0.05)
    return vh._stats_fwd("vatl_deconv4x4s2_winograd_fwd_stats", x, vh.pack_winograd_deconv_weight(wt), (n, 2 * h, 2 * w, cout),
                         vh.lib().vatl_winograd_deconv_stats_row_blocks(n, h, w), (n, h, w, cin, cout))


def _f32_dgrad(vh, shape, mask):
    """Data gradient of the transposed conv Cin -> Cout on an (H, W) input: dz (N,2H,2W,Cout) -> g (N,H,W,Cin), the gather instantiation."""
    n, h, w, cin, cout = shape
    dz, wt = _put(_rand(15, n, 2 * h, 2 * w, cout)), _put(_rand(16, cin, cout, 4, 4) * 0.05)
    spec = _spec(vh, mask, (n, h, w, cin))
    return _of_spec(vh.deconv4x4s2_winograd_dgrad(dz, vh.pack_winograd_deconv_dgrad_weight(wt), cin, spec=spec), spec)


def _f4_stats(vh, shape):
    n, h, w, cin, cout = shape
    x, wt = _put(_rand(17, n, h, w, cin)), _put(_rand(18, cout, cin, 3, 3) * (2.0 / (9 * cin)) ** 0.5)
    return vh._stats_fwd("vatl_conv3x3_winograd_f4_fwd_stats", x, vh.pack_winograd_f4_weight(wt), (n, h, w, cout),
                         vh.lib().vatl_winograd_f4_stats_row_blocks(n, h, w), (n, h, w, cin, cout))


def _f4_bnbwd(vh, shape, mask):
    n, h, w, cin, cout = shape
    dz, wt = _put(_rand(19, n, h, w, cout)), _put(_rand(20, cout, cin, 3, 3) * (2.0 / (9 * cin)) ** 0.5)
    spec = _spec(vh, mask, (n, h, w, cin))
    g = vh.conv3x3_winograd_f4_fwd_bnbwd(dz, vh.pack_winograd_f4_weight(wt, data_gradient=True), cin, spec, residual=_res((n, h, w, cin), mask != "recompute"))
    return _of_spec(g, spec)


def _case(fn, *args, halves=2):
    return lambda vh: _metered(vh, halves, lambda: fn(vh, *args))


def _metered(vh, halves, fn):
    """fn() -> (tensor, partials, blocks) under vatl_tune_set(21, halves), with the launch counts of ROUTES."""
    import torch
    vh.tune_set(21, halves)
    try:
        with vh.flop_meter() as fm:
            y, stats, blocks = fn()
    finally:
        vh.tune_set(21, 2)
    c = y.shape[-1]
    return (y, stats[:int(blocks) * c * 2], torch.tensor([int(blocks)], dtype=torch.int64),
            torch.tensor([fm.routes[r] for r in ROUTES], dtype=torch.int64))


def _tag(shape):
    return "x".join(str(v) for v in shape)


CASES = {}
CASES["igemm_stats_1x1_2x8x6x64x256"] = _case(_igemm_stats, (2, 8, 6, 64, 256), 1, 1)
CASES["igemm_stats_3x3s2_3x8x6x32x64"] = _case(_igemm_stats, (3, 8, 6, 32, 64), 3, 2)
CASES["igemm_stats_3x3_3x7x5x32x32"] = _case(_igemm_stats, (3, 7, 5, 32, 32), 3, 1)
CASES["igemm_stats_deconv_2x4x3x32x64"] = _case(_igemm_deconv_stats, (2, 4, 3, 32, 64))
for _m in MASKS:
    for _r in (False, True):
        _sfx = f"{_m}_res" if _r else _m
        for _s in ((3, 7, 5, 32, 16), (2, 8, 6, 256, 64)):
            CASES[f"igemm_bnbwd_{_tag(_s)}_{_sfx}"] = _case(_igemm_dgrad_s1, _s, _m, _r)
        CASES[f"igemm_bnbwd_s2_2x8x6x32x64_{_sfx}"] = _case(_igemm_dgrad_s2, _m, _r)
        for _s, _h in (((3, 8, 6, 32, 32), 2), ((2, 8, 6, 64, 64), 3)):
            CASES[f"f23_bnbwd_{_tag(_s)}_{_sfx}"] = _case(_f23_bnbwd, _s, _m, _r, halves=_h)
CASES["igemm_bnbwd_64x64_2x8x6x64x32"] = _case(_igemm_dgrad_s1, (2, 8, 6, 64, 32), "recompute", True)
CASES["igemm_bnbwd_128x128_16x64x48x256x32"] = _case(_igemm_dgrad_s1, (16, 64, 48, 256, 32), "saved", False)
CASES["igemm_bnbwd_3x7x5x32x16_in_streamk_scope"] = _case(_igemm_dgrad_s1, (3, 7, 5, 32, 16), "recompute", True, True)
CASES["streamk_bnbwd_86x8x6x128x256"] = _case(_igemm_dgrad_s1, (86, 8, 6, 128, 256), "recompute", True, True)
CASES["f23_stats_3x8x6x32x32"] = _case(_f23_stats, (3, 8, 6, 32, 32))
CASES["f23_stats_3x7x5x16x48"] = _case(_f23_stats, (3, 7, 5, 16, 48))
CASES["f23_stats_2h_2x8x6x64x64"] = _case(_f23_stats, (2, 8, 6, 64, 64), halves=3)
CASES["f32_stats_2x4x3x32x64"] = _case(_f32_stats, (2, 4, 3, 32, 64))
CASES["f32_stats_3x5x4x16x32"] = _case(_f32_stats, (3, 5, 4, 16, 32))
for _m in MASKS:
    CASES[f"f32_dgrad_2x4x3x32x32_{_m}"] = _case(_f32_dgrad, (2, 4, 3, 32, 32), _m)
    CASES[f"f32_dgrad_2h_2x4x3x64x64_{_m}"] = _case(_f32_dgrad, (2, 4, 3, 64, 64), _m, halves=3)
for _s in F4_SHAPES:
    CASES[f"f4_stats_{_tag(_s)}"] = _case(_f4_stats, _s)
    for _m in MASKS:
        CASES[f"f4_bnbwd_{_tag(_s)}_{_m}"] = _case(_f4_bnbwd, _s, _m)


def bits(t):
    """A device tensor as the fixture stores it: float32 / float64 as uint32 / uint64 bit patterns, integers raw; anything over DIGEST_ABOVE words as
    the eight uint32 words of the SHA-256 of those bits."""
    a = t.detach().cpu().numpy()
    a = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a
    if a.size > DIGEST_ABOVE:
        return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint32).copy()
    return a


def run(vh, name):
    """-> {fixture key: bits} of one case: the written tensor, the used partials, the block count, the route counts."""
    import torch
    outs = CASES[name](vh)
    torch.cuda.synchronize()
    return {f"{name}.{k}": bits(t) for k, t in enumerate(outs)}
