"""Weight-gradient kernels (csrc/conv_wgrad.hip, csrc/winograd_wgrad.hip): the seeded cases of tests/test_wgrad_cpu.py and
tests/test_gpu_wgrad.py, a float64 reference, and impulse inputs whose exact result is known without any arithmetic.

    dW[n][t][c] = sum_m G[m][n] * X[pix(m) + tap t][c]
    G (M, Gs)        the "plain" operand, NHWC rows m = (b, oy, ox): dz of a conv (Gs = CoutG >= Cout), the layer input of the
                     transposed conv
    X (N, Hg, Wg, Cx) the "gathered" operand: the conv input (4 channels for the 3-channel stem), dy of the transposed conv
    pix(m) + t       (oy*stride - pad + r, ox*stride - pad + s); a tap outside the image contributes zero

A case is ``(entry, N, H, W, Cin, Cout, CoutG, k, stride, pad)``: N, H, W are the layer INPUT's, as the wrappers take them.  Inputs are
regenerated from the case's seed, never stored.  The channels Cout..CoutG-1 of dz and the fourth channel of the stem's input carry
random values in every input set: the kernels must leave them out.

Impulse inputs: channel n of the plain operand is 1.0 at one pixel p_n and 0 elsewhere, the gathered operand is random.  Then
dW[n, :, r, s] is a copy of the gathered operand at p_n + (r, s), zero where the tap leaves the image: the direct kernel sums one
product by 1.0 and zeros, the slice reduction adds zeros, so every bit is known.

The module also restates the host-side shape rules (tile choice, packed taps, split counts) so that the pixel list can name the split
boundary and the CPU test can hold every case's comment to them; the GPU test holds the library itself to the same claims.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

DIRECT, DECONV, WINO, WINO_DECONV = "conv2d_wgrad", "deconv4x4s2_wgrad", "conv3x3_winograd_wgrad", "deconv4x4s2_winograd_wgrad"

CASES = []
CLAIMS = {}        # case -> what its comment claims: direct {"tile": (BN, BJ), "tpt", "slices"}; Winograd {"halves", "table", "splits"}


def _direct(entry, n, h, w, cin, cout, k, stride, pad, tile, slices, tpt=1, coutg=None):
    case = (entry, n, h, w, cin, cout, coutg or cout, k, stride, pad)
    CASES.append(case)
    CLAIMS[case] = {"tile": tile, "tpt": tpt, "slices": slices}


def _wino(entry, n, h, w, cin, cout, halves, table, splits):
    case = (entry, n, h, w, cin, cout, cout, 3, 1, 1) if entry == WINO else (entry, n, h, w, cin, cout, cout, 4, 2, 1)
    CASES.append(case)
    CLAIMS[case] = {"halves": halves, "table": table, "splits": splits}


# ---- conv2d_wgrad: the shapes the suite already had (tests/test_gpu_train.py), here also for the impulse and element-wise checks
_direct(DIRECT, 2, 16, 12, 256, 64, 1, 1, 0, (64, 128), 3)           # GRAD_CASES 1x1_256_64: 64x128 tile, 12 k-tiles in three splits
_direct(DIRECT, 2, 16, 12, 64, 256, 1, 1, 0, (128, 64), 3)           # GRAD_CASES 1x1_64_256: 128x64 tile
_direct(DIRECT, 2, 16, 12, 64, 64, 3, 1, 1, (64, 64), 3)             # GRAD_CASES 3x3_64_64: 64x64 tile, nine taps unpacked
_direct(DIRECT, 3, 8, 6, 128, 128, 3, 1, 1, (128, 128), 2)           # GRAD_CASES 3x3_128_128: 128x128 tile, 4 + 1 k-tiles (last one half full)
_direct(DIRECT, 2, 16, 12, 128, 128, 3, 2, 1, (128, 128), 1)         # GRAD_CASES 3x3s2_128_128: stride 2 on an even plane, one split
_direct(DIRECT, 2, 16, 12, 256, 512, 1, 2, 0, (128, 128), 1)         # GRAD_CASES 1x1s2_256_512: projection, four row tiles
_direct(DIRECT, 1, 8, 6, 512, 512, 3, 1, 1, (128, 128), 1)           # GRAD_CASES 3x3_512_512_oddM: M = 48, second k-tile half full
_direct(DIRECT, 2, 32, 24, 3, 64, 7, 2, 3, (64, 32), 6)              # stem of test_stem_and_head_wgrad: three splits x two k-step waves
_direct(DIRECT, 2, 16, 12, 256, 17, 1, 1, 0, (32, 128), 3, coutg=32)  # head of test_stem_and_head_wgrad: 17 of 32 channels, 32x128 tile
# ---- conv2d_wgrad: one case per tile, packing and walk branch
_direct(DIRECT, 2, 8, 6, 256, 256, 1, 1, 0, (128, 128), 1)           # 128x128 tile on a 1x1 filter
_direct(DIRECT, 3, 7, 5, 64, 160, 1, 1, 0, (128, 64), 1)             # 128x64 tile; Cn tail 128 + 32; M = 105
_direct(DIRECT, 3, 7, 5, 192, 48, 3, 1, 1, (64, 128), 1)             # 64x128 tile; Cn 48 of 64; second column tile half empty
_direct(DIRECT, 2, 9, 7, 48, 96, 3, 2, 1, (64, 64), 1)               # 64x64 tile; 64 % 48 != 0: unpacked with a channel mask; Ho*Wo = 20 < 32: the image carry fires every k-tile
_direct(DIRECT, 2, 8, 6, 128, 17, 3, 1, 1, (32, 128), 1, coutg=32)   # FastPose head: 3x3, 17 of 32 channels
_direct(DIRECT, 2, 8, 6, 32, 17, 1, 1, 0, (32, 128), 1, tpt=4, coutg=32)    # tpt = 4 with a single tap: three quarters of the column tile have no tap
_direct(DIRECT, 2, 8, 6, 64, 18, 3, 1, 1, (32, 128), 1, tpt=2, coutg=32)    # DCN v1 offset conv: tpt = 2, five tap groups, the last holding one tap
_direct(DIRECT, 2, 8, 6, 128, 27, 3, 2, 1, (32, 128), 1, coutg=32)   # DCN v2 offset + mask conv at stride 2: 27 of 32 channels
_direct(DIRECT, 2, 8, 6, 32, 32, 3, 1, 1, (32, 128), 1, tpt=4)       # HRNet 32-channel branch: tpt = 4, tap groups 4 + 4 + 1
_direct(DIRECT, 2, 8, 6, 32, 64, 3, 2, 1, (64, 64), 1, tpt=2)        # HRNet fuse: 64x64 tile, tpt = 2, five tap groups, stride 2
_direct(DIRECT, 1, 5, 3, 16, 64, 3, 1, 1, (64, 64), 1, tpt=4)        # M = 15: one partial k-tile
_direct(DIRECT, 5, 1, 1, 256, 16, 1, 1, 0, (32, 128), 1)             # SE Linear squeeze: Ho*Wo = 1, M = 5 below one k-tile
_direct(DIRECT, 5, 1, 1, 16, 256, 1, 1, 0, (128, 64), 1, tpt=4)      # SE Linear excite: 128x64 tile packs its single tap (tpt = 4)
_direct(DIRECT, 33, 1, 1, 256, 16, 1, 1, 0, (32, 128), 1)            # SE Linear: M = 33, one row into the second k-tile
_direct(DIRECT, 2, 4, 3, 576, 64, 1, 1, 0, (64, 128), 1)             # DCN column GEMM (Cx = 9 * 64): five column tiles, the last half full
_direct(DIRECT, 2, 7, 5, 64, 128, 1, 2, 0, (128, 64), 1)             # stride-2 1x1 projection on an odd plane (Ho*Wo = 12)
_direct(DIRECT, 3, 1, 9, 64, 64, 3, 1, 1, (64, 64), 1)               # Ho = 1: every row tap but the middle one leaves the image
_direct(DIRECT, 3, 9, 1, 64, 64, 3, 1, 1, (64, 64), 1)               # Wo = 1: the column carry fires at every pixel
_direct(DIRECT, 5, 8, 8, 64, 64, 3, 1, 1, (64, 64), 3)               # ten k-tiles in splits of 4, 4, 2
_direct(DIRECT, 2, 24, 24, 64, 64, 1, 1, 0, (64, 64), 9)             # 9 slices: the reduction's remainder loop alone, one lane with two slices
_direct(DIRECT, 2, 64, 48, 64, 64, 1, 1, 0, (64, 64), 48)            # 48 slices: the reduction's four-chain loop and its remainder loop
_direct(DIRECT, 3, 18, 14, 3, 64, 7, 2, 3, (64, 32), 4)              # stem on an odd output plane (9x7): two splits, two slices (k-step waves) per split
_direct(DIRECT, 1, 8, 8, 3, 64, 7, 2, 3, (64, 32), 2)                # stem with M = 16: half a k-tile, two slices per split
# ---- deconv4x4s2_wgrad (rows = Cin of the layer, gathered operand = dy)
_direct(DECONV, 2, 8, 6, 256, 128, 4, 2, 1, (128, 128), 1)           # test_deconv_backward: 128x128 tile over 16 taps
_direct(DECONV, 1, 5, 3, 64, 64, 4, 2, 1, (64, 64), 1)               # test_deconv_backward: 64x64 tile, M = 15
_direct(DECONV, 3, 5, 4, 32, 32, 4, 2, 1, (32, 128), 1, tpt=4)       # 32x128 tile, tpt = 4 over 16 taps
_direct(DECONV, 2, 3, 7, 160, 48, 4, 2, 1, (128, 64), 1)             # Cn tail 128 + 32; 64 % 48 != 0: unpacked with a channel mask
# ---- conv3x3_winograd_wgrad
_wino(WINO, 2, 8, 6, 256, 256, 2, True, 3)                           # two halves
_wino(WINO, 3, 7, 5, 256, 320, 2, True, 5)                           # two halves, odd plane, five channel tiles
_wino(WINO, 3, 10, 14, 288, 256, 2, True, 14)                        # two halves; nine input tiles; the finish kernel's partial 64-group; 105 tiles in 14 splits, the last one-eighth full
_wino(WINO, 1, 3, 3, 512, 256, 2, True, 1)                           # two halves; 4 tiles, fewer than one stage
_wino(WINO, 2, 8, 6, 256, 288, 1, True, 3)                           # stays one-half: 288 % 64 != 0
_wino(WINO, 3, 13, 9, 32, 48, 1, False, 14)                          # WGRAD_CASES of tests/test_gpu_winograd.py: Cout no whole tile, so in-kernel addresses
# ---- deconv4x4s2_winograd_wgrad
_wino(WINO_DECONV, 2, 5, 7, 128, 64, 1, True, 2)                     # plane not a multiple of 3
_wino(WINO_DECONV, 3, 2, 9, 128, 128, 1, True, 2)                    # one tile row of two pixels, three tile columns

TWO_HALF_CASES = [c for c in CASES if CLAIMS[c].get("halves") == 2]


def case_id(case):
    entry, n, h, w, cin, cout, coutg, k, stride, _ = case
    short = {DIRECT: "conv", DECONV: "deconv", WINO: "wino", WINO_DECONV: "winodeconv"}[entry]
    return f"{short}-{n}x{h}x{w}-{cin}-{cout}" + (f"in{coutg}" if coutg != cout else "") + f"-k{k}s{stride}"


def seed(case):
    return zlib.crc32(case_id(case).encode()) % 2 ** 31


def is_deconv(case):
    return case[0] in (DECONV, WINO_DECONV)


def is_winograd(case):
    return case[0] in (WINO, WINO_DECONV)


def geometry(case):
    """Shapes of a case: plain operand (N, Ho, Wo, Gs) with Cn valid channels, gathered operand (N, Hg, Wg, Cx) with Cv valid
    channels, the (R, S, stride, pad) of the gather, M, and the shape of dW."""
    _, n, h, w, cin, cout, coutg, k, stride, pad = case
    if is_deconv(case):
        return dict(N=n, Ho=h, Wo=w, Gs=cin, Cn=cin, Hg=2 * h, Wg=2 * w, Cx=cout, Cv=cout, R=4, S=4, stride=2, pad=1, M=n * h * w, dw=(cin, cout, 4, 4))
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    return dict(N=n, Ho=ho, Wo=wo, Gs=coutg, Cn=cout, Hg=h, Wg=w, Cx=4 if cin == 3 else cin, Cv=cin, R=k, S=k, stride=stride, pad=pad, M=n * ho * wo,
                dw=(cout, cin, k, k))


# ---- the host-side shape rules, restated ------------------------------------------------------------------------------------------

def _cdiv(a, b):
    return -(-a // b)


def direct_plan(case):
    """wgrad_cfg / wgrad_tpt / wgrad_plan of csrc/conv_wgrad.hip at their defaults."""
    g = geometry(case)
    cn, cx, taps, m = g["Cn"], g["Cx"], g["R"] * g["S"], g["M"]
    stem = case[0] == DIRECT and case[4] == 3
    if stem:
        bn, bj = 64, 32
    elif cn >= 128:
        bn, bj = 128, (128 if cx >= 128 else 64)
    elif cn > 32:
        bn, bj = 64, (128 if cx >= 128 else 64)
    else:
        bn, bj = 32, 128
    tpt = bj // cx if (not stem and cx < bj and bj % cx == 0) else 1
    tiles = _cdiv(cn, bn) * (g["R"] if stem else _cdiv(taps, tpt)) * (1 if stem else _cdiv(cx, bj))
    ktiles = _cdiv(m, 32)
    splits = max(1, min((512 if taps == 1 else 1024) // tiles, (ktiles + 3) // 4))
    kps = _cdiv(ktiles, splits)
    splits = _cdiv(ktiles, kps)
    packed = g["Cn"] * (g["R"] * 32 if stem else taps * cx)
    return dict(tile=(bn, bj), tpt=tpt, tiles=tiles, ktiles=ktiles, splits=splits, kps=kps, slices=splits * (2 if stem else 1), packed=packed,
                flops=2.0 * tiles * bn * bj * 32 * ktiles)


def winograd_plan(case):
    """ww_plan of csrc/winograd_wgrad.hip at its defaults (two halves where the layer allows, 1024 target blocks, address tables)."""
    g = geometry(case)
    mo = 3 if is_deconv(case) else 2
    cn, cx = (g["Cx"], g["Cn"]) if is_deconv(case) else (g["Cn"], g["Cx"])       # the transposed conv's transform-domain rows are Cout
    th, tw = _cdiv(g["Ho"], mo), _cdiv(g["Wo"], mo)
    mtiles = g["N"] * th * tw
    halves = 2 if (mo == 2 and cn % 64 == 0 and cn >= 256 and cx >= 256) else 1
    per_split = _cdiv(cn, 32 * halves) * _cdiv(cx, 32) * (4 if mo == 3 else 1)
    stages = _cdiv(mtiles, 8)
    want = min(max(1, 1024 * (4 if mo == 3 else 1) // per_split), stages)
    tps = _cdiv(stages, want) * 8
    splits, table, phases = _cdiv(mtiles, tps), cx % 32 == 0 and cn % (32 * halves) == 0, 4 if mo == 3 else 1
    cn_pad, cx_pad = _cdiv(cn, 32 * halves) * 32 * halves, _cdiv(cx, 32) * 32
    # workspace: the splits' partial sums in the transform domain, then the staging-address tables (x per phase and stage, gradient per stage)
    ns = 7 * mo + 4 + (4 - mo) * ((tw + 6) // tw)
    floats = splits * phases * (3 if mo == 2 else 2) * 4 * cn_pad * cx_pad
    if table:
        floats += (phases * _cdiv(4 * ns * 8, 64) + _cdiv(mo * 8 * mo * 8 * halves, 64)) * stages * 64
    return dict(mo=mo, th=th, tw=tw, mtiles=mtiles, halves=halves, tps=tps, splits=splits, table=table, floats=floats,
                flops=2.0 * cn_pad * cx_pad * 16 * phases * stages * 8)


def plan(case):
    return winograd_plan(case) if is_winograd(case) else direct_plan(case)


# ---- the pixels of the impulses -----------------------------------------------------------------------------------------------------

def pixels(case):
    """[(kind, m)] in the order they are dealt to the channels; m = (b*Ho + oy)*Wo + ox indexes the plain operand's rows."""
    g = geometry(case)
    n, ho, wo, m_all = g["N"], g["Ho"], g["Wo"], g["M"]
    at = lambda b, oy, ox: (b * ho + oy) * wo + ox
    out = [("row0", 0)] + [(f"row{m}", m) for m in (31, 32) if m < m_all] + [("last_row", m_all - 1)]
    q = plan(case)
    if q["splits"] > 1:
        if is_winograd(case):                         # splits own tps tiles: the last pixel of the first split's last tile, the first of the next tile
            mo, tw, tpi = q["mo"], q["tw"], q["th"] * q["tw"]
            first = lambda t: (t // tpi, (t % tpi) // tw * mo, t % tw * mo)
            b, oy, ox = first(q["tps"] - 1)
            out += [("split_end", at(b, min(oy + mo, ho) - 1, min(ox + mo, wo) - 1)), ("split_start", at(*first(q["tps"])))]
        else:
            out += [("split_end", q["kps"] * 32 - 1), ("split_start", q["kps"] * 32)]
    for b in sorted({0, n - 1}):
        out += [(f"corner_b{b}_y{oy}x{ox}", at(b, oy, ox)) for oy in sorted({0, ho - 1}) for ox in sorted({0, wo - 1})]
    out += [("last_column", at(0, ho // 2, wo - 1)), ("last_line", at(n - 1, ho - 1, wo // 2))]
    if ho * wo < 32:
        out += [(f"image{b}", at(b, (b * 7) % ho, (b * 3) % wo)) for b in range(min(n, _cdiv(32, ho * wo)))]
    return out


def impulse_pixel(case, channel):
    """m of the one pixel where ``channel`` of the plain operand is 1.0: the distinct pixels of the list, dealt cyclically."""
    distinct = list(dict.fromkeys(m for _, m in pixels(case)))
    return distinct[channel % len(distinct)]


# ---- inputs, reference, expectation -------------------------------------------------------------------------------------------------

def _randn(r, shape):
    return r.standard_normal(shape).astype(np.float32)


def random_inputs(case):
    """-> (plain (N,Ho,Wo,Gs), gathered (N,Hg,Wg,Cx)) float32 NHWC, every element random."""
    g, r = geometry(case), np.random.RandomState(seed(case))
    return _randn(r, (g["N"], g["Ho"], g["Wo"], g["Gs"])), _randn(r, (g["N"], g["Hg"], g["Wg"], g["Cx"]))


def impulse(case):
    """-> (plain, gathered, expected): plain one-hot per valid channel (random in the padding channels), gathered random, and the exact
    dW (float64 of float32 values) copied from the gathered operand."""
    g, r = geometry(case), np.random.RandomState(seed(case) ^ 0x5A5A)
    gathered = _randn(r, (g["N"], g["Hg"], g["Wg"], g["Cx"]))
    plain = _randn(r, (g["N"], g["Ho"], g["Wo"], g["Gs"]))
    plain[..., :g["Cn"]] = 0
    expected = np.zeros(g["dw"], np.float64)
    rows = plain.reshape(g["M"], g["Gs"])
    for ch in range(g["Cn"]):
        m = impulse_pixel(case, ch)
        rows[m, ch] = 1.0
        b, oy, ox = m // (g["Ho"] * g["Wo"]), m // g["Wo"] % g["Ho"], m % g["Wo"]
        for rr in range(g["R"]):
            for ss in range(g["S"]):
                iy, ix = oy * g["stride"] - g["pad"] + rr, ox * g["stride"] - g["pad"] + ss
                if 0 <= iy < g["Hg"] and 0 <= ix < g["Wg"]:
                    expected[ch, :, rr, ss] = gathered[b, iy, ix, :g["Cv"]]
    return plain, gathered, expected


def reference(case, inputs=None):
    """dW in float64 by torch autograd on the CPU (F.conv2d / F.conv_transpose2d) of ``inputs`` = (plain, gathered), by default the
    case's random inputs.  Only the valid channels of either operand enter."""
    g = geometry(case)
    plain, gathered = inputs if inputs is not None else random_inputs(case)
    p = torch.from_numpy(np.ascontiguousarray(plain[..., :g["Cn"]])).double().permute(0, 3, 1, 2)
    x = torch.from_numpy(np.ascontiguousarray(gathered[..., :g["Cv"]])).double().permute(0, 3, 1, 2)
    wt = torch.zeros(g["dw"], dtype=torch.float64, requires_grad=True)
    if is_deconv(case):
        F.conv_transpose2d(p, wt, None, 2, 1).backward(x)
    else:
        F.conv2d(x, wt, None, g["stride"], g["pad"]).backward(p)
    return wt.grad.numpy()


def abs_sum(case, inputs=None):
    """S = sum_m |G[m][n] * X[...]| per element of dW, in float64: the scale of the element-wise rounding bound."""
    plain, gathered = inputs if inputs is not None else random_inputs(case)
    return reference(case, (np.abs(plain), np.abs(gathered)))


U = 2.0 ** -24


def elementwise_bound(case, slices, s):
    """2 * gamma_n * S with n = M + slices + 17: M rounded products summed in any order, then the slices; the factor 2 covers the
    matrix core pairing two products per step."""
    n = geometry(case)["M"] + slices + 17
    return 2.0 * (n * U / (1.0 - n * U)) * s
