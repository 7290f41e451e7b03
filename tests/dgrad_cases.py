"""fp32 data gradients (alphapose/models/hip_train.py: _ConvBN._dgrad — _igemm_dgrad, the launch logic on vatl_conv2d_fwd_ex every layer class
shares, and the F(2x2,3x3) data-gradient filter): the seeded cases of tests/test_dgrad_cpu.py and tests/test_gpu_dgrad.py, one per launch
branch, a float64 reference, and a host restatement of everything between the layer and the kernel.  The module imports no library: it is
proved against autograd on the host (tests/test_dgrad_cpu.py) before the GPU test holds the library to it.

    dx[b][iy][ix][c] = sum_{n, r, s} dz[b][oy][ox][n] * w[n][c][r][s]   with (iy, ix) = (oy*stride - pad + r, ox*stride - pad + s)   (+ residual)
    dz (N, Ho, Wo, CoutK)   NHWC gradient of the conv's output; CoutK >= Cout is what the tensor carries (the 17-joint head and the DCN offset conv
                            travel in 32 channels), ZERO behind Cout: the packed filter is zero there as well, and 0 * 0 adds nothing
    w  (Cout, Cin, k, k)    the conv's own filter.  Its Cout is the reduction of the data gradient, its Cin the output width
    dx (N, H, W, Cin)       NHWC

A case is ``Case(route, n, h, w, cin, cout, k, stride, pad, coutk, via, knobs, scope)``: n, h, w are the layer INPUT's (= dx's).  ``route`` is the
route counter the case must bump, ``via`` says who issues the launches ("layer": _ConvBN._dgrad; "direct": the launches of ``launches(case)`` on
conv2d_fwd_ex with ``cout_k``, which must equal what _igemm_dgrad issues with the ``cout_k`` _DeformConvBN.backward and the head pass),
``knobs`` the product knobs set for the run (all documented bit-identical), ``scope`` whether the run is inside vatl_hip.streamk_scope.
Inputs are regenerated from the case's seed, never stored.
"""
import zlib
from collections import Counter, namedtuple

import numpy as np
import torch
import torch.nn.functional as F

Case = namedtuple("Case", "route n h w cin cout k stride pad coutk via knobs scope")
Launch = namedtuple("Launch", "taps r s pad_y pad_x ho wo osy osx ooy oox")

IGEMM, PERSISTENT, RING, STREAMK, WINO, WINO_2H = "igemm", "persistent_1x1", "gemm1x1_ring", "streamk", "winograd", "winograd_2h"
WINO_PERSIST = "winograd_persist"
BM, VAR, PERSIST_K, WINO_HALVES = 5, 0, 7, 21                       # product knobs (include/vatl_hip.h): tile rows, k-loop schedule, persistent K limit, halves
KNOB_DEFAULTS = {BM: 0, VAR: 4, PERSIST_K: 1, WINO_HALVES: 2}

CASES = []
CLAIMS = {}        # case -> what its comment claims: {"tile": (BM, BN)} (+ "var": per launch, on the 128x32 tile), Winograd {"halves": 1 | 2}


def _case(route, n, h, w, cin, cout, k=1, stride=1, pad=0, coutk=None, via="layer", knobs=(), scope=False, **claim):
    case = Case(route, n, h, w, cin, cout, k, stride, pad, coutk or cout, via, tuple(knobs), scope)
    CASES.append(case)
    CLAIMS[case] = claim
    return case


# ---- implicit GEMM, 128x32 tile (output width <= 32)
_case(IGEMM, 3, 7, 7, 32, 64, tile=(128, 32), var=[0])                              # 1x1 64 -> 32: two k-tiles, VAR 0 (nothing to pipeline); M = 147, two blocks
_case(IGEMM, 2, 16, 12, 32, 64, 3, 2, 1, tile=(128, 32), var=[0, 4, 4, 4])          # HRNet transition 3x3/2 from 32 channels: phases of 2, 4, 4, 8 k-tiles, VAR 0 then VAR 4
# ---- 64x64 tile
_case(IGEMM, 3, 7, 5, 64, 128, tile=(64, 64))                                       # full: 64 output channels; M = 105, second block ragged
_case(IGEMM, 2, 9, 7, 48, 96, tile=(64, 64))                                        # ragged: HRNet-W48's 48 output channels in a 64 tile
# ---- 64x128 tile
_case(IGEMM, 3, 7, 5, 128, 64, tile=(64, 128))                                      # full: 128 output channels
_case(IGEMM, 2, 9, 7, 96, 64, tile=(64, 128))                                           # ragged: 96 of 128
_case(IGEMM, 2, 5, 7, 192, 96, tile=(64, 128))                                      # ragged: 192 in two tiles, the second half empty
# ---- 128-row tiles through knob 5 (the dispatcher picks them from 768 / 1536 blocks on)
_case(IGEMM, 3, 5, 3, 64, 96, knobs=[(BM, 128)], tile=(128, 64))                    # 128x64, M = 45 below one tile
_case(IGEMM, 2, 13, 9, 64, 32, knobs=[(BM, 128)], tile=(128, 64))                   # 128x64, M = 234 = 128 + 106
_case(IGEMM, 3, 5, 3, 128, 288, knobs=[(BM, 128)], tile=(128, 128))                 # 128x128, nine k-tiles (past the persistent kernel, short of the ring), M = 45
_case(IGEMM, 2, 13, 9, 160, 288, knobs=[(BM, 128)], tile=(128, 128))                # 128x128, M = 234, 160 output channels in two tiles
_case(IGEMM, 2, 14, 10, 128, 64, 3, 2, 1, knobs=[(BM, 128)], tile=(128, 128))       # 128x128 under the four scattered phases, M = 70
# ---- stride 1, 3x3, on the implicit GEMM: nine flipped taps, pad r - 1 - pad
_case(IGEMM, 2, 5, 3, 64, 64, 3, 1, 1, via="direct", tile=(64, 64))                 # as _DeformConvBN issues it
_case(IGEMM, 2, 6, 5, 40, 32, 3, 1, 1, tile=(64, 64))                               # 40 input channels: the Winograd route refuses (not a multiple of 16)
_case(IGEMM, 2, 6, 4, 64, 32, 3, 1, 0, tile=(64, 64))                               # pad 0: the data gradient pads by 2, dz is 4x2
# ---- padded K: the reduction carried in more channels than the filter has
_case(IGEMM, 2, 8, 6, 256, 17, coutk=32, via="direct", tile=(64, 128))              # 17-joint head in 32 channels
_case(IGEMM, 2, 6, 4, 64, 27, 3, 1, 1, coutk=32, via="direct", tile=(64, 64))       # DCN v2 offset + mask conv: 27 in 32, nine taps
_case(IGEMM, 2, 8, 6, 128, 27, 3, 2, 1, coutk=32, via="direct", tile=(64, 128))     # ... at stride 2: four phases with cout_k
# ---- 1x1 / stride 2: one launch scattered to the even pixels
_case(IGEMM, 2, 10, 6, 64, 128, 1, 2, 0, tile=(64, 64))                             # dz 5x3
_case(IGEMM, 1, 4, 4, 256, 512, 1, 2, 0, tile=(64, 128))                            # ResNet projection, M = 4
# ---- 3x3 / stride 2 / pad 1: four phases of 1, 2, 2, 4 taps; the last dz row and column feed the odd phases alone
_case(IGEMM, 2, 2, 2, 64, 32, 3, 2, 1, tile=(64, 64))                               # dz 1x1: every tap but one of each phase leaves dz
_case(IGEMM, 3, 6, 4, 48, 96, 3, 2, 1, tile=(64, 64))                               # dz 3x2, ragged output channels
_case(IGEMM, 2, 16, 12, 128, 64, 3, 2, 1, tile=(64, 128))                           # dz 8x6
# ---- persistent 1x1 GEMM and LDS-DMA ring: whole 128x128 tiles of a stride-1 1x1 layer, smallest shapes their gates admit with knob 5 = 128
_case(PERSISTENT, 1, 5, 3, 128, 32, knobs=[(BM, 128)], tile=(128, 128))             # one k-tile: the look-ahead-1 kernel; M = 15
_case(PERSISTENT, 2, 13, 9, 96, 256, knobs=[(BM, 128)], tile=(128, 128))            # eight k-tiles (the gate's limit): the look-ahead-2 kernel; 96 of 128 channels; M = 234
_case(RING, 1, 5, 3, 128, 512, knobs=[(BM, 128)], tile=(128, 128))                  # 16 k-tiles (the gate's floor), M = 15
_case(RING, 2, 13, 9, 256, 576, knobs=[(BM, 128)], tile=(128, 128))                 # 18 k-tiles, two column tiles, M = 234
# ---- stream-K inside streamk_scope: 64x128 tiles, >= 64 tiles, >= 8 k-tiles, tiles * k-tiles >= 6 * 768.  The gate forces M * Cin * K >= 64 * 128 * 32 * 4608,
# ---- so these two are the only cases above a few hundred thousand elements per tensor (about 1.2 and 2.1 million)
_case(STREAMK, 1, 32, 32, 1024, 1152, scope=True, tile=(64, 128))                   # 1x1: 128 tiles x 36 k-tiles = 4608 units
_case(STREAMK, 2, 64, 64, 256, 576, 3, 2, 1, scope=True, tile=(64, 128))            # 3x3/2: the four-tap phase has 64 tiles x 72 k-tiles and scatters; the other three stay whole-tile
# ---- Winograd F(2x2,3x3) data gradient: multiples of 16 that are no multiples of 32, odd planes and whole tiles
_case(WINO, 2, 5, 3, 48, 80, 3, 1, 1, halves=1)                                     # 12 tiles, fewer than one block; 48 output channels in two 32-halves
_case(WINO, 3, 13, 9, 16, 48, 3, 1, 1, halves=1)                                    # 105 tiles in four blocks; 16 output channels: one filter half, half empty
_case(WINO, 2, 8, 6, 80, 48, 3, 1, 1, halves=1)                                     # whole tiles
_case(WINO_2H, 2, 13, 9, 80, 48, 3, 1, 1, knobs=[(WINO_HALVES, 3)], halves=2)       # two halves per block (the floor of 400 blocks lifted): 80 of 128 channels
_case(WINO_2H, 2, 8, 6, 128, 16, 3, 1, 1, knobs=[(WINO_HALVES, 3)], halves=2)       # two halves, one 16-channel stage
# the persistent route wants a grid of whole rounds of 768 resident blocks, at least 90 % busy, with two periods of whole images per block: the smallest
# shape its gate admits has 2766 8x8 images of 16 channels (2.8 million elements).  One more image is the remainder the plain kernel takes
_case(WINO_PERSIST, 2767, 8, 8, 16, 16, 3, 1, 1, halves=1, persist_images=2766)


def case_id(case):
    c = case
    tail = "".join(f"-knob{k}={v}" for k, v in c.knobs) + ("-scope" if c.scope else "") + ("-direct" if c.via == "direct" else "")
    return f"{c.route}-{c.n}x{c.h}x{c.w}-{c.cout}" + (f"in{c.coutk}" if c.coutk != c.cout else "") + f"to{c.cin}-k{c.k}s{c.stride}p{c.pad}" + tail


def seed(case):
    return zlib.crc32(case_id(case).encode()) % 2 ** 31


def is_winograd(case):
    return case.route in (WINO, WINO_2H, WINO_PERSIST)


def out_size(case):
    return (case.h + 2 * case.pad - case.k) // case.stride + 1, (case.w + 2 * case.pad - case.k) // case.stride + 1


def _cdiv(a, b):
    return -(-a // b)


# ---- the launch logic, restated ---------------------------------------------------------------------------------------------------

def flipped_taps(r, s):
    """hip_train._flipped_taps: tap t of the data gradient's filter is element (r-1-i, s-1-j) of the conv's."""
    return [(r - 1 - i, s - 1 - j) for i in range(r) for j in range(s)]


PHASE_TAPS = {0: [1], 1: [2, 0]}      # 3x3 / stride 2 / pad 1, per input parity: dz row y + t meets filter row PHASE_TAPS[parity][t]


def launches(case):
    """The conv2d_fwd_ex launches hip_train._igemm_dgrad issues (for a Winograd case: the stride-1 launch that computes the same tensor)."""
    c = case
    ho, wo = out_size(c)
    if c.stride == 1:
        return [Launch(flipped_taps(c.k, c.k), c.k, c.k, c.k - 1 - c.pad, c.k - 1 - c.pad, c.h, c.w, 1, 1, 0, 0)]
    assert c.stride == 2 and c.h == 2 * ho and c.w == 2 * wo
    if c.k == 1:
        return [Launch([(0, 0)], 1, 1, 0, 0, ho, wo, 2, 2, 0, 0)]
    assert c.k == 3 and c.pad == 1
    return [Launch([(a, b) for a in PHASE_TAPS[py] for b in PHASE_TAPS[px]], len(PHASE_TAPS[py]), len(PHASE_TAPS[px]), 0, 0, ho, wo, 2, 2, py, px)
            for py in (0, 1) for px in (0, 1)]


def cout_pad(c):
    """vatl_conv_cout_pad: output channels rounded up to the column tile (32, 64 or 128 wide)."""
    bn = 32 if c <= 32 else (64 if c <= 64 else 128)
    return _cdiv(c, bn) * bn


def expect_dgrad_pack(w, taps, cout_k=None):
    """pack_dgrad_weight: (Cout,Cin,R,S) -> [CinPad][taps][CoutK], out[c][t][n] = w[n][c][taps[t]], zeros behind Cin and behind Cout."""
    cout, cin = w.shape[:2]
    out = np.zeros((cout_pad(cin), len(taps), cout_k or cout), w.dtype)
    for t, (r, s) in enumerate(taps):
        out[:cin, t, :cout] = w[:, :, r, s].T
    return out


def fwd_ex_model(x, wp, cout, L, out, residual=None):
    """conv2d_fwd_ex in float64 (stride 1 on the GEMM grid, as every data-gradient launch has it): pixel (oy, ox) of the Ho x Wo grid sums
    x[oy - pad_y + a][ox - pad_x + b] . wp[c][a*s + b] over the taps inside x, adds the residual READ AT THE SCATTERED POSITION and lands at
    (oy*osy + ooy, ox*osx + oox) of ``out`` (N, OH, OW, cout), which is modified in place and keeps every other element."""
    n, h, w, k = x.shape
    acc = torch.zeros((n, L.ho, L.wo, cout), dtype=torch.float64)
    for a in range(L.r):
        for b in range(L.s):
            y0, y1 = max(0, L.pad_y - a), min(L.ho, h + L.pad_y - a)
            x0, x1 = max(0, L.pad_x - b), min(L.wo, w + L.pad_x - b)
            if y1 > y0 and x1 > x0:
                acc[:, y0:y1, x0:x1] += x[:, y0 - L.pad_y + a:y1 - L.pad_y + a, x0 - L.pad_x + b:x1 - L.pad_x + b] @ wp[:cout, a * L.s + b, :].T
    view = out[:, L.ooy::L.osy, L.oox::L.osx]
    assert tuple(view.shape) == tuple(acc.shape), (view.shape, acc.shape)
    if residual is not None:
        acc = acc + residual[:, L.ooy::L.osy, L.oox::L.osx]
    view.copy_(acc)
    return out


def dgrad_model(case, dz, w, residual=None, only=None):
    """hip_train._igemm_dgrad on the host model, float64: the output starts as NaN (stride 1 and the four phases must write every pixel), as zeros
    or as a clone of the residual (1x1 / stride 2).  ``only``: indices of the launches to issue."""
    c = case
    x = torch.from_numpy(np.asarray(dz, np.float64))
    res = None if residual is None else torch.from_numpy(np.asarray(residual, np.float64))
    if c.stride == 2 and c.k == 1:
        out = torch.zeros((c.n, c.h, c.w, c.cin), dtype=torch.float64) if res is None else res.clone()
    else:
        out = torch.full((c.n, c.h, c.w, c.cin), float("nan"), dtype=torch.float64)
    for i, L in enumerate(launches(c)):
        if only is None or i in only:
            wp = torch.from_numpy(expect_dgrad_pack(np.asarray(w, np.float64), L.taps, c.coutk))
            fwd_ex_model(x, wp, c.cin, L, out, res)
    return out.numpy()


def _wino_persist_images(case, nb):
    """launch_wino_persist of csrc/conv_winograd.hip at its defaults (knobs 22 = 8, 24 = 2): -> (images the persistent launch covers, tiles per
    period).  Blocks of at most eight 16-channel stages; a period is lcm(tiles per image, 32) tiles; at least eight periods; the (group, filter
    tile) units of a period fit the resident blocks; the best cut into whole rounds keeps 90 % of the slots busy (95 % and eight periods per
    block from five stages on)."""
    c = case
    stages, tpi = c.cout // 16, _cdiv(c.h, 2) * _cdiv(c.w, 2)
    a, b = tpi, 32
    while b:
        a, b = b, a % b
    lt = tpi // a * 32
    pi, pg = lt // tpi, lt // 32
    periods = c.n // pi
    units, slots = pg * _cdiv(c.cin, 32 * nb), (512 if nb == 2 else 768)
    if stages > 8 or periods < 8 or pg > 4096 or units > slots:
        return 0, lt
    best_eff, best_chunk = 0.0, 0
    for k in range(1, 5):
        np_max = min(periods, k * slots // units)
        if np_max < 1:
            continue
        chunk = _cdiv(periods, np_max)
        if chunk < 2:
            break
        eff = periods * units / (_cdiv(_cdiv(periods, chunk) * units, slots) * slots * chunk)
        if eff > best_eff + 0.02:
            best_eff, best_chunk = eff, chunk
    if best_eff < 0.9 or (stages > 4 and (best_eff < 0.95 or best_chunk < 8)):
        return 0, lt
    return periods * pi, lt


def plan(case):
    """What dispatch() of csrc/conv_igemm.hip (tile_n_for, tile_m_for, streamk_wanted, persistent_wanted, ring_wanted) and winograd_impl of
    csrc/conv_winograd.hip do with the case's launches: -> dict(tile, var, routes, flops, launches = [(M, k-tiles, route)])."""
    c, knob = case, dict(KNOB_DEFAULTS)
    knob.update(dict(case.knobs))
    if is_winograd(c):
        nhp = 1 if c.cin <= 32 else 2
        pad = _cdiv(c.cin, 32 * nhp) * 32 * nhp

        def halves(n):                                                     # decided per launch, from its own block count
            mt = _cdiv(n * _cdiv(c.h, 2) * _cdiv(c.w, 2), 32)
            return 2 if nhp == 2 and pad % 64 == 0 and (knob[WINO_HALVES] == 3 or (knob[WINO_HALVES] == 2 and mt * _cdiv(c.cin, 64) >= 400)) else 1
        nb = halves(c.n)
        covered, lt = _wino_persist_images(c, nb)
        routes, flops = {}, 0.0
        if covered:
            routes[WINO_PERSIST] = 1
            flops += 2.0 * (covered // (lt // (_cdiv(c.h, 2) * _cdiv(c.w, 2))) * lt) * _cdiv(c.cin, 32 * nb) * 32 * nb * 16 * c.cout
        if covered < c.n:                                                  # the images that fill no period: the plain kernel
            nb = halves(c.n - covered)
            routes[WINO_2H if nb == 2 else WINO] = 1
            flops += 2.0 * _cdiv((c.n - covered) * _cdiv(c.h, 2) * _cdiv(c.w, 2), 32) * 32 * _cdiv(c.cin, 32 * nb) * 32 * nb * 16 * c.cout
        return dict(halves=nb, routes=routes, flops=flops, direct=False, persist_images=covered)
    bn = 32 if c.cin <= 32 else (64 if c.cin <= 64 else 128)
    n_tiles = cout_pad(c.cin) // bn
    routes, flops, out, tiles, var = Counter(), 0.0, [], set(), []
    for L in launches(c):
        m, kt = c.n * L.ho * L.wo, L.r * L.s * c.coutk // 32
        if bn < 64:
            bm = 128
        elif knob[BM] in (64, 128):
            bm = knob[BM]
        else:
            b128 = _cdiv(m, 128) * n_tiles
            bm = (128 if b128 >= 1536 else 64) if bn == 64 else (64 if b128 < 768 else 128)
        plain = (L.r, L.s, L.pad_y, L.pad_x, L.osy, L.osx) == (1, 1, 0, 0, 1, 1)
        t = _cdiv(m, 64) * n_tiles
        if c.scope and bn == 128 and bm == 64 and c.cin % 4 == 0 and kt >= 8 and t * 100 < _cdiv(t, 768) * 768 * 85 and t * kt >= 6 * 768 and t >= 64:
            route, bm = STREAMK, 64
        elif bm == 64:
            route = IGEMM
        elif bn == 128 and knob[VAR] == 4 and plain and c.cin % 4 == 0 and knob[PERSIST_K] and kt <= 8 * knob[PERSIST_K]:
            route = PERSISTENT
        elif bn == 128 and knob[VAR] == 4 and plain and c.cin == cout_pad(c.cin) and kt % 2 == 0 and kt >= 16:
            route = RING
        else:
            route = IGEMM
        routes[route] += 1
        flops += 2.0 * _cdiv(m, bm) * bm * n_tiles * bn * kt * 32
        tiles.add((bm, bn))
        var.append(0 if kt < 4 else 4)
        out.append((m, kt, route))
    assert len(tiles) == 1
    return dict(tile=tiles.pop(), var=var if bn == 32 else None, routes=dict(routes), flops=flops, launches=out, direct=True)


# ---- inputs, reference, bounds --------------------------------------------------------------------------------------------------------

def inputs(case, regime):
    """-> dz (N,Ho,Wo,CoutK) with zeros behind Cout, w (Cout,Cin,k,k), residual (N,H,W,Cin), float32.  "random": standard normal, the
    weights scaled by 1/sqrt(fan-in); "integer": integers in [-2, 2]."""
    c, r = case, np.random.RandomState(seed(case) ^ (0 if regime == "random" else 0x1234))
    ho, wo = out_size(c)
    shapes = ((c.n, ho, wo, c.coutk), (c.cout, c.cin, c.k, c.k), (c.n, c.h, c.w, c.cin))
    if regime == "integer":
        dz, w, res = (r.randint(-2, 3, s).astype(np.float32) for s in shapes)
    else:
        assert regime == "random"
        dz, w, res = (r.standard_normal(s).astype(np.float32) for s in shapes)
        w = (w / np.sqrt(c.cin * c.k * c.k)).astype(np.float32)
    dz[..., c.cout:] = 0
    return dz, w, res


def _nchw64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).transpose(0, 3, 1, 2)))


def reference(case, dz, w):
    """dx (N,H,W,Cin) in float64, without the residual: autograd of F.conv2d on the host.  Only the Cout valid channels of dz enter."""
    c = case
    x = torch.zeros((c.n, c.cin, c.h, c.w), dtype=torch.float64, requires_grad=True)
    F.conv2d(x, torch.from_numpy(np.asarray(w, np.float64)), None, c.stride, c.pad).backward(_nchw64(dz[..., :c.cout]))
    return np.ascontiguousarray(x.grad.permute(0, 2, 3, 1).numpy())


def abs_sum(case, dz, w, residual=None):
    """S = the sum of the absolute terms of every element of dx: conv_transpose2d(|dz|, |w|) (+ |residual|)."""
    c = case
    opad = ((c.h + 2 * c.pad - c.k) % c.stride, (c.w + 2 * c.pad - c.k) % c.stride)
    s = F.conv_transpose2d(_nchw64(np.abs(dz[..., :c.cout])), torch.from_numpy(np.abs(np.asarray(w, np.float64))), None, c.stride, c.pad, output_padding=opad)
    s = np.ascontiguousarray(s.permute(0, 2, 3, 1).numpy())
    return s if residual is None else s + np.abs(np.asarray(residual, np.float64))


U = 2.0 ** -24


def elementwise_bound(case, s):
    """2 * gamma_n * S with n = K + 1: K = k * k * Cout rounded products summed in any order (stream-K's slabs are one such order), then the
    residual's addition; the factor 2 covers the matrix core pairing two products per step (as wgrad_cases.elementwise_bound)."""
    n = case.k * case.k * case.cout + 1
    return 2.0 * (n * U / (1.0 - n * U)) * s


def exact_headroom(case):
    """The largest possible partial sum of the integer regime, which must stay below 2^24.  Direct kernels: K products of at most 4 and the
    residual.  F(2x2,3x3): the data transform (+-1, four terms) gives at most 8, the filter transform (halves) at most 9/4 * 2 in multiples of
    1/4, so a transform-domain sum is a multiple of 1/4 below 36 * Cout and 16 * 36 * Cout bounds it in units of 1/4 with the output transform."""
    return 16 * 36 * case.cout if is_winograd(case) else 4 * case.k * case.k * case.cout + 2


# ---- impulses -----------------------------------------------------------------------------------------------------------------------------

def impulse_sites(case):
    """[(image, channel, oy, ox)]: the four corners, the middle of each edge and one interior pixel of dz, in the first and the last image,
    at the first and the last channel."""
    ho, wo = out_size(case)
    px = [(0, 0), (0, wo - 1), (ho - 1, 0), (ho - 1, wo - 1), (0, wo // 2), (ho - 1, wo // 2), (ho // 2, 0), (ho // 2, wo - 1), (ho // 2, wo // 2)]
    px = list(dict.fromkeys(px))
    return [(b, ch, oy, ox) for b in sorted({0, case.n - 1}) for ch in sorted({0, case.cout - 1}) for oy, ox in px]


def impulse_footprint(case, oy, ox):
    """[((iy, ix), (r, s))]: dz = 1.0 at pixel (oy, ox) of channel n makes dx[iy][ix][:] a copy of w[n, :, r, s]; taps outside dx are dropped."""
    c = case
    spots = [((oy * c.stride - c.pad + r, ox * c.stride - c.pad + s), (r, s)) for r in range(c.k) for s in range(c.k)]
    return [(p, t) for p, t in spots if 0 <= p[0] < c.h and 0 <= p[1] < c.w]


def impulse_weights(case):
    c = case
    return np.random.RandomState(seed(case) ^ 0x5A5A).standard_normal((c.cout, c.cin, c.k, c.k)).astype(np.float32)


def impulse_dz(case, site):
    ho, wo = out_size(case)
    dz = np.zeros((case.n, ho, wo, case.coutk), np.float32)
    b, ch, oy, ox = site
    dz[b, oy, ox, ch] = 1.0
    return dz


def impulse_expectation(case, site, w):
    """dx (N,H,W,Cin) of the impulse at ``site``: zeros and copies of filter elements."""
    b, ch, oy, ox = site
    dx = np.zeros((case.n, case.h, case.w, case.cin), np.float64)
    for (iy, ix), (r, s) in impulse_footprint(case, oy, ox):
        dx[b, iy, ix, :] = w[ch, :, r, s]
    return dx
