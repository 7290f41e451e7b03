"""Inputs and case list of the scorer bit fixture (tests/golden/scorer_bits.npz): what tools/make_scorer_bits.py records from the parent
commit's library and tests/test_gpu_scorer_bits.py replays.  Inputs are regenerated from the seeds, never stored; nothing here imports
the library: every case takes the ``vatl_hip`` module as an argument.

Heat-map tensors are (5, 17, H, W): 85 planes = 21 full four-wave blocks and one partial one on the wave-per-plane routes.  Plane sizes
are the smallest at which each kernel and branch is reached:
  64x48, 96x72   wave-per-plane routes (NV = 12 / 27), register local-peak kernel, peaks5 wave kernel (64x48, min_distance 5)
  the same 64x48 on a view one float into its storage: not 16-byte aligned, so every entry takes its block kernel
  32x24          block kernels with float4 loads
  7x5 / 10x7     block kernels with scalar loads (H * W odd / not a multiple of 4)
  16x8           register local-peak kernel with two row groups per wave; on the unaligned view the LDS-tile kernel
  5x260          LDS-tile local-peak kernel (65 float4 columns: more than a wave holds)
  5x4            W % 4 == 0 on an aligned base, so localpeak_mean takes the register kernel; 4x5, 7x5, 24x18: the generic kernel
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scorer_bits.npz")
N, J = 5, 17


def heatmaps(h, w, seed, n=N, j=J):
    """(n, j, h, w) float32 in [0, 1) with planted planes 0..12 (flat plane index = item * j + joint)."""
    r = np.random.RandomState(seed)
    hm = r.random_sample((n, j, h, w)).astype(np.float32)
    p, flat, hw = hm.reshape(n * j, h, w), hm.reshape(n * j, h * w), h * w
    p[0] = 0.25                                                    # constant
    p[1] = -p[1] - 0.1                                             # all negative
    flat[2, [hw // 3, 2 * hw // 3]] = 2.0                          # two exactly equal maxima
    p[3, 0, w - 1] = 3.0                                           # maximum on the border
    p[4, h // 2, w // 2] = 3.0                                     # maximum in the interior (quarter-pixel shift)
    flat[5, [1, hw - 2]] = np.nan                                  # NaN at two positions: the first is the arg-max
    flat[6, hw // 2] = np.inf
    flat[7] = np.where(np.arange(hw) % 2 == 0, 0.5, -0.5)          # sums to exactly zero
    if hw % 2:
        flat[7, -1] = 0.0
    flat[8, hw // 4] = -0.125                                      # one negative entry
    p[9] *= 0.01                                                   # more than five well-spaced peaks of distinct heights
    for k, (y, x) in enumerate((y, x) for y in range(6, h - 6, 7) for x in range(6, w - 6, 7)):
        p[9, y, x] = 1.0 + 0.03125 * k
    p[10] = 0.0                                                    # plateau: every pixel inside the outer ring is a candidate
    p[10, 1:h - 1, 1:w - 1] = 1.0
    if h >= 20 and w >= 20:                                        # plateau of 81 equal candidates (more than a wave's 64, fewer than 256)
        p[11] *= 0.01
        p[11, 6:15, 6:15] = 1.0
    p[12] = -p[12]                                                 # maximum exactly 0: the decoders zero its coordinates
    p[12, 0, 0] = 0.0
    return hm


def bboxes(n=N):
    w = np.linspace(60.0, 240.0, n) + 0.37
    return np.stack([np.full(n, 100.25), np.full(n, 50.5), 100.25 + w, 50.5 + w * 4.0 / 3.0], 1).astype(np.float32)


def ae_weights(d, z, seed):
    """Flat WholeBodyAE parameters in vatl_pack_ae order: (W, b) of D-24-12-7-z-7-12-24-D."""
    dims = [d, 24, 12, 7, z, 7, 12, 24, d]
    r = np.random.RandomState(seed)
    return (0.4 * r.standard_normal(sum(o * i + o for i, o in zip(dims[:-1], dims[1:])))).astype(np.float32)


def poses(seed, n=6):
    """(n, 17, 3) float32 key-points and crop boxes (n, 4) xyxy; item n-2 has box height 0 (status 1), item n-1 no score weight (status 2)."""
    r = np.random.RandomState(seed)
    k = np.concatenate([r.uniform(100, 300, (n, 17, 2)), r.uniform(0.05, 1.0, (n, 17, 1))], 2).astype(np.float32)
    b = bboxes(n)
    b[n - 2, 3] = b[n - 2, 1] - 1.0
    k[n - 1, :, 2] = 0.0
    return k, b


def _put(a, unaligned=False):
    """Device copy of ``a``; ``unaligned``: a contiguous view one element into its storage (base 4 or 8 bytes past a 16-byte boundary)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not unaligned:
        return t.to("cuda:0")
    holder = torch.zeros(t.numel() + 4, dtype=t.dtype, device="cuda:0")
    view = holder[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


HM_SIZES = {"64x48": (64, 48, False), "96x72": (96, 72, False), "32x24": (32, 24, False), "7x5": (7, 5, False), "10x7": (10, 7, False),
            "64x48u": (64, 48, True), "16x8": (16, 8, False), "16x8u": (16, 8, True), "5x260": (5, 260, False), "5x4": (5, 4, False),
            "4x5": (4, 5, False), "24x18": (24, 18, False), "12x11": (12, 11, False), "8x6": (8, 6, False)}


def _hm(size):
    h, w, unaligned = HM_SIZES[size]
    return _put(heatmaps(h, w, seed=1000 + 7 * h + w), unaligned)


# stream flags of five items: every (is_prev, is_next) pattern an item can see, exactly one neighbour included (the ends ignore their outer flag)
FLAGS = {"all": ([1, 1, 1, 1, 1], [1, 1, 1, 1, 1]), "mixed": ([1, 1, 0, 0, 1], [1, 0, 1, 0, 1]), "none": ([0, 0, 0, 0, 0], [0, 0, 0, 0, 0])}


def _flags(which, n):
    ip, inx = FLAGS[which]
    return _put(np.array(ip[:n], np.uint8)), _put(np.array(inx[:n], np.uint8))


def _decode(vh, size):
    return vh.decode(_hm(size), _put(bboxes()))


def _decode_pose(vh, size):
    return vh.decode_pose(_hm(size), _put(bboxes()))


def _decode_pose_j136(vh):
    """J = 136 > 128: both halves of NumPy's pairwise sum."""
    return vh.decode_pose(_put(heatmaps(7, 5, seed=136, n=2, j=136)), _put(bboxes(2)))


def _softargmax(vh, size, norm):
    return vh.decode_softargmax(_hm(size), _put(bboxes()), norm)


def _entropy(vh, size):
    return (vh.plane_entropy(_hm(size)),)


def _localpeak(vh, size, order):
    hm = _hm(size)
    mean, cnt = vh.localpeak_mean(hm, order)
    return mean, cnt, vh.localpeak_mask(hm, order)


def _peaks5(vh, size, md):
    return vh.peaks5(_hm(size), md)


def _thc_pairs(vh, size, norm):
    hm = _hm(size)
    return (vh.thc_pairs(hm[:-1], hm[1:], norm),)


def _thc_stream(vh, n, which):
    return (vh.thc_stream(_hm("8x6")[:n].contiguous(), *_flags(which, n), "L1"),)


def _tpc_stream(vh, n, which):
    hm, bb = _hm("32x24")[:n].contiguous(), _put(bboxes()[:n])
    return (vh.tpc_stream(hm, bb, vh.decode(hm, bb)[0], *_flags(which, n)),)


def _wpu(vh, d, z, only38):
    k, b = poses(seed=42)
    return vh.hybrid_ae_wpu(_put(k), _put(b), _put(ae_weights(d, z, seed=d + z)), d, z, only38)


def _ae_forward(vh, d):
    feat = np.random.RandomState(d).random_sample((6, d)).astype(np.float32)
    return vh.ae_forward(_put(feat), _put(ae_weights(d, 5, seed=d)), d, 5, True)


def _hybrid_f64(vh):
    k, _ = poses(seed=43)
    box = np.tile(np.array([100.0, 50.0, 80.5, 160.25]), (6, 1))
    box[4, 3] = 0.0
    k64 = k.astype(np.float64)
    k64[:, :, :2] += 0.001                                         # coordinates that are no float32 values
    return vh.hybrid_feature_f64(_put(k64.reshape(6, 51)), _put(box))


def _oks(vh):
    """Item 3 has no visible joint: the box-distance form."""
    r = np.random.RandomState(44)
    k, _ = poses(seed=44)
    gt = k.astype(np.float64) + r.uniform(-6, 6, k.shape)
    gt[:, :, 2] = (r.random_sample((6, 17)) > 0.3).astype(np.float64)
    gt[3, :, 2] = 0.0
    box = np.stack([np.full(6, 100.0), np.full(6, 100.0), np.linspace(60, 200, 6), np.linspace(90, 260, 6)], 1)
    return (vh.oks(_put(k), _put(gt.reshape(6, 51)), _put(box)),)


def _case(fn, *args):
    return lambda vh: fn(vh, *args)


CASES = {}
for _s in ("64x48", "96x72", "32x24", "7x5", "64x48u"):
    CASES[f"decode_{_s}"] = _case(_decode, _s)
    CASES[f"decode_pose_{_s}"] = _case(_decode_pose, _s)
CASES["decode_pose_j136"] = _decode_pose_j136
for _s in ("64x48", "96x72", "32x24", "10x7", "64x48u"):
    for _norm in ("softmax", "sigmoid", "divide_sum"):
        CASES[f"softargmax_{_norm}_{_s}"] = _case(_softargmax, _s, _norm)
    CASES[f"entropy_{_s}"] = _case(_entropy, _s)
for _s in ("64x48", "96x72", "16x8", "16x8u", "5x260", "5x4", "4x5", "7x5", "24x18"):
    for _order in (0.5, 0.9):
        CASES[f"localpeak_{_s}_{_order}"] = _case(_localpeak, _s, _order)
for _s, _md in (("64x48", 5), ("64x48", 3), ("64x48u", 5), ("32x24", 5), ("12x11", 5)):
    CASES[f"peaks5_{_s}_md{_md}"] = _case(_peaks5, _s, _md)
for _s in ("64x48", "8x6"):
    for _norm in ("L1", "L2"):
        CASES[f"thc_pairs_{_norm}_{_s}"] = _case(_thc_pairs, _s, _norm)
for _n, _which in ((5, "all"), (5, "mixed"), (5, "none"), (1, "all")):
    CASES[f"thc_stream_n{_n}_{_which}"] = _case(_thc_stream, _n, _which)
    CASES[f"tpc_stream_n{_n}_{_which}"] = _case(_tpc_stream, _n, _which)
for _d, _z, _only38 in ((42, 5, False), (38, 5, False), (42, 5, True), (42, 1, False)):
    CASES[f"wpu_d{_d}_z{_z}" + ("_only38" if _only38 else "")] = _case(_wpu, _d, _z, _only38)
for _d in (38, 42, 64):
    CASES[f"ae_forward_d{_d}"] = _case(_ae_forward, _d)
CASES["hybrid_feature_f64"] = _hybrid_f64
CASES["oks"] = _oks


def bits(t):
    """A device tensor as the fixture stores it: float32 / float64 as uint32 / uint64 bit patterns, masks (uint8) as packed bits, integers raw."""
    a = t.detach().cpu().numpy()
    if a.dtype == np.uint8:
        return np.packbits(a.reshape(-1))
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == "f" else a


def run(vh, name):
    """-> {fixture key: bits} of one case: its outputs in the order the wrapper returns them."""
    import torch
    outs = CASES[name](vh)
    torch.cuda.synchronize()
    return {f"{name}.{k}": bits(t) for k, t in enumerate(outs)}
