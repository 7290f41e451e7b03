"""Inputs and case list of the glue-kernel bit fixture (tests/golden/glue_bits.npz): what tools/make_scorer_bits.py records from the parent
commit's library (``--cases tests.glue_cases``) and tests/test_gpu_scorer_bits.py replays.  Same protocol as tests/scorer_cases.py: inputs
are regenerated from the seeds, never stored; nothing here imports the library.  The kernels are the HBM-bound passes around the
convolutions: csrc/layout.hip, pool.hip, fusion.hip, pack.hip (bn_fold) and bn_train.hip.

Shapes are the smallest that reach each kernel and branch:
  max-pool        2 x 7 x 5 (odd: the last window row / column is cut by the border) and 2 x 8 x 6, C = 8 (float4 kernels) and C = 6 (scalar
                  kernels); channel c holds a random plane (c % 3 == 0), an all-negative one (1) or one quantised to four levels (2), so that
                  windows hold exact ties and the first-maximum rule decides
  hw_reduce       C = 32 gives cols = 8 and 32 pixels per sweep: 70 pixels run the tail loop only, 200 the four-deep main loop and the tail;
                  N = 256, HW = 64, C = 128 is the smallest batch that widens a block to cols = 16
  BatchNorm       M = 2 x 9 x 7 with C = 8 (one row block); C = 64 with M = 2 x 192 x 172 = 66048 rows, which row_split() below cuts into 258
                  row blocks: more than one, and more than the 256 partials one sweep of the finalize kernels takes
  bn_bwd_from_stats  fed by a 1x1, 32 -> 32 channel conv2d_fwd_ex_bnbwd launch over 2 x 4 x 3 pixels (Cin % 32 == 0 is that route's floor)
Outputs of more than 65536 words (the element-wise passes at the large BatchNorm size) are stored as their SHA-256.
"""
import functools
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glue_bits.npz")
DIGEST_ABOVE = 65536
BN_SIZES = {"small": ((2, 9, 7), 8), "large": ((2, 192, 172), 64)}


def row_split(m, c):
    """csrc/bn_train.hip's row_split(), restated: -> (rows per block, row blocks)."""
    c4 = max(c >> 2, 1)
    cols = min(c4, 256)
    rstep, gy = 256 // cols, (c4 + 255) // 256
    rpb, want = 256, max(1024 // gy, 1)
    if (m + rpb - 1) // rpb < want:
        rpb = max((m + want - 1) // want, 16 * rstep)
        rpb = (rpb + rstep - 1) // rstep * rstep
    nrb = (m + rpb - 1) // rpb
    if nrb > 4096:
        rpb = (m + 4095) // 4096
    return rpb, (m + rpb - 1) // rpb


assert row_split(2 * 9 * 7, 8)[1] == 1 and row_split(2 * 192 * 172, 64)[1] == 258


def _rand(seed, *shape):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def _put(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def pool_input(h, w, c, seed):
    x = _rand(seed, 2, h, w, c)
    for k in range(c):
        if k % 3 == 1:
            x[..., k] = -np.abs(x[..., k]) - 0.25
        elif k % 3 == 2:
            x[..., k] = np.round(x[..., k] * 1.5) / 2.0
    return x


def _pool_shapes(h, w, c):
    return pool_input(h, w, c, seed=100 * h + 10 * w + c), ((h - 1) // 2 + 1, (w - 1) // 2 + 1)


def _nchw_to_nhwc(vh, c, cpad):
    return (vh.nchw_to_nhwc(_put(_rand(c, 2, c, 5, 3)), cpad),)


def _nhwc_to_nchw(vh):
    return (vh.nhwc_to_nchw(_put(_rand(1, 2, 5, 3, 6))),)


def _shuffles(vh):
    return vh.pixelshuffle2_fwd(_put(_rand(2, 2, 3, 5, 16))), vh.pixelunshuffle2(_put(_rand(3, 2, 6, 10, 4)))


def _pool_fwd(vh, h, w):
    return (vh.maxpool3x3s2_fwd(_put(_pool_shapes(h, w, 8)[0])),)


def _pool_fwd_idx(vh, h, w, c):
    return vh.maxpool3x3s2_fwd_idx(_put(_pool_shapes(h, w, c)[0]))


def _pool_fwd_idx_affine(vh, h, w):
    scale = np.array([1.5, -0.75, 1.0, 0.5, -2.0, 0.25, 1.25, 3.0], np.float32)
    return vh.maxpool3x3s2_fwd_idx_affine(_put(_pool_shapes(h, w, 8)[0]), _put(scale), _put(_rand(5, 8) * 0.5))


def _pool_bwd(vh, h, w, c):
    x, (ho, wo) = _pool_shapes(h, w, c)
    return (vh.maxpool3x3s2_bwd(_put(x), _put(_rand(6, 2, ho, wo, c))),)


def _pool_bwd_idx(vh, h, w, c):
    x, (ho, wo) = _pool_shapes(h, w, c)
    _, idx = vh.maxpool3x3s2_fwd_idx(_put(x))
    return (vh.maxpool3x3s2_bwd_idx(_put(_rand(7, 2, ho, wo, c)), idx, (h, w)),)


GAP_SHAPES = {"thread": (2, 4, 3, 8), "tail": (2, 10, 7, 32), "main": (2, 20, 10, 32), "cols16": (256, 8, 8, 128)}


def _gap_fwd(vh, which):
    return (vh.gap_fwd(_put(_rand(8, *GAP_SHAPES[which]))),)


def _gap_bwd(vh):
    return (vh.gap_bwd(_put(_rand(9, 2, 8)), 12),)


def _se_bwd_gate(vh, which):
    s = GAP_SHAPES[which]
    return (vh.se_bwd_gate(_put(_rand(10, *s)), _put(_rand(11, *s)), _put(_rand(12, *s)), _put(_rand(13, s[0], s[3]))),)


def _se_bwd_apply(vh):
    s = GAP_SHAPES["thread"]
    return vh.se_bwd_apply(_put(_rand(14, *s)), _put(_rand(15, *s)), _put(_rand(16, s[0], s[3])), _put(_rand(17, s[0], s[3])))


def _se_scale_add_relu(vh):
    s = GAP_SHAPES["thread"]
    return (vh.se_scale_add_relu(_put(_rand(18, *s)), _put(_rand(19, s[0], s[3])), _put(_rand(20, *s))),)


def _fuse(vh, sources, relu):
    ups = [(_put(_rand(22 + k, 2, 8 >> (k + 1), 8 >> (k + 1), 8)), k + 1) for k in range(sources)]
    return (vh.fuse_upsample_add(_put(_rand(21, 2, 8, 8, 8)), ups, relu),)


def _upsample_bwd(vh, shift, mask):
    return (vh.upsample_nearest_bwd(_put(_rand(25, 2, 8, 8, 8)), _put(_rand(26, 2, 8, 8, 8)) if mask else None, shift),)


def _relu_bwd(vh):
    return (vh.relu_bwd(_put(_rand(27, 1027)), _put(_rand(28, 1027))),)


def _bn_fold(vh, stats, conv_bias):
    gamma, beta, mean, var = (_put(a) for a in (_rand(29, 8) + 1.0, _rand(30, 8), _rand(31, 8), np.abs(_rand(32, 8)) + 0.5))
    cb = _put(_rand(33, 8)) if conv_bias else None
    return vh.bn_fold(gamma, beta, mean, var, 1e-5, cb) if stats else vh.bn_fold(None, None, None, None, 1e-5, cb)


@functools.lru_cache(maxsize=None)
def bn_host(size):
    """Host tensors of one BatchNorm size: z, dy, res, gamma, beta, the batch statistics and folded (scale, bias) in float32, and
    y = relu(z * scale + bias + res).  Fixed inputs only: they need not be what the library's forward would have produced."""
    (n, h, w), c = BN_SIZES[size]
    z = _rand(40, n, h, w, c) * 2.0 + 0.5
    dy, res = _rand(41, n, h, w, c), _rand(42, n, h, w, c)
    gamma, beta = (_rand(43, c) * 0.25 + 1.0), _rand(44, c) * 0.1
    z2 = z.reshape(-1, c).astype(np.float64)
    mean, var = z2.mean(0), z2.var(0)
    invstd = 1.0 / np.sqrt(var + 1e-5)
    scale = (gamma * invstd).astype(np.float32)
    bias = (beta - mean * gamma * invstd).astype(np.float32)
    y = np.maximum(z * scale + bias + res, 0.0).astype(np.float32)
    return dict(z=z, dy=dy, res=res, gamma=gamma, beta=beta, mean=mean.astype(np.float32), invstd=invstd.astype(np.float32), scale=scale, bias=bias, y=y)


def _bn(size, *keys):
    h = bn_host(size)
    return [_put(h[k]) for k in keys]


def _bn_fwd_stats(vh, size, running):
    z, gamma, beta = _bn(size, "z", "gamma", "beta")
    c = z.shape[-1]
    rm, rv = (_put(_rand(45, c) * 0.1), _put(np.abs(_rand(46, c)) + 0.5)) if running else (None, None)
    outs = vh.bn_train_fwd_stats(z, gamma, beta, rm, rv, 0.1, 1e-5)
    return tuple(outs) + ((rm, rv) if running else ())


def _scale_bias_act(vh, size, residual, relu):
    z, scale, bias, res = _bn(size, "z", "scale", "bias", "res")
    return (vh.scale_bias_act(z, scale, bias, res if residual else None, relu),)


def _bn_bwd(vh, size, mask, want_g):
    dy, y, z, gamma, mean, invstd = _bn(size, "dy", "y", "z", "gamma", "mean", "invstd")
    dz, g, dgamma, dbeta = vh.bn_train_bwd(dy, y if mask else None, z, gamma, mean, invstd, want_g=want_g)
    return (dz, dgamma, dbeta) + ((g,) if want_g else ())


def _bn_bwd_relu(vh, size):
    dy, scale, bias, z, gamma, mean, invstd = _bn(size, "dy", "scale", "bias", "z", "gamma", "mean", "invstd")
    return vh.bn_train_bwd_relu(dy, scale, bias, z, gamma, mean, invstd)


def _bn_bwd_from_stats(vh):
    c = 32
    x, w = _put(_rand(50, 2, 4, 3, c)), _put(_rand(51, c, c, 1, 1) * 0.2)
    z = _rand(52, 2, 4, 3, c)
    z2 = z.reshape(-1, c).astype(np.float64)
    mean, invstd = z2.mean(0).astype(np.float32), (1.0 / np.sqrt(z2.var(0) + 1e-5)).astype(np.float32)
    spec = vh.BnBwdSpec(_put(z), _put(mean), _put(invstd), scale=_put(_rand(53, c) * 0.25 + 1.0), bias=_put(_rand(54, c) * 0.1))
    g = vh.conv2d_fwd_ex_bnbwd(x, vh.pack_conv_weight(w), c, 1, 1, 1, 0, 0, 4, 3, 4, 3, 1, 1, 0, 0, spec)
    return vh.bn_bwd_from_stats(spec, g, _put(_rand(55, c) * 0.25 + 1.0))


def _bn_bwd_relu_pool(vh):
    h, w, c = 8, 6, 8
    z = _put(pool_input(h, w, c, seed=60))
    scale, bias, gamma, mean, invstd = (_put(a) for a in (_rand(61, c) * 0.5 + 1.0, _rand(62, c) * 0.3, _rand(63, c) * 0.25 + 1.0, _rand(64, c) * 0.1,
                                                            np.abs(_rand(65, c)) + 0.5))
    _, idx = vh.maxpool3x3s2_fwd_idx_affine(z, scale, bias)
    return vh.bn_train_bwd_relu_pool(_put(_rand(66, 2, 4, 3, c)), idx, scale, bias, z, gamma, mean, invstd)


def _col_sum(vh, c):
    return (vh.col_sum(_put(_rand(70 + c, 2 * 9 * 7, c))),)


def _case(fn, *args):
    return lambda vh: fn(vh, *args)


CASES = {}
for _c, _cpad in ((3, 4), (17, 32), (5, 5)):
    CASES[f"nchw_to_nhwc_c{_c}_{_cpad}"] = _case(_nchw_to_nhwc, _c, _cpad)
CASES["nhwc_to_nchw"] = _nhwc_to_nchw
CASES["pixelshuffle2_and_inverse"] = _shuffles
for _h, _w in ((7, 5), (8, 6)):
    CASES[f"maxpool_fwd_{_h}x{_w}_c8"] = _case(_pool_fwd, _h, _w)
    CASES[f"maxpool_fwd_idx_affine_{_h}x{_w}_c8"] = _case(_pool_fwd_idx_affine, _h, _w)
    for _c in (8, 6):
        CASES[f"maxpool_fwd_idx_{_h}x{_w}_c{_c}"] = _case(_pool_fwd_idx, _h, _w, _c)
        CASES[f"maxpool_bwd_{_h}x{_w}_c{_c}"] = _case(_pool_bwd, _h, _w, _c)
        CASES[f"maxpool_bwd_idx_{_h}x{_w}_c{_c}"] = _case(_pool_bwd_idx, _h, _w, _c)
for _which in GAP_SHAPES:
    CASES[f"gap_fwd_{_which}"] = _case(_gap_fwd, _which)
CASES["gap_bwd"] = _gap_bwd
for _which in ("thread", "tail", "main"):
    CASES[f"se_bwd_gate_{_which}"] = _case(_se_bwd_gate, _which)
CASES["se_bwd_apply"] = _se_bwd_apply
CASES["se_scale_add_relu"] = _se_scale_add_relu
for _k in (1, 2, 3):
    for _relu in (False, True):
        CASES[f"fuse_upsample_add_{_k}" + ("_relu" if _relu else "")] = _case(_fuse, _k, _relu)
for _shift in (1, 2):
    for _mask in (False, True):
        CASES[f"upsample_nearest_bwd_s{_shift}" + ("_mask" if _mask else "")] = _case(_upsample_bwd, _shift, _mask)
CASES["relu_bwd_1027"] = _relu_bwd
for _stats, _cb, _tag in ((True, False, "stats"), (False, True, "conv_bias"), (True, True, "both")):
    CASES[f"bn_fold_{_tag}"] = _case(_bn_fold, _stats, _cb)
for _size in BN_SIZES:
    for _running in (False, True):
        CASES[f"bn_fwd_stats_{_size}" + ("_running" if _running else "")] = _case(_bn_fwd_stats, _size, _running)
    for _res, _relu in ((False, False), (False, True), (True, True)):
        CASES[f"scale_bias_act_{_size}" + ("_res" if _res else "") + ("_relu" if _relu else "")] = _case(_scale_bias_act, _size, _res, _relu)
    for _mask, _g, _tag in ((True, False, "ymask"), (False, False, "nomask"), (True, True, "ymask_g")):
        CASES[f"bn_bwd_{_size}_{_tag}"] = _case(_bn_bwd, _size, _mask, _g)
    CASES[f"bn_bwd_relu_{_size}"] = _case(_bn_bwd_relu, _size)
CASES["bn_bwd_from_stats"] = _bn_bwd_from_stats
CASES["bn_bwd_relu_pool_8x6"] = _bn_bwd_relu_pool
for _c in (32, 17):
    CASES[f"col_sum_c{_c}"] = _case(_col_sum, _c)


def bits(t):
    """A device tensor as the fixture stores it: float32 / float64 as uint32 / uint64 bit patterns, the pool's tap bytes raw; anything
    over DIGEST_ABOVE words as the eight uint32 words of the SHA-256 of those bits."""
    a = t.detach().cpu().numpy()
    a = a.view({4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == "f" else a
    if a.size > DIGEST_ABOVE:
        return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint32).copy()
    return a


def run(vh, name):
    """-> {fixture key: bits} of one case: its outputs in the order the case returns them."""
    import torch
    outs = CASES[name](vh)
    torch.cuda.synchronize()
    return {f"{name}.{k}": bits(t) for k, t in enumerate(outs)}
