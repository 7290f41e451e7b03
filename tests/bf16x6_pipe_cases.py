"""Cases, inputs and launches shared by tests/test_gpu_gemm1x1_bf16x6_pipe.py and tools/make_bf16x6_bits.py: the three forms of the bf16x6 GEMM
(csrc/gemm1x1_bf16x6.hip) at the places where its software-pipelined k-loop can go wrong — the first stages, the last three, the dual crossing from x to
x2, partial tiles.  No GPU is needed to import this module or to build the inputs."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bf16x6_parent_bits.npz")

# rows M = n H W: one row | a partial tile | a whole tile | a tile and one row | a tile and a tail of 16
ROWS = ((1, 1, 1), (1, 8, 6), (1, 16, 8), (1, 43, 3), (3, 8, 6))
# form -> (K1, K2, N): short: 8 stages (prologue and tail are the whole loop), 12, 28; long: 32 and 36 stages, one and two n-tiles; dual: the crossing
# right behind the prologue (stage 4 of 24), right in front of the tail (stage 20 of 24) and in the middle
SHAPES = {"short": ((128, 0, 512), (192, 0, 512), (448, 0, 512)),
          "long": ((512, 0, 128), (576, 0, 256)),
          "dual": ((64, 320, 128), (320, 64, 128), (128, 256, 256))}
ROUTE = {"short": "gemm1x1_bf16x6_short", "long": "gemm1x1_bf16x6", "dual": "gemm1x1_bf16x6"}


def _cases():
    """Every (shape, rows) pair of every form; residual and ReLU cycle so that each of their values meets every shape and every row count of the form
    (the dual form takes no residual)."""
    out = []
    for form, shapes in SHAPES.items():
        for si, (k1, k2, n) in enumerate(shapes):
            for ri, rows in enumerate(ROWS):
                q = si + ri
                res = form != "dual" and q % 2 == 0
                relu = (q // 2 + si) % 2 == 0
                out.append((form, k1, k2, n, rows, res, relu))
                if form != "dual" and ri in (1, 4):      # both residual states on the partial-tile and the tile-and-tail rows
                    out.append((form, k1, k2, n, rows, not res, not relu))
    return tuple(out)


CASES = _cases()
# the cases whose bits the parent commit's library recorded (tools/make_bf16x6_bits.py)
BITS = tuple(c for c in CASES if (c[0], c[1], c[4]) in (("short", 128, (3, 8, 6)), ("short", 192, (1, 43, 3)), ("short", 448, (1, 8, 6)),
                                                       ("long", 512, (3, 8, 6)), ("long", 576, (1, 43, 3)),
                                                       ("dual", 64, (3, 8, 6)), ("dual", 320, (1, 43, 3)), ("dual", 128, (1, 16, 8))))


def case_id(c):
    form, k1, k2, n, (b, h, w), res, relu = c
    return f"{form}_{k1}" + (f"+{k2}" if k2 else "") + f"_{n}_m{b * h * w}" + ("_res" if res else "") + ("" if relu else "_norelu")


def _seed(c):
    form, k1, k2, n, (b, h, w), res, relu = c
    return (k1 * 7 + k2 * 3 + n + 131 * b * h * w + 2 * res + relu) % (2 ** 31)


def inputs(c, integers):
    """dict of float32 arrays: a (b,h,w,K1), x2 (b,2h,2w,K2) for the dual form (projection stride 2), w1 / w2 [N][K], scale (None for the dual form and for
    the integer data: scale 1), bias, residual or None.  integers: every value an integer of magnitude <= 8, every k different."""
    form, k1, k2, n, (b, h, w), res, relu = c
    r = np.random.RandomState(_seed(c) + (1 << 20) * integers)
    if integers:
        draw = lambda *s: r.randint(-8, 9, s).astype(np.float32)
        wdraw = lambda k: draw(n, k)
    else:
        draw = lambda *s: r.standard_normal(s).astype(np.float32)
        wdraw = lambda k: (r.standard_normal((n, k)) / np.sqrt(k1 + k2)).astype(np.float32)
    d = {"a": draw(b, h, w, k1), "w1": wdraw(k1), "bias": draw(n), "scale": None, "x2": None, "w2": None, "res": None}
    if form == "dual":
        d["x2"], d["w2"] = draw(b, 2 * h, 2 * w, k2), wdraw(k2)
    elif not integers:
        d["scale"] = r.uniform(0.5, 1.5, n).astype(np.float32)
    if res:
        d["res"] = draw(b, h, w, n)
    return d


def reference(c, d, dtype):
    """The layer in `dtype` (np.int64 on the integer data, np.float64 otherwise), rows x N."""
    form, k1, k2, n, (b, h, w), res, relu = c
    y = d["a"].astype(dtype).reshape(-1, k1) @ d["w1"].T.astype(dtype)
    if form == "dual":
        y = y + d["x2"][:, ::2, ::2].astype(dtype).reshape(-1, k2) @ d["w2"].T.astype(dtype)
    if d["scale"] is not None:
        y = y * d["scale"].astype(dtype)
    y = y + d["bias"].astype(dtype)
    if res:
        y = y + d["res"].astype(dtype).reshape(-1, n)
    return np.maximum(y, 0) if relu else y


def pack(vh, c, d, to_dev):
    """(fp32 rows, bf16x6 planes, bias on the device) of the case's filter."""
    form, k1, k2, n = c[:4]
    if form == "dual":
        one, zero = to_dev(np.ones(n, np.float32)), to_dev(np.zeros(n, np.float32))
        wp, bias = vh.pack_conv1x1_dual_weight(to_dev(d["w1"].reshape(n, k1, 1, 1)), one, to_dev(d["bias"]), to_dev(d["w2"].reshape(n, k2, 1, 1)), one, zero)
    else:
        wp, bias = vh.pack_conv_weight(to_dev(d["w1"].reshape(n, k1, 1, 1))), to_dev(d["bias"])
    return wp, vh.pack_gemm1x1_bf16x6_weight(wp), bias


def launch(vh, c, packed, a, x2, scale, res):
    """One launch of the case on the bf16x6 route (asserted through the route meter) from device tensors -> (b,h,w,N)."""
    form, k1, k2, n, rows, _, relu = c
    wp, ux6, bias = packed
    with vh.flop_meter() as fm:
        if form == "dual":
            y = vh.conv1x1_dual_fwd(a, x2, wp, bias, n, 2, relu, u_x6=ux6)
        elif form == "short":
            y = vh.conv1x1_rows_fwd(a, wp, scale, bias, n, relu, residual=res, u_x6=ux6)
        else:
            y = vh.conv2d_fwd(a, wp, scale, bias, n, 1, 1, 1, 0, relu, residual=res, u_x6=ux6)
    assert fm.routes[ROUTE[form]] == 1 and sum(fm.routes.values()) == 1, fm.routes
    return y


def run(vh, c, d, to_dev):
    opt = lambda v: None if v is None else to_dev(v)
    return launch(vh, c, pack(vh, c, d, to_dev), to_dev(d["a"]), opt(d["x2"]), opt(d["scale"]), opt(d["res"]))


def digest(y):
    """SHA-256 of the output's bytes as 32 uint8."""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(y, np.float32).tobytes()).digest(), np.uint8)
