"""The JPEG decoder's cases, shared by tools/make_jpeg_golden.py (which writes tests/golden/jpeg.npz with Pillow) and by
tests/test_jpeg_host.py / tests/test_gpu_jpeg.py (which read it): the streams, a numpy restatement of the device's pixel stage
(csrc/jpeg.hip: libjpeg-turbo's ISLOW inverse DCT, h2v2 fancy upsampling, YCbCr -> RGB) and the seeded truncations / corruptions
that the host entropy decoder must survive."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg.npz")

# name -> (height, width, content, Pillow save arguments).  Fixture order: the 9x9 frame first, so that in a batch of all of them the
# second frame starts at byte 243 of the arena — an odd offset.
ADMITTED = (
    ("c9x9_420", 9, 9, "mixed", dict(quality=85, subsampling="4:2:0")),             # dw = dh = 5: second MCU row / column one pixel deep
    ("c8x8_444", 8, 8, "mixed", dict(quality=85, subsampling="4:4:4")),             # one block
    ("c16x16_420", 16, 16, "mixed", dict(quality=85, subsampling="4:2:0")),         # one MCU
    ("c17x23_420", 17, 23, "mixed", dict(quality=85, subsampling="4:2:0")),         # partial MCUs both ways, odd chroma sizes
    ("c15x33_420", 15, 33, "mixed", dict(quality=92, subsampling="4:2:0")),
    ("c31x18_420", 31, 18, "mixed", dict(quality=60, subsampling="4:2:0")),
    ("c40x56_444", 40, 56, "mixed", dict(quality=85, subsampling="4:4:4")),         # several MCU rows
    ("c40x56_420", 40, 56, "mixed", dict(quality=85, subsampling="4:2:0")),
    ("c17x23_gray", 17, 23, "gray", dict(quality=85)),
    ("c33x47_420_rst_blocks3", 33, 47, "mixed", dict(quality=85, subsampling="4:2:0", restart_marker_blocks=3)),
    ("c33x47_420_rst_rows1", 33, 47, "mixed", dict(quality=85, subsampling="4:2:0", restart_marker_rows=1)),
    ("c24x24_444_rst", 24, 24, "mixed", dict(quality=85, subsampling="4:4:4", restart_marker_blocks=2)),
    ("noise_q50", 24, 40, "noise", dict(quality=50, subsampling="4:2:0")),          # large coefficients
    ("noise_q100", 24, 40, "noise", dict(quality=100, subsampling="4:2:0")),        # quantiser 1
    ("checker_0_255", 32, 24, "checker", dict(quality=75, subsampling="4:4:4")),    # range limiting
    ("optimize_420", 17, 23, "mixed", dict(quality=85, subsampling="4:2:0", optimize=True)),      # non-default Huffman tables
)
REFUSED = (
    ("progressive", 40, 56, "mixed", dict(quality=85, subsampling="4:2:0", progressive=True), "not_baseline"),
    ("c16x16_422", 16, 16, "mixed", dict(quality=85, subsampling="4:2:2"), "sampling"),
    ("c6x40_420", 6, 40, "mixed", dict(quality=85, subsampling="4:2:0"), "too_small"),
    ("c40x6_420", 40, 6, "mixed", dict(quality=85, subsampling="4:2:0"), "too_small"),
    ("png", 12, 12, "mixed", None, "not_jpeg"),
)
ADMITTED_NAMES = tuple(c[0] for c in ADMITTED)
REFUSED_NAMES = tuple(c[0] for c in REFUSED)


def content(kind, h, w, seed):
    """Synthetic (h, w, 3) uint8 (or (h, w) for "gray") frames: a smooth colour ramp with texture on it, plain noise, or a
    checkerboard of 0 / 255 with noisy cells."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "noise":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "checker":
        cell = (((yy // 3) + (xx // 2)) % 2)[..., None] * 255
        flip = rng.rand(h, w, 3) < 0.15
        return np.where(flip, 255 - cell, cell).astype(np.uint8)
    ramp = np.stack([255 * xx / max(w - 1, 1), 255 * yy / max(h - 1, 1), 127 + 120 * np.sin(0.7 * xx + 0.4 * yy)], -1)
    img = np.clip(ramp + rng.normal(0, 18, (h, w, 3)), 0, 255).astype(np.uint8)
    return img[..., 1].copy() if kind == "gray" else img


def load():
    """-> {name: (stream bytes, Pillow's RGB)}, identification {"pillow": ..., "jpeglib": ...}"""
    z = np.load(GOLDEN)
    cases = {str(n): (z["bytes_" + str(n)].tobytes(), z["rgb_" + str(n)]) for n in z["names"]}
    return cases, {"pillow": str(z["pillow"]), "jpeglib": str(z["jpeglib"])}


# ---------------------------------------------------------------------------------------------------------------------
# the pixel stage in numpy (int32 throughout, like the kernels)
# ---------------------------------------------------------------------------------------------------------------------

def _idct_pass(i, shift):
    i = [v.astype(np.int32) for v in i]
    z1 = (i[2] + i[6]) * 4433
    t2, t3 = z1 - i[6] * 15137, z1 + i[2] * 6270
    t0, t1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return [(v + (1 << (shift - 1))) >> shift for v in out]


def idct_plane(coef, q, bh, bw):
    """coef (bh * bw, 64) int16 in natural order, q (64,) -> the (8 bh, 8 bw) uint8 plane."""
    x = coef.astype(np.int32).reshape(-1, 8, 8) * q.astype(np.int32).reshape(1, 8, 8)
    ws = np.stack(_idct_pass([x[:, k, :] for k in range(8)], 11), axis=1)           # pass 1: down the columns
    px = np.stack(_idct_pass([ws[:, :, k] for k in range(8)], 18), axis=2)          # pass 2: along the rows
    px = np.clip(px + 128, 0, 255).astype(np.uint8)
    return px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample_h2v2(c, h, w):
    """The (8 bh, 8 bw) chroma plane of a 4:2:0 frame -> (h, w) int32, "fancy" triangle filter."""
    dw, dh = (w + 1) // 2, (h + 1) // 2
    c = c[:dh, :dw].astype(np.int32)
    r = np.arange(dh)
    up, down = c[np.maximum(r - 1, 0)], c[np.minimum(r + 1, dh - 1)]
    s = np.empty((2 * dh, dw), np.int32)
    s[0::2], s[1::2] = 3 * c + up, 3 * c + down
    out = np.empty((2 * dh, 2 * dw), np.int32)
    left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out[:, 0::2] = (3 * s + left + 8) >> 4          # column 0: (3 s0 + s0 + 8) >> 4 = (4 s0 + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4         # column 2 dw - 1: (4 s + 7) >> 4
    return out[:h, :w]


def pixel_stage(coef, qt, desc):
    """Coefficients (natural order, per component in block raster), (3, 64) quantiser tables and the descriptor -> (h, w, 3) uint8."""
    d = [int(v) for v in desc]
    h, w, comps, samp, bw0, bh0, bwc, bhc = d[2], d[3], d[4], d[5], d[8], d[9], d[10], d[11]
    coef = np.asarray(coef).reshape(-1, 64)
    n0, nc = bw0 * bh0, bwc * bhc
    y = idct_plane(coef[:n0], qt[0], bh0, bw0)[:h, :w].astype(np.int32)
    if comps == 1:
        return np.repeat(y[..., None], 3, 2).astype(np.uint8)
    cb, cr = idct_plane(coef[n0:n0 + nc], qt[1], bhc, bwc), idct_plane(coef[n0 + nc:n0 + 2 * nc], qt[2], bhc, bwc)
    if samp == 2:
        cb, cr = upsample_h2v2(cb, h, w), upsample_h2v2(cr, h, w)
    else:
        cb, cr = cb[:h, :w].astype(np.int32), cr[:h, :w].astype(np.int32)
    cb, cr = cb - 128, cr - 128
    rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# damaged streams
# ---------------------------------------------------------------------------------------------------------------------

CUTS = 8          # truncations per admitted case, and as many single-byte corruptions: 16 * 16 = 256 streams


def _scan_start(data):
    """Offset of the first entropy-coded byte (right behind the SOS header).  The streams are Pillow's own, so a plain walk does."""
    i = 2
    while i + 4 <= len(data):
        assert data[i] == 0xFF
        m, ln = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        i += 2 + ln
        if m == 0xDA:
            return i
    raise ValueError("no scan")


def damaged(name, data):
    """-> [(label, bytes)]: CUTS truncations (header and scan) and CUTS single-byte corruptions inside the entropy-coded segment,
    seeded by the case's name."""
    rng = np.random.RandomState(sum(name.encode()) * 7919 % (2 ** 31))
    scan = _scan_start(data)
    out = []
    cuts = [2, scan - 3, scan, scan + 1, len(data) - 2]                  # in the header, at the scan's first bytes, before EOI
    while len(cuts) < CUTS:                                              # ... and inside the entropy-coded segment
        c = int(rng.randint(scan + 2, len(data) - 2))
        if c not in cuts:
            cuts.append(c)
    for c in cuts:
        out.append((f"{name}:cut{c}", data[:c]))
    for _ in range(CUTS):
        at = int(rng.randint(scan, len(data) - 2))
        b = bytearray(data)
        b[at] = (b[at] ^ int(rng.randint(1, 256))) & 0xFF
        out.append((f"{name}:flip{at}", bytes(b)))
    return out
