"""Cases, inputs and a numpy model of the flip-test kernels (csrc/flip.hip), shared by tools/make_flip_golden.py (which runs the
REFERENCE's flip / flip_heatmap / heatmap_to_coord_simple on them and writes tests/golden/flip_test.npz), tests/test_flip_cpu.py and
tests/test_gpu_flip.py.  Inputs are regenerated from the seeds, never stored (the fixture keeps their SHA-256, so a drifting generator is
noticed); nothing here imports the library or the reference.  Outputs of more than DIGEST_ABOVE words are stored as their SHA-256.

Shapes are the smallest at which the kernels can go wrong:
  W   1 (a row is its own mirror image), 2, 5 (odd: the thread-per-pixel kernels), 48 (the 16-byte kernels; 12 quads a row)
  H   1, 3, 64          J   1, 15, 17
  pair table   empty; the eight COCO pairs; JRDB2022's list (coco_video.py:237), which repeats joints: a general permutation
  shift        off and on, every case
  "full"       one 17 x 64 x 48 item pair of the product's size, with boxes: the planes the decode test reads
  "big"        88 x 17 x 64 x 48 = 4.6 M words = 1.15 M quads: more than the 4096 x 256 threads of the largest grid, so the grid-stride loop of
               the 16-byte kernels takes a second trip (and that of the thread-per-pixel kernels, which misaligned views of it reach, a fifth)
  "special"    +-inf and NaN entries on both sides (inf + -inf included)
"""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flip_test.npz")
DIGEST_ABOVE = 4096

COCO_PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
JRDB_PAIRS = ((1, 2), (0, 4), (3, 4), (8, 10), (5, 7), (10, 13), (14, 16), (4, 5), (7, 12), (4, 8), (3, 6), (13, 15), (11, 14), (6, 9), (8, 11))
TABLES = {"none": (), "coco": COCO_PAIRS, "jrdb": JRDB_PAIRS}

# name -> (N, J, H, W, pair table, seed)
CASES = {
    "w1": (2, 1, 1, 1, "none", 1),
    "w2": (2, 15, 3, 2, "none", 2),
    "w5": (2, 17, 3, 5, "coco", 3),
    "w5_jrdb": (2, 17, 1, 5, "jrdb", 4),
    "w48": (1, 17, 3, 48, "coco", 5),
    "w48_jrdb": (1, 17, 1, 48, "jrdb", 6),
    "h64": (1, 1, 64, 48, "none", 7),
    "j15": (1, 15, 64, 1, "none", 8),
    "special": (2, 17, 3, 5, "coco", 9),
    "full": (2, 17, 64, 48, "jrdb", 10),
    "big": (88, 17, 64, 48, "coco", 11),
}
DECODE_CASE = "full"                         # its planes are decoded with boxes()
assert CASES["big"][0] * 17 * 64 * 48 // 4 > 4096 * 256


def inputs(name):
    """-> (hm, hm_flip): the heat-maps of the first pass and of the mirrored pass, (N,J,H,W) float32."""
    n, j, h, w, _, seed = CASES[name]
    rs = np.random.RandomState(seed)
    hm, fl = (rs.standard_normal((n, j, h, w)).astype(np.float32) for _ in range(2))
    if name == "special":
        for k, v in enumerate((np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan)):
            hm.reshape(-1)[7 * k + 3] = v
            fl.reshape(-1)[11 * k + 2] = v
        # a pair that meets in the merge at shift = 0: hm[0, 1, 0, 0] takes hm_flip[0, 2, 0, W-1] (COCO swaps joints 1 and 2)
        hm[0, 1, 0, 0], fl[0, 2, 0, w - 1] = np.inf, -np.inf
    return hm, fl


def boxes(n, seed=12):
    """xyxy crop boxes of the decode planes."""
    rs = np.random.RandomState(seed)
    xy = rs.uniform(0, 400, (n, 2))
    wh = rs.uniform(40, 300, (n, 2))
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def digest(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def src_joints(pairs, j):
    """The joint each output joint takes from the mirrored maps: the swaps composed in list order, from the identity."""
    src = list(range(j))
    for a, b in pairs:
        src[a], src[b] = src[b], src[a]
    return src


def source_x(w, shift):
    """The mirrored pixel each output pixel takes: W-1-x; with the shift pixel 0 keeps W-1 and pixel x takes W-x."""
    x = np.arange(w)
    return np.where(x == 0, w - 1, w - x) if shift else w - 1 - x


def flip_heatmap_model(fl, pairs, shift):
    return fl[:, src_joints(pairs, fl.shape[1])][..., source_x(fl.shape[3], shift)]


def merge_model(hm, fl, pairs, shift):
    """csrc/flip.hip's vatl_flip_merge: one float32 sum, one exact halving."""
    with np.errstate(invalid="ignore"):                      # inf - inf of the "special" case
        return (hm + flip_heatmap_model(fl, pairs, shift)) * np.float32(0.5)


def same_bits(got, want) -> bool:
    """Bit equality, except that a NaN matches any NaN (the payload of inf - inf is the adder's business)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])
