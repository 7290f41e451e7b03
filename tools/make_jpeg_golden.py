"""Writes tests/golden/jpeg.npz: the JPEG streams of tests/jpeg_cases.py, encoded AND decoded by Pillow alone
(`Image.open(...).convert("RGB")`, what alphapose/datasets/coco_video.py `_read_rgb` does), plus the Pillow / libjpeg identification.
The fixture pins libjpeg-turbo's output (ISLOW inverse DCT, fancy upsampling); see tests/golden/jpeg.md.

    python tools/make_jpeg_golden.py                      # rewrite the fixture
    python tools/make_jpeg_golden.py --dump-streams DIR   # instead: every fixture stream and every damaged stream of the host test as
                                                          # DIR/<n>.bin — the input of tools/jpeg_entropy_check.cpp
"""
import io
import os
import sys

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_cases  # noqa: E402


def encode(kind, h, w, save, seed):
    img = jpeg_cases.content(kind, h, w, seed)
    buf = io.BytesIO()
    if save is None:
        Image.fromarray(img).save(buf, format="PNG")
    else:
        Image.fromarray(img).save(buf, format="JPEG", **save)
    return buf.getvalue()


def decode(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def make():
    out = {"names": np.array([c[0] for c in jpeg_cases.ADMITTED + jpeg_cases.REFUSED]),
           "pillow": np.array(Image.__version__),
           "jpeglib": np.array(f"jpg {features.version('jpg')} libjpeg_turbo={bool(features.check_feature('libjpeg_turbo'))}")}
    for seed, case in enumerate(jpeg_cases.ADMITTED + jpeg_cases.REFUSED):
        name, h, w, kind, save = case[:5]
        data = encode(kind, h, w, save, 1000 + seed)
        rgb = decode(data)
        assert rgb.shape == (h, w, 3), (name, rgb.shape)
        out["bytes_" + name] = np.frombuffer(data, np.uint8)
        out["rgb_" + name] = rgb
    return out


if __name__ == "__main__":
    if "--dump-streams" in sys.argv:
        target = sys.argv[sys.argv.index("--dump-streams") + 1]
        os.makedirs(target, exist_ok=True)
        cases, _ = jpeg_cases.load()
        streams = [(n, cases[n][0]) for n in cases]
        for n in jpeg_cases.ADMITTED_NAMES:
            streams += jpeg_cases.damaged(n, cases[n][0])
        import jpeg_synth                                  # hand-packed Huffman tables: large values on short codes
        streams.append(("synth", jpeg_synth.gray_block_stream(jpeg_synth.SHORT_CODE_TABLE, jpeg_synth.SHORT_CODE_COEFFICIENTS)[0]))
        for k, (label, data) in enumerate(streams):
            with open(os.path.join(target, f"{k:04d}.bin"), "wb") as f:
                f.write(data)
        print(f"{len(streams)} streams -> {target}")
    else:
        fixture = make()
        np.savez_compressed(jpeg_cases.GOLDEN, **fixture)
        print(f"{jpeg_cases.GOLDEN}: {os.path.getsize(jpeg_cases.GOLDEN)} bytes, {fixture['pillow']}, {fixture['jpeglib']}")
