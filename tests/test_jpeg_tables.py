"""Huffman tables that Pillow's encoder does not write but a baseline stream may carry (tests/jpeg_synth.py): the host entropy decoder's
one-probe path must give what the two-step path gives, whatever code length a symbol has.  No GPU needed."""
import io
import os
import re

import numpy as np
import pytest

import jpeg_cases
import jpeg_synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def test_large_values_on_short_codes(vh):
    """A size-8 AC symbol with a 1-bit code: code + magnitude bits fit the 9-bit look-ahead, the value (128 .. 255 in size) does not fit
    a signed byte.  Every coefficient comes out as packed; where Pillow is importable, the numpy pixel stage equals its decode."""
    data, want = jpeg_synth.gray_block_stream(jpeg_synth.SHORT_CODE_TABLE, jpeg_synth.SHORT_CODE_COEFFICIENTS)
    info = vh.jpeg_probe(data)
    assert info.admitted and (info.height, info.width, info.components) == (8, 8, 1), info
    f = vh.jpeg_entropy_decode(data)
    assert f.coef.numpy().tolist() == want.tolist()
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(io.BytesIO(data)) as im:
        rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
    assert np.array_equal(jpeg_cases.pixel_stage(f.coef.numpy(), f.qt, f.desc), rgb)


@pytest.mark.parametrize("size", range(1, 11))
@pytest.mark.parametrize("length", [1, 2, 5, 9, 10, 16])
def test_every_size_on_every_code_length(vh, size, length):
    """One AC symbol of each size 1 .. 10 on codes of 1 .. 16 bits (around the look-ahead's 9 and past it), with the four values at
    the ends of the size's range: the coefficients are the packed ones."""
    table = {length: [size]}
    table.setdefault(length + 1 if length < 16 else 15, []).append(0x00)
    if length == 16:                                   # canonical codes: the shorter code comes first
        table = {15: [0x00], 16: [size]}
    lo, hi = 1 << (size - 1), (1 << size) - 1
    data, want = jpeg_synth.gray_block_stream(table, [(0, lo), (0, -lo), (0, hi), (0, -hi)])
    f = vh.jpeg_entropy_decode(data)
    assert f.coef.numpy().tolist() == want.tolist()


def test_oversized_and_hollow_frames_are_refused(vh):
    """A few bytes whose frame header claims 65535x65535 must not make a decode-ahead worker allocate gigabytes: frames over 2^26
    pixels are refused ("too_large"), and so is a stream too short to hold even two bits per block of the frame it declares."""
    data, _ = jpeg_synth.gray_block_stream(jpeg_synth.SHORT_CODE_TABLE, [(0, 100)])
    sof = data.index(b"\xff\xc0")
    huge = bytearray(data)
    huge[sof + 5:sof + 9] = b"\xff\xff\xff\xff"
    info = vh.jpeg_probe(bytes(huge))
    assert not info.admitted and info.reason == "too_large" and info.detail
    hollow = bytearray(data)
    hollow[sof + 5:sof + 9] = (4096).to_bytes(2, "big") * 2          # 262144 blocks declared, three bytes of entropy-coded data
    info = vh.jpeg_probe(bytes(hollow))
    assert not info.admitted and info.reason == "bad_header" and "short" in info.detail
    with pytest.raises(vh.VatlError):
        vh.jpeg_entropy_decode(bytes(hollow))


def test_python_names_mirror_the_header(vh):
    """The refusal names, the descriptor length and the library's own enums are one list: include/vatl_hip.h's VATL_JPEG_* defines (which
    csrc/jpeg.hip static_asserts against csrc/jpeg_entropy.h's enums) against vatl_hip.JPEG_REFUSALS / JPEG_DESC_INTS."""
    src = open(os.path.join(ROOT, "include", "vatl_hip.h")).read()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VATL_JPEG_([A-Z_]+)\s+(\d+)", src)}
    assert defines.pop("DESC_INTS") == vh.JPEG_DESC_INTS
    assert {name.lower(): code for name, code in defines.items()} == {name: code for code, name in enumerate(vh.JPEG_REFUSALS) if code}
