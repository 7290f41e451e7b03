"""Host half of the hybrid JPEG decoder (csrc/jpeg_entropy.h through vatl_jpeg_probe / vatl_jpeg_entropy_decode): no GPU needed.
The fixture tests/golden/jpeg.npz holds Pillow-written streams and Pillow's own RGB for them (tools/make_jpeg_golden.py)."""
import io
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import jpeg_cases


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


@pytest.fixture(scope="module")
def fixture():
    return jpeg_cases.load()


@pytest.mark.parametrize("name", jpeg_cases.ADMITTED_NAMES)
def test_entropy_decode_plus_numpy_pixel_stage_equals_pillow(vh, fixture, name):
    """Bytes -> coefficients on the host, then the specified integer pixel stage in numpy: Pillow's RGB exactly.  Pins the entropy decoder
    (coefficient order, de-interleaving, restart intervals, custom Huffman tables) and the arithmetic the kernels restate."""
    data, rgb = fixture[0][name]
    f = vh.jpeg_entropy_decode(data)
    assert f.coef.dtype.is_floating_point is False and f.coef.numel() == 64 * f.blocks and (f.height, f.width) == rgb.shape[:2]
    got = jpeg_cases.pixel_stage(f.coef.numpy(), f.qt, f.desc)
    assert np.array_equal(got, rgb), f"{name}: {np.count_nonzero(got != rgb)} bytes differ"


def test_this_machines_pillow_is_the_pinned_flavour(fixture):
    """`Image.open` of the fixture bytes equals the fixture RGB: says whether the libjpeg behind this machine's Pillow is the flavour
    the fixture pins (libjpeg-turbo: ISLOW + fancy upsampling; an IJG libjpeg >= 7 decodes 4:2:0 differently)."""
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("Pillow is not importable here")
    cases, ident = fixture
    for name, (data, rgb) in cases.items():
        with Image.open(io.BytesIO(data)) as im:
            got = np.asarray(im.convert("RGB"), dtype=np.uint8)
        assert np.array_equal(got, rgb), f"{name}: this Pillow decodes differently from the fixture's ({ident})"


def test_probe_admits_and_refuses(vh, fixture):
    cases, _ = fixture
    for name, h, w, kind, save in jpeg_cases.ADMITTED:
        info = vh.jpeg_probe(cases[name][0])
        assert info.admitted and info.reason == "admitted", (name, info)
        assert (info.height, info.width) == (h, w) and info.components == (1 if kind == "gray" else 3)
        assert info.sampling == ("gray" if kind == "gray" else save["subsampling"])
        per = 16 if info.sampling == "4:2:0" else 8
        luma = (-(-h // per) * per // 8) * (-(-w // per) * per // 8)
        assert info.blocks[0] == luma and info.coefficients == 64 * sum(info.blocks)
        if info.components == 3:
            assert info.blocks[1] == info.blocks[2] == (luma // 4 if per == 16 else luma)
    for name, h, w, kind, save, reason in jpeg_cases.REFUSED:
        info = vh.jpeg_probe(cases[name][0])
        assert not info.admitted and info.reason == reason and info.detail, (name, info)
        with pytest.raises(vh.VatlError):
            vh.jpeg_entropy_decode(cases[name][0])
    assert vh.jpeg_probe(b"").reason == "not_jpeg" and vh.jpeg_probe(b"\xff\xd8\xff").reason == "not_jpeg"


def test_damaged_streams_return_an_error_or_stay_inside_their_blocks(vh, fixture):
    """Every admitted case cut short at seeded points and hit by as many seeded single-byte corruptions of its entropy-coded segment
    (256 streams): each call is refused, raises the library's error, or succeeds with exactly the coefficient count its descriptor
    declares, written into a buffer of exactly that size with canaries behind it.  The process survives."""
    lib = vh.lib()
    outcomes = {"refused": 0, "error": 0, "decoded": 0}
    n = 0
    for name in jpeg_cases.ADMITTED_NAMES:
        for label, data in jpeg_cases.damaged(name, fixture[0][name][0]):
            n += 1
            info = vh.jpeg_probe(data)
            if not info.admitted:
                outcomes["refused"] += 1
                continue
            src = np.frombuffer(data, np.uint8).copy()
            coef = np.full(info.coefficients + 64, 0x5A5A, np.int16)                  # 64 canaries behind the declared count
            qt, desc = np.zeros((3, 64), np.uint16), np.zeros(vh.JPEG_DESC_INTS, np.int32)
            rc = lib.vatl_jpeg_entropy_decode(src.ctypes.data, src.size, coef.ctypes.data, info.coefficients, qt.ctypes.data, desc.ctypes.data)
            assert np.all(coef[info.coefficients:] == 0x5A5A), label
            if rc != 0:
                assert rc < 0 and lib.vatl_last_error(), label
                outcomes["error"] += 1
            else:
                assert 64 * int(desc[12]) == info.coefficients, label
                outcomes["decoded"] += 1
    assert n == 2 * jpeg_cases.CUTS * len(jpeg_cases.ADMITTED_NAMES) <= 400
    assert outcomes["error"] >= len(jpeg_cases.ADMITTED_NAMES), outcomes          # cuts inside the scan are errors, not silent zeros
    # too small a capacity is an error before anything is written
    data = fixture[0]["c40x56_420"][0]
    info = vh.jpeg_probe(data)
    src, coef = np.frombuffer(data, np.uint8), np.full(info.coefficients, 0x5A5A, np.int16)
    qt, desc = np.zeros((3, 64), np.uint16), np.zeros(vh.JPEG_DESC_INTS, np.int32)
    assert lib.vatl_jpeg_entropy_decode(src.ctypes.data, src.size, coef.ctypes.data, info.coefficients - 1, qt.ctypes.data, desc.ctypes.data) < 0
    assert np.all(coef == 0x5A5A)


def test_eight_threads_decode_what_one_thread_decodes(vh, fixture):
    cases, _ = fixture
    single = {n: vh.jpeg_entropy_decode(cases[n][0]) for n in jpeg_cases.ADMITTED_NAMES}
    jobs = [n for _ in range(8) for n in jpeg_cases.ADMITTED_NAMES]
    with ThreadPoolExecutor(max_workers=8) as pool:
        many = list(pool.map(lambda n: vh.jpeg_entropy_decode(cases[n][0]), jobs))
    for n, f in zip(jobs, many):
        assert np.array_equal(f.coef.numpy(), single[n].coef.numpy()) and np.array_equal(f.qt, single[n].qt) and np.array_equal(f.desc, single[n].desc), n
