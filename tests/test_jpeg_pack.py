"""Host half of the device Huffman decoder (csrc/jpeg_pack.h through vh.jpeg_pack) and the algorithm the kernels run, as a pure-Python
model (tests/jpeg_huffman_model.py), both against the host decoder vh.jpeg_entropy_decode.  No GPU needed."""
import numpy as np
import pytest

import jpeg_cases
import jpeg_huffman_model as model
import jpeg_synth


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


@pytest.fixture(scope="module")
def streams():
    """{name: bytes}: the sixteen admitted fixture streams and the hand-packed one."""
    cases = jpeg_cases.load()[0]
    out = {n: cases[n][0] for n in jpeg_cases.ADMITTED_NAMES}
    out["synth"] = jpeg_synth.gray_block_stream(jpeg_synth.SHORT_CODE_TABLE, jpeg_synth.SHORT_CODE_COEFFICIENTS)[0]
    return out


NAMES = jpeg_cases.ADMITTED_NAMES + ("synth",)
RESTART_MCUS = {"c33x47_420_rst_blocks3": 3, "c33x47_420_rst_rows1": 3, "c24x24_444_rst": 2}     # 33x47 at 4:2:0: three MCUs a row


def unstuff(data, start):
    """The entropy-coded segments of a well-formed stream, FF00 -> FF, cut at every marker: [bytes], in a few lines."""
    segments, cur, i = [], bytearray(), start
    while i < len(data):
        if data[i] != 0xFF:
            cur.append(data[i]); i += 1
        elif i + 1 < len(data) and data[i + 1] == 0x00:
            cur.append(0xFF); i += 2
        else:
            segments.append(bytes(cur)); cur = bytearray()
            if i + 1 >= len(data) or not 0xD0 <= data[i + 1] <= 0xD7:
                break
            i += 2
    return segments


@pytest.mark.parametrize("name", NAMES)
def test_pack_is_the_unstuffed_scan_with_its_segment_rows(vh, streams, name):
    data = streams[name]
    p, want = vh.jpeg_pack(data), vh.jpeg_entropy_decode(data)
    assert np.array_equal(p.qt, want.qt) and np.array_equal(p.desc, want.desc)
    segments = unstuff(data, int(p.desc[14]))
    scan, rows = p.scan.numpy().tobytes(), p.segments.tolist()
    assert len(rows) == len(segments) and len(scan) % vh.JPEG_SUB_BYTES == 0 and p.huff.size == vh.JPEG_HUFF_BYTES
    at = 0
    for (off, bits, mcu0, mcus), seg in zip(rows, segments):
        assert off == at and off % vh.JPEG_SUB_BYTES == 0 and bits == 8 * len(seg)
        padded = -(-max(len(seg), 1) // vh.JPEG_SUB_BYTES) * vh.JPEG_SUB_BYTES
        assert scan[off:off + padded] == seg + bytes(padded - len(seg))
        at += padded
    assert at == len(scan)
    total = int(p.desc[6]) * int(p.desc[7])
    ri = RESTART_MCUS.get(name)
    if ri is None:
        assert [r[2:] for r in rows] == [[0, total]]
    else:
        assert int(p.desc[13]) == ri and len(rows) == -(-total // ri) > 1
        assert [r[2] for r in rows] == list(range(0, total, ri)) and [r[3] for r in rows] == [min(ri, total - m) for m in range(0, total, ri)]


def test_refused_streams_are_refused_with_the_probes_reasons(vh):
    cases = jpeg_cases.load()[0]
    for name, *_, reason in jpeg_cases.REFUSED:
        assert vh.jpeg_probe(cases[name][0]).reason == reason
        with pytest.raises(vh.VatlError, match=reason):
            vh.jpeg_pack(cases[name][0])


def test_a_misnumbered_restart_marker_is_an_error(vh, streams):
    data = bytearray(streams["c24x24_444_rst"])
    at = data.index(b"\xff\xd1", int(vh.jpeg_probe(bytes(data)).desc[14]))
    data[at + 1] = 0xD3
    with pytest.raises(vh.VatlError, match="RST1"):
        vh.jpeg_pack(bytes(data))
    with pytest.raises(vh.VatlError):
        vh.jpeg_entropy_decode(bytes(data))
    data[at:at + 2] = b"\xff\xff\xff\xd1"                              # fill bytes in front of the right marker are allowed
    assert np.array_equal(vh.jpeg_pack(bytes(data)).segments, vh.jpeg_pack(streams["c24x24_444_rst"]).segments)


def test_damaged_streams_pack_or_raise(vh, streams):
    """The 256 damaged streams: a VatlError or a packed frame, never a crash; what fails to pack the host decoder rejects too."""
    packed = failed = 0
    for name in jpeg_cases.ADMITTED_NAMES:
        for label, data in jpeg_cases.damaged(name, streams[name]):
            try:
                p = vh.jpeg_pack(data)
            except vh.VatlError:
                failed += 1
                with pytest.raises(vh.VatlError):
                    vh.jpeg_entropy_decode(data)
                continue
            packed += 1
            assert p.scan.numel() % vh.JPEG_SUB_BYTES == 0 and p.scan.numel() <= len(data) + vh.JPEG_SUB_BYTES * len(p.segments), label
    assert packed + failed == 256 and packed > 100 and failed > 10


@pytest.mark.parametrize("name", NAMES)
def test_the_model_of_the_kernels_reproduces_the_host_decoder(vh, streams, name):
    want = vh.jpeg_entropy_decode(streams[name]).coef.numpy().reshape(-1, 64)
    coef, status, rounds = model.decode(vh.jpeg_pack(streams[name]))
    assert status == "ok" and np.array_equal(coef, want)
    if name in ("noise_q50", "noise_q100"):                            # more than one subsequence: the guess at a boundary is wrong, states have to travel
        assert rounds >= 1


def test_the_model_rejects_what_the_host_decoder_rejects(vh, streams):
    """Damaged streams of three cases (restart markers, noise, plain) through the model: "ok" exactly where the host decoder succeeds."""
    seen = set()
    for name in ("c33x47_420_rst_rows1", "noise_q100", "c40x56_444"):
        for label, data in jpeg_cases.damaged(name, streams[name]):
            try:
                p = vh.jpeg_pack(data)
            except vh.VatlError:
                continue
            coef, status, _ = model.decode(p)
            try:
                want = vh.jpeg_entropy_decode(data).coef.numpy().reshape(-1, 64)
            except vh.VatlError:
                assert status != "ok", label
                seen.add(status)
                continue
            assert status == "ok" and np.array_equal(coef, want), label
            seen.add("ok")
    assert "ok" in seen and len(seen) >= 3


def test_a_segment_above_the_cap_is_refused(vh):
    """One lane walks a whole segment in the worst case, so `jpeg_pack` refuses more than 768 KiB between restart markers — a refusal of
    its own ("segment_too_long": the probe admits the stream and the host decoder takes it); with restart markers the same picture packs."""
    import io
    from PIL import Image
    img = Image.fromarray(np.random.RandomState(1).randint(0, 256, (512, 1024, 3)).astype(np.uint8))
    plain, rst = io.BytesIO(), io.BytesIO()
    img.save(plain, "JPEG", quality=100, subsampling="4:4:4")
    img.save(rst, "JPEG", quality=100, subsampling="4:4:4", restart_marker_rows=8)
    assert len(plain.getvalue()) > 800 * 1024 and vh.jpeg_probe(plain.getvalue()).admitted
    with pytest.raises(vh.VatlError, match="segment_too_long"):
        vh.jpeg_pack(plain.getvalue())
    assert vh.jpeg_entropy_decode(plain.getvalue()).blocks == 3 * 64 * 128
    assert vh.jpeg_pack(rst.getvalue()).segments.shape[0] == 8
