"""The hand-packed stream of tests/jpeg_synth.py (large coefficients on short Huffman codes, quantiser 1) through the whole hybrid path."""
import io

import numpy as np
import pytest

import jpeg_cases
import jpeg_synth
from gpu_util import dev

pytestmark = pytest.mark.gpu


def test_short_code_stream_on_the_device():
    import vatl_hip as vh
    data, want = jpeg_synth.gray_block_stream(jpeg_synth.SHORT_CODE_TABLE, jpeg_synth.SHORT_CODE_COEFFICIENTS)
    f = vh.jpeg_entropy_decode(data)
    assert f.coef.numpy().tolist() == want.tolist()
    out, offsets, hw = vh.jpeg_decode_batch([f], dev())
    got = out.cpu().numpy().reshape(8, 8, 3)
    assert np.array_equal(got, jpeg_cases.pixel_stage(want, f.qt, f.desc))
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        assert np.array_equal(got, np.asarray(im.convert("RGB"), dtype=np.uint8))
