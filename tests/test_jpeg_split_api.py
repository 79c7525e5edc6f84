"""CPU: the public face of the split entropy stage (DD_JPEGDEC_SPLIT): the header declares the flag and dd_jpegdec_split_stats, the
binding knows the entry, and the ring refuses the option where there is nothing to decode.  What the option computes is held on the card
(tests/test_gpu_jpeg_split.py, tests/test_gpu_ingest_jpeg_split.py) and on the host (tests/test_jpeg_split_host.py)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_the_header_declares_the_flag_and_the_entry():
    text = open(os.path.join(ROOT, 'include', 'deepdish_hip.h')).read()
    assert re.search(r'^#define\s+DD_JPEGDEC_SPLIT\s+2\s*$', text, re.M)
    assert re.search(r'^int\s+dd_jpegdec_split_stats\(dd_jpegdec \*dec, int64_t \*out_host\);', text, re.M)
    from deepdish_amd import jpeg
    from deepdish_amd._lib import SIGNATURES
    assert 'dd_jpegdec_split_stats' in SIGNATURES and len(SIGNATURES['dd_jpegdec_split_stats']) == 2
    assert (jpeg.DEC_PROGRESSIVE, jpeg.DEC_SPLIT) == (1, 2)


@pytest.mark.parametrize('fmt', ['bgr', 'nv12', 'yuy2'])
def test_jpeg_split_on_a_ring_that_holds_no_files_is_a_value_error(fmt):
    from deepdish_amd.ingest import FrameIngest
    with pytest.raises(ValueError, match='jpeg_split'):
        FrameIngest(3, (64, 48), slots=1, pixel_format=fmt, jpeg_split=True)


def test_the_decoder_takes_the_argument():
    import inspect
    from deepdish_amd.ingest import FrameIngest
    from deepdish_amd.jpeg import JpegDecoder
    assert inspect.signature(JpegDecoder.__init__).parameters['split'].default is False
    assert inspect.signature(FrameIngest.__init__).parameters['jpeg_split'].default is False
    assert callable(JpegDecoder.split_stats)
