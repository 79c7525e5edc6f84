"""CPU: tests/jpeg_scaled_ref.py held to Pillow (libjpeg-turbo) byte for byte: Image.draft selects libjpeg's 1/2, 1/4 and 1/8 decode, and
the ref must give those pixels for every sampling, table kind and restart layout at the sizes where the block sizes, the plane sizes and
the choice of up-sampler can go wrong.  draft_scale is held to the size Image.draft ends up with."""
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_scaled_ref  # noqa: E402
from jpeg_dec_cases import SAMPLINGS, pillow_file  # noqa: E402
from jpeg_scaled_cases import SCALES, SIZES, files, pairs, reference  # noqa: E402


def _pillow(data, H, W, s):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.draft(im.mode, (W // s, H // s))
    assert im.size == (-(-W // s), -(-H // s)), 'Pillow chose another scale'
    return np.asarray(im.convert('RGB'))[..., ::-1]


def test_the_condition_leaves_out_only_the_smallest_sides():
    """Pillow's draft cannot be asked for a side of 0: (size, s) pairs need both sides >= s."""
    kept = pairs()
    assert all(((H, W), 2) in kept for (H, W) in SIZES)
    dropped = [(hw, s) for hw in SIZES for s in SCALES if (hw, s) not in kept]
    assert all(s in (4, 8) and min(hw) in (3, 5) for hw, s in dropped), dropped


@pytest.mark.parametrize('sampling', SAMPLINGS)
@pytest.mark.parametrize('H,W', SIZES, ids=lambda v: str(v))
def test_ref_equals_pillow_draft(H, W, sampling):
    scales = [s for (hw, s) in pairs() if hw == (H, W)]
    assert scales
    for data in files(H, W, sampling):
        for s in scales:
            got = reference(data, s)
            assert got.shape == (-(-H // s), -(-W // s), 3)
            assert np.array_equal(got, _pillow(data, H, W, s)), 'scale 1/%d differs from Pillow' % s


def test_scale_1_is_the_full_size_ref():
    import jpeg_dec_ref
    data = pillow_file(17, 9, 'noise', 95, '4:2:0')
    assert np.array_equal(jpeg_scaled_ref.decode(data, 1), jpeg_dec_ref.decode(data))
    with pytest.raises(ValueError, match='3'):
        jpeg_scaled_ref.decode(data, 3)


def test_block_sizes_are_jdmasters():
    """4:2:0 chroma keeps twice the luma's block (no up-sampling at all); 4:2:2 chroma the luma's (h2v1); everything else 8 / s."""
    for s, n in ((2, 4), (4, 2), (8, 1)):
        assert jpeg_scaled_ref.block_size(2, 2, 2, 2, s) == n and jpeg_scaled_ref.block_size(1, 1, 2, 2, s) == 2 * n
        assert jpeg_scaled_ref.block_size(2, 1, 2, 1, s) == n and jpeg_scaled_ref.block_size(1, 1, 2, 1, s) == n
        assert jpeg_scaled_ref.block_size(1, 1, 1, 1, s) == n
    assert jpeg_scaled_ref.block_size(1, 1, 2, 2, 1) == 8
    assert jpeg_scaled_ref.plane_size(37, 53, 1, 1, 2, 1, 2) == (4, 19, 14)


@pytest.mark.parametrize('src', [(64, 48), (640, 480), (1920, 1080), (1280, 720), (3840, 2160), (17, 9), (100, 7)], ids=lambda v: '%dx%d' % v)
def test_draft_scale_is_pillows_rule(src):
    from PIL import Image
    data = pillow_file(src[1], src[0], 'ramp', 50, '4:2:0') if src[0] <= 100 else None
    for want in [(640, 480), (300, 300), (32, 24), (20, 15), (1, 1), (7, 5), (4000, 3000), src, (src[0] // 2, src[1] // 2), (src[0] // 2 + 1, src[1] // 2)]:
        if want[0] < 1 or want[1] < 1:
            continue
        s = jpeg_scaled_ref.draft_scale(src, want)
        k = min(src[0] // want[0], src[1] // want[1])
        assert s in (1, 2, 4, 8) and (s <= k or (k == 0 and s == 1)) and (s == 8 or 2 * s > k)
        if data is not None:
            im = Image.open(io.BytesIO(data))
            im.draft(im.mode, want)
            assert im.size == (-(-src[0] // s), -(-src[1] // s)), (src, want, s)
