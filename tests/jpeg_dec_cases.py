"""Files shared by the JPEG decoder's tests: tests/test_jpeg_dec_ref.py (jpeg_dec_ref against Pillow), tests/test_jpeg_parse.py (the header
parser against jpeg_dec_ref's), tests/test_gpu_jpeg_decode.py and tests/test_gpu_ingest_jpeg.py (the kernels against jpeg_dec_ref).  All
are written at test time, by Pillow and by jpeg_ref.encode, from seeded pictures."""
import functools
import io

import numpy as np

import jpeg_dec_ref
import jpeg_ref

SAMPLINGS = ['4:2:0', '4:2:2', '4:4:4', 'L']
RESTARTS = {'none': {}, 'mcu1': {'restart_marker_blocks': 1}, 'mcu3': {'restart_marker_blocks': 3}, 'row1': {'restart_marker_rows': 1}}


@functools.lru_cache(maxsize=None)
def picture(H, W, kind, seed=0):
    """u8 [H, W, 3] BGR: 'noise', a smooth 'ramp', or a rendered-looking 'scene' (a gradient, flat boxes, a little grain)."""
    rng = np.random.default_rng(H * 8209 + W * 17 + seed)
    if kind == 'noise':
        f = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    elif kind == 'ramp':
        y, x = np.mgrid[0:H, 0:W]
        f = np.stack([(x * 7 + y * 3 + seed) % 256, (x * 2 + y * 5) % 256, (x + y) * 255 // max(1, H + W - 2)], axis=-1).astype(np.uint8)
    elif kind == 'scene':
        y, x = np.mgrid[0:H, 0:W]
        f = np.stack([60 + 120 * y / H, 90 + 60 * x / W, 140 - 80 * y / H], axis=-1)
        for _ in range(12):
            y0, x0 = int(rng.integers(0, H - 8)), int(rng.integers(0, W - 8))
            f[y0:y0 + int(rng.integers(8, H // 3)), x0:x0 + int(rng.integers(8, W // 4))] = rng.integers(0, 256, 3)
        f = np.clip(f + rng.normal(0, 2.0, f.shape), 0, 255).astype(np.uint8)
    else:
        raise ValueError(kind)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def pillow_file(H, W, kind, quality, sampling, restart='none', optimize=False, seed=0, progressive=False):
    from PIL import Image
    bgr = picture(H, W, kind, seed)
    f = io.BytesIO()
    kw = dict(RESTARTS[restart], quality=quality, optimize=optimize, progressive=progressive)
    if sampling == 'L':
        Image.fromarray(np.ascontiguousarray(bgr[..., 1])).save(f, 'JPEG', **kw)
    else:
        Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(f, 'JPEG', subsampling=sampling, **kw)
    return f.getvalue()


@functools.lru_cache(maxsize=None)
def own_file(H, W, kind, quality, restart_rows, seed=0):
    """What this build's own encoder writes (4:2:0, Annex K tables, a DRI segment)."""
    return jpeg_ref.encode(picture(H, W, kind, seed), quality, restart_rows)


def pillow_decode(data):
    """Pillow's pixels as cv2.imread orders them."""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))[..., ::-1]


@functools.lru_cache(maxsize=None)
def reference(data):
    """jpeg_dec_ref.decode, computed once per file and left unchanged."""
    out = jpeg_dec_ref.decode(data)
    out.setflags(write=False)
    return out
