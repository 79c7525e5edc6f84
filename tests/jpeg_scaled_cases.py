"""Files and expected frames shared by the scaled JPEG decoder's tests: tests/test_jpeg_scaled_ref.py (jpeg_scaled_ref against Pillow's
draft mode), tests/test_gpu_jpeg_scaled.py and tests/test_gpu_ingest_jpeg_scaled.py (the kernels against jpeg_scaled_ref)."""
import functools

import jpeg_scaled_ref
from jpeg_dec_cases import SAMPLINGS, pillow_file

# (H, W): exact MCUs, odd sides, a 4:2:2 chroma width <= 2 after scaling (replication instead of the filter), the one-MCU frame; every
# lopsided size both ways round
SIZES = [(8, 8), (16, 16), (17, 9), (9, 17), (37, 53), (53, 37), (33, 16), (16, 33), (16, 5), (5, 16), (3, 40), (40, 3)]
SCALES = (2, 4, 8)
RESTARTS = ('none', 'mcu1', 'row1')


def pairs():
    """(size, s) with both sides >= s: what Pillow's draft can be asked for."""
    return [((H, W), s) for (H, W) in SIZES for s in SCALES if H >= s and W >= s]


def files(H, W, sampling=None):
    """Quality 50 and 95, optimised and standard tables, no DRI, one MCU and one MCU row: 12 files a sampling, noise and ramp in turn."""
    out = []
    for smp in ([sampling] if sampling else SAMPLINGS):
        for q in (50, 95):
            for opt in (False, True):
                for r in RESTARTS:
                    out.append(pillow_file(H, W, 'ramp' if len(out) % 2 else 'noise', q, smp, r, opt))
    return out


@functools.lru_cache(maxsize=None)
def reference(data, s):
    """jpeg_scaled_ref.decode, computed once per file and scale and left unchanged."""
    out = jpeg_scaled_ref.decode(data, s)
    out.setflags(write=False)
    return out
