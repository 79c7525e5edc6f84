#!/usr/bin/env python
"""Generate tests/golden/letterbox_geometry.npz by running the REFERENCE's own letterbox_image (yolo3/utils.py:18-28).

For every (W, H, canvas) the reference function is called on an all-white image and the paste rectangle is read off its result: the
bounding box of the pixels that are not the canvas's 128.  Where Pillow refuses the resize (a picture without width or height:
ValueError) the row is recorded as invalid.  The fixture holds integers only:

    rows  int32 [n, 9] = W, H, w, h, new_w, new_h, off_x, off_y, valid

Nothing in the reference tree is touched.  Runs only in the build container (needs the reference tree and Pillow).
"""
import os
import sys

import numpy as np
from PIL import Image

REF = os.environ.get('DEEPDISH_REFERENCE', '/root/reference')
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'letterbox_geometry.npz')

# the geometries tests/test_gpu_letterbox.py runs, as (W, H, w, h)
NAMED = [(96, 54, 64, 64), (54, 96, 64, 64), (64, 48, 64, 64), (33, 17, 64, 64), (49, 7, 64, 64), (70, 50, 64, 48), (200, 120, 96, 96),
         (1280, 720, 640, 640), (640, 480, 640, 640), (128, 96, 640, 640), (4096, 48, 2048, 32), (3840, 2160, 640, 640)]
INVALID = [(2, 161, 64, 64), (161, 2, 64, 64), (1, 200, 64, 64)]


def cases():
    out = [(W, H, 64, 64) for W in range(2, 121) for H in range(2, 121)]
    out += NAMED + INVALID
    for net in (640, 416):
        out += [(W, H, net, net) for (W, H) in ((48, 64), (64, 48), (320, 240), (1920, 1080))]
    return out


def main():
    sys.path.insert(0, REF)
    from yolo3.utils import letterbox_image
    rows = []
    for (W, H, w, h) in cases():
        try:
            boxed = np.asarray(letterbox_image(Image.new('RGB', (W, H), (255, 255, 255)), (w, h)))
        except ValueError:
            rows.append((W, H, w, h, 0, 0, 0, 0, 0))
            continue
        assert boxed.shape == (h, w, 3)
        inside = (boxed != 128).any(axis=2)
        ys, xs = np.where(inside.any(axis=1))[0], np.where(inside.any(axis=0))[0]
        assert inside[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1].all()
        rows.append((W, H, w, h, xs[-1] + 1 - xs[0], ys[-1] + 1 - ys[0], xs[0], ys[0], 1))
    rows = np.array(rows, dtype=np.int32)
    np.savez_compressed(OUT, rows=rows)
    print('%s: %d rows, %d invalid, %d bytes' % (OUT, len(rows), int((rows[:, 8] == 0).sum()), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
