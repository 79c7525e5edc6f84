"""Frames and the case list shared by tests/test_jpeg_ref.py (jpeg_ref against Pillow) and tests/test_gpu_jpeg.py (the kernel against
jpeg_ref).  A case is (H, W, quality, restart_rows, kind); restart_rows 0 stands for "all rows"."""
import functools

import numpy as np


def smooth(H, W, seed=0):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = np.stack([128 + 100 * np.sin((x + 3 * seed) / 37.0 + y / 53.0), 128 + 90 * np.cos(x / 71.0 - (y + seed) / 29.0), 40 + 150 * (x + y) / (H + W)], axis=-1)
    return np.clip(f, 0, 255).astype(np.uint8)


def checker(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


@functools.lru_cache(maxsize=None)
def frame(H, W, kind, seed=0):
    if kind == 'noise':
        f = np.random.default_rng(H * 8209 + W * 17 + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    elif kind == 'smooth':
        f = smooth(H, W, seed)
    elif kind == 'checker':
        f = checker(H, W)
    elif kind == 'zero':
        f = np.zeros((H, W, 3), np.uint8)
    elif kind == 'white':
        f = np.full((H, W, 3), 255, np.uint8)
    else:
        raise ValueError(kind)
    f.setflags(write=False)
    return f


def rows(H, restart_rows):
    return restart_rows if restart_rows else (H + 15) // 16


SHAPES = [(16, 16, 95, 1, 'smooth'), (8, 8, 95, 1, 'smooth'), (1, 1, 95, 1, 'noise'), (17, 16, 95, 1, 'smooth'), (16, 17, 95, 1, 'smooth'),
          (33, 47, 95, 1, 'smooth'), (33, 47, 50, 1, 'noise'), (40, 56, 75, 1, 'smooth'), (50, 70, 97, 1, 'noise'), (32, 48, 100, 1, 'checker'),
          (32, 48, 1, 1, 'noise'), (32, 48, 95, 2, 'noise'), (64, 80, 20, 1, 'smooth'), (48, 64, 95, 1, 'noise'), (96, 128, 95, 1, 'noise')]
EXTRA = [(32, 48, 95, 0, 'noise'), (96, 128, 95, 0, 'smooth'), (160, 32, 95, 1, 'noise'),          # all rows; 10 intervals: RSTn wraps past 7
         (40, 56, 95, 1, 'zero'), (40, 56, 95, 1, 'white'), (48, 64, 10, 1, 'noise')]
CASES = SHAPES + EXTRA
QUALITIES = list(range(1, 101))
