#!/usr/bin/env python3
"""time_ingest_jpeg_anysize.py -- what jpeg_any_size costs on uniform input, and what one ring for a mixed fleet costs against a ring per size.

    python scripts/time_ingest_jpeg_anysize.py [--reps 3] [--out profiles/r25_jpeg_anysize.jsonl]

One process, three repetitions, the variants of a part following each other inside a repetition, so a drift of the machine hits all alike.
The files are the rendered-looking scenes of scripts/time_ingest_jpeg.py (4:2:0, quality 75, one restart interval per MCU row), 16 distinct
pictures a size, repeated.

  uniform   1 536 files of 640 x 480 into dst 640 x 480.  Device events (JpegDecoder.profile()): the kernels of a default decoder and of an
            any_size decoder of the same maximum.  Host clock: a fixed ring (decodes straight into the slot) and an any-size ring of the same
            maximum with jpeg_scale='auto' (staging buffer, then crop_resize), from the first put (16 threads) to status(slot) coming back.
  fleet     768 streams, one third each 640 x 480, 1280 x 720 and 1920 x 1080, into dst 640 x 480.  Host clock, the same span: one any-size
            ring (maximum 1920 x 1080, 'auto': 4.8 GB of staging) against three fixed rings of 256 streams at their own sizes and 'auto',
            filled and submitted one after the other and then waited for.

One JSON line per run, appended to --out.  No figure here is asserted anywhere.  The frames are: the warm-up holds the any-size decoder's
and the any-size ring's output on the uniform input to the fixed ones', byte for byte."""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'scripts')):
    if p not in sys.path:
        sys.path.insert(0, p)

THREADS = 16
DST = (640, 480)
FLEET = [(640, 480), (1280, 720), (1920, 1080)]


def scene_files(w, h, distinct=16):
    from jpeg_dec_cases import pillow_file
    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(lambda k: pillow_file(h, w, 'scene', 75, '4:2:0', 'row1', seed=k), range(distinct)))


def arena(files):
    return sum((len(f) + 63) & ~63 for f in files) + 64


def fill(threads, ring, slot, files, z0=0):
    n = len(files)
    chunk = (n + THREADS - 1) // THREADS

    def work(t):
        for z in range(t * chunk, min(n, (t + 1) * chunk)):
            ring.put(slot, z0 + z, files[z])
    list(threads.map(work, range(THREADS)))


def read(ctx, addr, n):
    import torch
    ctx.sync()
    out = torch.empty(n, dtype=torch.uint8, device='cuda:0')
    assert ctypes.CDLL('libamdhip64.so').hipMemcpy(ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(addr), ctypes.c_size_t(n), 3) == 0
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--uniform', type=int, default=1536)
    ap.add_argument('--fleet', type=int, default=768, help='streams of the fleet, a multiple of 3')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r25_jpeg_anysize.jsonl'))
    args = ap.parse_args()
    assert args.fleet % 3 == 0
    base = {wh: scene_files(*wh) for wh in FLEET}             # before anything touches the GPU
    import torch
    from deepdish_amd.ingest import FrameIngest
    from deepdish_amd.jpeg import JpegDecoder
    from deepdish_amd.runtime import Context
    torch.cuda.set_device(0)
    ctx = Context(0)
    threads = ThreadPoolExecutor(THREADS)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---------------------------------------------------------------- uniform: the kernels
    n, (w, h) = args.uniform, FLEET[0]
    files = [base[FLEET[0]][i % 16] for i in range(n)]
    kw = dict(max_frames=n, max_bytes=arena(files), context=ctx)
    decs = [('fixed', JpegDecoder(h, w, **kw)), ('any_size', JpegDecoder(h, w, any_size=True, **kw))]
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device='cuda:0')
    want = torch.empty_like(out)
    status = torch.empty(n, dtype=torch.int32, device='cuda:0')
    torch.cuda.synchronize()
    for _, dec in decs:
        dec.profile(True)
    for rep in range(-1, args.reps):
        for name, dec in decs:
            dec.decode(files, out=want if (rep < 0 and name == 'fixed') else out, status=status)
            ms = dec.kernel_ms()
            ctx.sync()
            if rep < 0:
                assert int(status.abs().sum().item()) == 0 and (name == 'fixed' or torch.equal(out, want))
                continue
            emit({'what': 'uniform_kernels', 'variant': name, 'files': n, 'size': [w, h], 'rep': rep, 'ms_markers': round(ms['markers'], 3),
                  'ms_entropy': round(ms['entropy'], 3), 'ms_pixels': round(ms['pixels'], 3)})
    del decs, out, want, status
    torch.cuda.empty_cache()

    # ---------------------------------------------------------------- uniform: the rings
    rkw = dict(slots=2, context=ctx, pixel_format='jpeg', jpeg_slot_bytes=arena(files))
    rings = [('fixed', FrameIngest(n, (w, h), DST, **rkw)), ('any_size', FrameIngest(n, (w, h), DST, jpeg_any_size=True, jpeg_scale='auto', **rkw))]
    frames = {}
    for rep in range(-1, args.reps):
        for name, ring in rings:
            slot = rep % 2
            t0 = time.perf_counter()
            fill(threads, ring, slot, files)
            t1 = time.perf_counter()
            ring.submit(slot)
            st = ring.status(slot)
            dt = time.perf_counter() - t0
            assert int(np.abs(st).sum()) == 0
            if rep < 0:
                frames[name] = read(ctx, ring.acquire(slot), n * DST[0] * DST[1] * 3)
            ring.release(slot)
            if rep >= 0:
                emit({'what': 'uniform_ring', 'variant': name, 'streams': n, 'size': [w, h], 'dst': list(DST), 'rep': rep, 'ms_put': round(1e3 * (t1 - t0), 3),
                      'ms_submit_to_status': round(1e3 * (dt - (t1 - t0)), 3), 'ms': round(1e3 * dt, 3), 'frames_per_s': round(n / dt, 1)})
    assert torch.equal(frames['fixed'], frames['any_size']), 'the any-size ring differs from the fixed ring'
    del rings, frames
    torch.cuda.empty_cache()

    # ---------------------------------------------------------------- fleet
    third = args.fleet // 3
    per = {wh: [base[wh][i % 16] for i in range(third)] for wh in FLEET}
    mixed = [f for wh in FLEET for f in per[wh]]
    big_w, big_h = FLEET[-1]
    one = FrameIngest(args.fleet, (big_w, big_h), DST, slots=2, context=ctx, pixel_format='jpeg', jpeg_slot_bytes=arena(mixed), jpeg_any_size=True, jpeg_scale='auto')
    three = [FrameIngest(third, wh, DST, slots=2, context=ctx, pixel_format='jpeg', jpeg_slot_bytes=arena(per[wh]), jpeg_scale='auto') for wh in FLEET]
    scales = [r.jpeg_scale for r in three]
    for rep in range(-1, args.reps):
        slot = rep % 2
        for name in ('any_size_one_ring', 'three_fixed_rings'):
            t0 = time.perf_counter()
            if name == 'any_size_one_ring':
                fill(threads, one, slot, mixed)
                one.submit(slot)
                bad = int(np.abs(one.status(slot)).sum())
                one.release(slot)
            else:
                for ring, wh in zip(three, FLEET):
                    fill(threads, ring, slot, per[wh])
                    ring.submit(slot)
                bad = sum(int(np.abs(ring.status(slot)).sum()) for ring in three)
                for ring in three:
                    ring.release(slot)
            dt = time.perf_counter() - t0
            assert bad == 0
            if rep >= 0:
                emit({'what': 'fleet', 'variant': name, 'streams': args.fleet, 'sizes': [list(wh) for wh in FLEET], 'dst': list(DST), 'fixed_ring_scales': scales, 'rep': rep,
                      'ms': round(1e3 * dt, 3), 'frames_per_s': round(args.fleet / dt, 1), 'staging_bytes': args.fleet * big_w * big_h * 3 if name == 'any_size_one_ring' else None})
    assert sorted(set(map(tuple, one.source_sizes(0).tolist()))) == sorted((wh[0], wh[1], sc) for wh, sc in zip(FLEET, scales))

    summary = {'what': 'summary'}
    for what, key in (('uniform_kernels', 'ms_pixels'), ('uniform_ring', 'ms'), ('fleet', 'ms')):
        for variant in sorted({r['variant'] for r in rows if r['what'] == what}):
            v = [r[key] for r in rows if r['what'] == what and r['variant'] == variant]
            summary['%s.%s.%s' % (what, variant, key)] = [min(v), max(v)]
    emit(summary)
    with open(args.out, 'a') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
