#!/usr/bin/env python3
"""time_jpeg_scaled.py -- the JPEG decoder and the ingest ring's JPEG slots at scale 1, 1/2, 1/4 and 1/8, timed in one process.

    python scripts/time_jpeg_scaled.py [--reps 3] [--out profiles/r18_jpeg_scaled.jsonl] [--skip-ring]

1. JpegDecoder(scale=s).decode with JpegDecoder.profile on 1 536 files of 640 x 480 and on 256 files of 1920 x 1080 (rendered-looking
   scenes, 4:2:0, quality 75, one restart interval per MCU row; 64 / 16 distinct pictures, repeated) at s = 1, 2, 4, 8: the device-event
   times of the call's parts (clearing + jpeg_entropy_k, which the scale does not touch, and the pixel kernel: jpeg_pixels_k at s = 1,
   jpeg_pixels_scaled_k<s> otherwise) and a device-to-device copy of each scale's output bytes beside it.  The s = 1 rows are the
   full-size kernels, the baseline of the same process.
2. The ring on a 256-stream group of 1920 x 1080 files with dst_size=(640, 480), jpeg_scale=1 against 'auto' (1/2): put() by 16 threads,
   submit, acquire and a wait for the slot -- upload, decode and resize -- on the host clock, the two rings alternating.

Three repetitions, reported separately.  One JSON line per measurement, appended to --out.  No figure here is asserted anywhere."""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

THREADS = 16
GROUPS = (((480, 640), 1536, 64), ((1080, 1920), 256, 16))              # (H, W), files in a call, distinct pictures
SCALES = (1, 2, 4, 8)


def scene_files(H, W, distinct):
    from jpeg_dec_cases import pillow_file
    return [pillow_file(H, W, 'scene', 75, '4:2:0', 'row1', seed=k) for k in range(distinct)]


def decoder_rows(args, ctx):
    import torch
    from deepdish_amd.jpeg import JpegDecoder
    hip = ctypes.CDLL('libamdhip64.so')
    rows = []
    for (H, W), n, distinct in GROUPS:
        base = scene_files(H, W, distinct)
        files = [base[i % distinct] for i in range(n)]
        nbytes = sum(len(f) for f in files)
        for s in SCALES:
            dec = JpegDecoder(H, W, max_frames=n, max_bytes=nbytes + 64 * n + 64, context=ctx, scale=s)
            dec.profile(True)
            out = torch.empty((n, dec.out_H, dec.out_W, 3), dtype=torch.uint8, device='cuda:0')
            twin = torch.empty_like(out)
            status = torch.empty(n, dtype=torch.int32, device='cuda:0')
            torch.cuda.synchronize()
            for rep in range(-1, args.reps):                      # rep -1 warms up
                t0 = time.perf_counter()
                dec.decode(files, out=out, status=status)
                ms = dec.kernel_ms()
                ctx.sync()
                host_ms = 1e3 * (time.perf_counter() - t0)
                if rep < 0:
                    assert int(status.abs().sum().item()) == 0
                    continue
                rows.append({'what': 'decode', 'size': '%dx%d' % (W, H), 'frames': n, 'scale': s, 'rep': rep, 'out_size': '%dx%d' % (dec.out_W, dec.out_H),
                             'file_bytes_mean': nbytes // n, 'host_ms_whole_call': round(host_ms, 3), 'ms_upload': round(ms['upload'], 3),
                             'ms_markers': round(ms['markers'], 3), 'ms_entropy': round(ms['entropy'], 3), 'ms_pixels': round(ms['pixels'], 3),
                             'ms_decode': round(ms['markers'] + ms['entropy'] + ms['pixels'], 3)})
                print(json.dumps(rows[-1]), flush=True)
            for rep in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(ctx.torch_stream):
                    e0.record()
                    assert hip.hipMemcpyAsync(ctypes.c_void_p(twin.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_size_t(out.numel()), 3,
                                              ctypes.c_void_p(ctx.stream_ptr)) == 0
                    e1.record()
                ctx.sync()
                rows.append({'what': 'd2d_copy_of_the_output', 'size': '%dx%d' % (W, H), 'frames': n, 'scale': s, 'rep': rep, 'bytes': out.numel(),
                             'ms': round(e0.elapsed_time(e1), 3)})
                print(json.dumps(rows[-1]), flush=True)
            del dec, out, twin
            torch.cuda.empty_cache()
    return rows


def ring_rows(args, ctx):
    import torch
    from deepdish_amd.ingest import FrameIngest
    (H, W), S, distinct = GROUPS[1]
    base = scene_files(H, W, distinct)
    files = [base[i % distinct] for i in range(S)]
    arena = sum((len(f) + 63) & ~63 for f in files) + 64
    rings = {name: FrameIngest(S, (W, H), (640, 480), slots=2, context=ctx, pixel_format='jpeg', jpeg_slot_bytes=arena, jpeg_scale=scale)
             for name, scale in (('scale_1', 1), ('auto', 'auto'))}
    assert rings['auto'].jpeg_scale == 2
    threads = ThreadPoolExecutor(THREADS)
    chunk = (S + THREADS - 1) // THREADS

    def step(ring, slot):
        def work(t):
            for z in range(t * chunk, min(S, (t + 1) * chunk)):
                ring.put(slot, z, files[z])
        list(threads.map(work, range(THREADS)))
        ring.submit(slot)
        ring.acquire(slot)
        status = ring.status(slot)                                # waits for the slot's work
        ring.release(slot)
        return status

    rows = []
    for name, ring in rings.items():
        for k in range(2):
            assert int(np.abs(step(ring, k % 2)).sum()) == 0
    for rep in range(args.reps):
        for name, ring in rings.items():                          # alternating: a drift of the machine hits both alike
            t0 = time.perf_counter()
            for k in range(args.steps):
                step(ring, k % 2)
            dt = time.perf_counter() - t0
            rows.append({'what': 'ring_1080p_to_640x480', 'jpeg_scale': name, 'scale': ring.jpeg_scale, 'rep': rep, 'streams': S, 'steps': args.steps,
                         'ms_per_step': round(1e3 * dt / args.steps, 3), 'frames_per_s': round(args.steps * S / dt, 1)})
            print(json.dumps(rows[-1]), flush=True)
    torch.cuda.synchronize()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=8, help='ring: steps per repetition')
    ap.add_argument('--skip-ring', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r18_jpeg_scaled.jsonl'))
    args = ap.parse_args()
    import torch
    from deepdish_amd.runtime import Context
    torch.cuda.set_device(0)
    ctx = Context(0)
    rows = decoder_rows(args, ctx)
    if not args.skip_ring:
        rows += ring_rows(args, ctx)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
