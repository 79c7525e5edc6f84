#!/usr/bin/env python3
"""time_jpeg_progressive.py -- progressive (SOF2) files beside baseline ones through the JPEG decoder, timed in one process.

    python scripts/time_jpeg_progressive.py [--reps 3] [--out profiles/r21_jpeg_progressive.jsonl]

1 536 files of 640 x 480 (rendered-looking scenes, 4:2:0, quality 75; 64 distinct pictures, repeated) as Pillow writes them: baseline and
progressive (libjpeg's default script: 10 scans, 3 levels), each with one restart interval per MCU row and with none.  For each kind
JpegDecoder(progressive=True).decode with JpegDecoder.profile: the device-event times of the call's parts -- the uploads, the marker
kernels, clearing + the entropy kernels, the pixel kernel -- and jpeg_prog_entropy_k level by level; the baseline kinds also on a decoder
made without the option, the same process's yardstick for what the option costs files that do not need it.  Beside them Pillow
(libjpeg-turbo) decoding the same 1 536 files on 16 threads, on the host clock.

Three repetitions, reported separately.  One JSON line per measurement, appended to --out.  No figure here is asserted anywhere."""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

THREADS = 16
H, W, N, DISTINCT = 480, 640, 1536, 64
KINDS = (('baseline', 'row1', False), ('baseline', 'none', False), ('progressive', 'row1', True), ('progressive', 'none', True))


def scene_files(restart, progressive):
    from jpeg_dec_cases import pillow_file
    base = [pillow_file(H, W, 'scene', 75, '4:2:0', restart, seed=k, progressive=progressive) for k in range(DISTINCT)]
    return [base[i % DISTINCT] for i in range(N)]


def pillow_ms(files, threads):
    from PIL import Image

    def work(data):
        return Image.open(io.BytesIO(data)).convert('RGB').size
    t0 = time.perf_counter()
    list(threads.map(work, files, chunksize=N // THREADS))
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r21_jpeg_progressive.jsonl'))
    args = ap.parse_args()
    import torch
    from deepdish_amd.jpeg import JpegDecoder
    from deepdish_amd.runtime import Context
    torch.cuda.set_device(0)
    ctx = Context(0)
    threads = ThreadPoolExecutor(THREADS)
    rows = []
    for fmt, restart, progressive in KINDS:
        files = scene_files(restart, progressive)
        nbytes = sum(len(f) for f in files)
        for option in ((True, False) if not progressive else (True,)):
            dec = JpegDecoder(H, W, max_frames=N, max_bytes=nbytes + 64 * N + 64, context=ctx, progressive=option)
            dec.profile(True)
            out = torch.empty((N, H, W, 3), dtype=torch.uint8, device='cuda:0')
            status = torch.empty(N, dtype=torch.int32, device='cuda:0')
            torch.cuda.synchronize()
            for rep in range(-1, args.reps):                      # rep -1 warms up
                t0 = time.perf_counter()
                dec.decode(files, out=out, status=status)
                ms = dec.kernel_ms()
                levels = dec.level_ms() if option else []
                ctx.sync()
                host_ms = 1e3 * (time.perf_counter() - t0)
                if rep < 0:
                    assert int(status.abs().sum().item()) == 0
                    continue
                rows.append({'what': 'decode', 'files': fmt, 'restart': restart, 'decoder': 'progressive=True' if option else 'default', 'size': '%dx%d' % (W, H),
                             'frames': N, 'rep': rep, 'file_bytes_mean': nbytes // N, 'host_ms_whole_call': round(host_ms, 3), 'ms_upload': round(ms['upload'], 3),
                             'ms_markers': round(ms['markers'], 3), 'ms_entropy': round(ms['entropy'], 3), 'ms_prog_entropy_per_level': [round(v, 3) for v in levels],
                             'ms_pixels': round(ms['pixels'], 3), 'ms_decode': round(ms['markers'] + ms['entropy'] + ms['pixels'], 3),
                             'frames_per_s_decode': round(N / (1e-3 * (ms['markers'] + ms['entropy'] + ms['pixels'])), 1)})
                print(json.dumps(rows[-1]), flush=True)
            del dec, out
            torch.cuda.empty_cache()
        for rep in range(args.reps):
            ms = pillow_ms(files, threads)
            rows.append({'what': 'pillow_16_threads', 'files': fmt, 'restart': restart, 'size': '%dx%d' % (W, H), 'frames': N, 'rep': rep, 'ms': round(ms, 3),
                         'frames_per_s': round(N / (1e-3 * ms), 1)})
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
