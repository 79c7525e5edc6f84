#!/usr/bin/env python3
"""time_ingest_jpeg.py -- the JPEG decoder and the ingest ring's JPEG slots at 640x480, timed.

    python scripts/time_ingest_jpeg.py --kernels [--frames 256,1536] [--reps 3] [--out profiles/r15_ingest_jpeg.jsonl]
    python scripts/time_ingest_jpeg.py [--streams 1536] [--steps 12] [--warmup 3] [--slots 3] [--reps 3]

--kernels: JpegDecoder.decode alone on 256 and 1536 files of a rendered-looking scene (64 distinct pictures, repeated), at quality 75
and 95, without restart markers (one lane decodes a whole file) and with one interval per MCU row: the host time of a call that has run
to its end, the device-event times of its parts (the two uploads, jpeg_markers_k, clearing + jpeg_entropy_k, jpeg_pixels_k), a
device-to-device copy of the output bytes beside it, and Pillow's decode of the same files on 16 CPU threads.  Three repetitions,
reported separately: the load of a shared machine drifts.

Default mode: the --ingest-host loop of bench.py on ONE worker group (uint8 SSD-MobileNet-v1 + MARS + deep_sort, injected detections)
with BGR, NV12 and JPEG slots in one process, alternating.  The JPEG files are this build's own encoder's (quality 95) of the rendered
frames, once with an interval per MCU row ('jpeg') and once with one interval per file ('jpeg1').  BGR and NV12 slots are filled before
the timed region (a decoder would write there directly); a JPEG slot is filled inside it, by 16 threads calling put() -- the copy into
the arena and the header parse are part of what a host pays per frame.  Per run: frames/s and the host-to-device GB/s of the slots'
bytes.  One JSON line per run plus a summary, appended to --out.  No figure here is asserted anywhere.
"""
import argparse
import io
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

W, H = 640, 480
THREADS = 16


def scene_files(quality, restart, distinct=64):
    from jpeg_dec_cases import pillow_file
    return [pillow_file(H, W, 'scene', quality, '4:2:0', restart, seed=k) for k in range(distinct)]


def kernel_mode(args):
    import ctypes
    import torch
    from PIL import Image
    from deepdish_amd.jpeg import JpegDecoder
    from deepdish_amd.runtime import Context
    torch.cuda.set_device(0)
    ctx = Context(0)
    hip = ctypes.CDLL('libamdhip64.so')
    counts = [int(v) for v in args.frames.split(',')]
    rows = []
    dec = JpegDecoder(H, W, max_frames=max(counts), max_bytes=max(counts) * 131072, context=ctx)
    dec.profile(True)
    out = torch.empty((max(counts), H, W, 3), dtype=torch.uint8, device='cuda:0')
    twin = torch.empty_like(out)
    status = torch.empty(max(counts), dtype=torch.int32, device='cuda:0')
    torch.cuda.synchronize()
    pool = ThreadPoolExecutor(THREADS)

    def pillow_one(data):
        return np.asarray(Image.open(io.BytesIO(data)).convert('RGB')).shape[0]

    for quality in (75, 95):
        for restart in ('none', 'row1'):
            base = scene_files(quality, restart)
            for n in counts:
                files = [base[i % len(base)] for i in range(n)]
                nbytes = sum(len(f) for f in files)
                for rep in range(-1, args.reps):              # rep -1 warms up
                    t0 = time.perf_counter()
                    dec.decode(files, out=out[:n], status=status[:n])
                    ms = dec.kernel_ms()
                    ctx.sync()
                    host_ms = 1e3 * (time.perf_counter() - t0)
                    if rep < 0:
                        assert int(status[:n].abs().sum().item()) == 0
                        continue
                    dev_ms = ms['markers'] + ms['entropy'] + ms['pixels']
                    rows.append({'what': 'decode', 'quality': quality, 'restart': restart, 'frames': n, 'rep': rep, 'file_bytes_mean': nbytes // n,
                                 'host_ms_whole_call': round(host_ms, 3), 'ms_upload': round(ms['upload'], 3), 'ms_markers': round(ms['markers'], 3),
                                 'ms_entropy': round(ms['entropy'], 3), 'ms_pixels': round(ms['pixels'], 3), 'kernels_frames_per_s': round(1e3 * n / dev_ms, 1)})
                    print(json.dumps(rows[-1]), flush=True)
                for rep in range(args.reps):
                    size = n * H * W * 3
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(ctx.torch_stream):
                        e0.record()
                        assert hip.hipMemcpyAsync(ctypes.c_void_p(twin.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_size_t(size), 3,
                                                  ctypes.c_void_p(ctx.stream_ptr)) == 0
                        e1.record()
                    ctx.sync()
                    rows.append({'what': 'd2d_copy_of_the_output', 'frames': n, 'rep': rep, 'ms': round(e0.elapsed_time(e1), 3)})
                    print(json.dumps(rows[-1]), flush=True)
                if n == counts[0]:
                    for rep in range(args.reps):
                        t0 = time.perf_counter()
                        list(pool.map(pillow_one, files))
                        dt = time.perf_counter() - t0
                        rows.append({'what': 'pillow_decode_16_threads', 'quality': quality, 'restart': restart, 'frames': n, 'rep': rep,
                                     'frames_per_s': round(n / dt, 1)})
                        print(json.dumps(rows[-1]), flush=True)
    return rows


def ring_mode(args):
    import bench
    cfg = bench.CONFIGS[2]
    assert (cfg['W'], cfg['H']) == (W, H)
    model = cfg['model'] + '-uint8'
    S, K = args.streams, args.slots
    pool = bench.start_gen_pool(1, S)                         # before anything touches the GPU
    os.environ.setdefault('DD_HOST_THREADS', str(bench.host_threads(1, 1)))
    import torch
    from deepdish_amd.ingest import FrameIngest
    from deepdish_amd.jpeg import JpegEncoder
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import Context
    from time_ingest_yuv import to_yuv420_dev
    torch.cuda.set_device(0)
    dev = torch.empty((K, S, H, W, 3), dtype=torch.uint8, device='cuda:0')
    dets = bench.make_inputs_rendered(pool, 0, S, K, W, H, [dev], [0, S], 'cuda:0')
    ctx = Context(0)
    pipe = MultiStreamPipeline(S, model=model, input_size=(W, H), context=ctx)
    injected = [pipe.pack_injected([dets[s][f] for s in range(S)]) for f in range(K)]
    formats = ('bgr', 'nv12', 'jpeg', 'jpeg1')
    rings, files = {}, {}
    for fmt in formats:
        if fmt.startswith('jpeg'):
            enc = JpegEncoder(H, W, quality=95, restart_rows=1 if fmt == 'jpeg' else (H + 15) // 16, context=ctx)
            files[fmt] = [[] for _ in range(K)]
            for f in range(K):
                for z0 in range(0, S, 64):
                    files[fmt][f] += enc.encode_to_host(dev[f, z0:z0 + 64])
            largest = max(sum((len(d) + 63) & ~63 for d in files[fmt][f]) for f in range(K))
            rings[fmt] = FrameIngest(S, (W, H), slots=K, context=ctx, pixel_format='jpeg', jpeg_slot_bytes=largest + 64)
        else:
            ring = FrameIngest(S, (W, H), slots=K, context=ctx, pixel_format=fmt)
            for f in range(K):
                torch.from_numpy(ring.host(f)).copy_(dev[f] if fmt == 'bgr' else to_yuv420_dev(dev[f], fmt))
            rings[fmt] = ring
    del dev
    torch.cuda.synchronize()
    det_stream = pipe.detector_stream()
    threads = ThreadPoolExecutor(THREADS)

    def fill(fmt, slot):
        if not fmt.startswith('jpeg'):
            return
        ring, data = rings[fmt], files[fmt][slot]
        chunk = (S + THREADS - 1) // THREADS

        def work(t):
            for z in range(t * chunk, min(S, (t + 1) * chunk)):
                ring.put(slot, z, data[z])
        list(threads.map(work, range(THREADS)))

    def run(fmt, f0, f1):                                     # bench.py's --ingest-host loop, slots reused round-robin
        ring = rings[fmt]
        fill(fmt, f0 % K)
        ring.submit(f0 % K)
        for f in range(f0, f1):
            if f + 1 < f1:
                fill(fmt, (f + 1) % K)
                ring.submit((f + 1) % K)                      # the next step's upload and decode run under this step's kernels
            nxt = ring.frames((f + 1) % K, stream=det_stream) if f + 1 < f1 else None
            pipe.step(ring.frames(f % K), injected[f % K], nxt)
            ring.release(f % K)
        torch.cuda.synchronize()

    rows = []
    for fmt in formats:
        run(fmt, 0, args.warmup)
        if fmt.startswith('jpeg'):
            assert int(np.abs(rings[fmt].status((args.warmup - 1) % K)).sum()) == 0
    for rep in range(args.reps):
        for fmt in formats:                                   # alternating: a drift of the machine hits all alike
            t0 = time.perf_counter()
            run(fmt, 0, args.steps)
            dt = time.perf_counter() - t0
            nbytes = sum(len(d) for d in files[fmt][0]) if fmt.startswith('jpeg') else rings[fmt].host(0).nbytes
            rows.append({'what': 'ring', 'pixel_format': fmt, 'rep': rep, 'frames_per_s': round(args.steps * S / dt, 1),
                         'h2d_GB_per_s': round(args.steps * nbytes / dt / 1e9, 2), 'ms_per_step': round(1e3 * dt / args.steps, 3),
                         'slot_bytes': nbytes, 'streams': S, 'steps': args.steps, 'slots': K, 'model': model})
            print(json.dumps(rows[-1]), flush=True)
    summary = {'what': 'ring_summary', 'streams': S, 'steps': args.steps}
    for fmt in formats:
        v = [r['frames_per_s'] for r in rows if r['pixel_format'] == fmt]
        summary[fmt] = {'frames_per_s_min': min(v), 'frames_per_s_max': max(v), 'frames_per_s_median': float(np.median(v))}
    for fmt in ('jpeg', 'jpeg1'):                             # faster only when the gap exceeds the spread of the repetitions of each
        summary[fmt + '_faster_than_bgr'] = summary[fmt]['frames_per_s_min'] > summary['bgr']['frames_per_s_max']
    rows.append(summary)
    print(json.dumps(summary), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=1536)
    ap.add_argument('--steps', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--slots', type=int, default=3, help='slots per ring (>= 2), reused round-robin')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--kernels', action='store_true', help='time the decode alone (see the module docstring)')
    ap.add_argument('--frames', default='256,1536')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r15_ingest_jpeg.jsonl'))
    args = ap.parse_args()
    assert args.slots >= 2
    rows = kernel_mode(args) if args.kernels else ring_mode(args)
    with open(args.out, 'a') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
