#!/usr/bin/env python3
"""time_jpeg.py -- the JPEG encoder (csrc/jpeg.hip) beside a copy of its input, the raw download it replaces and Pillow on the CPU; and a
group step with render and with render_jpeg.

    python scripts/time_jpeg.py [--frames 256] [--calls 10] [--reps 3] [--steps 8] [--out profiles/r14_jpeg.jsonl]

For 640x480 and 1280x720 BGR frames (--frames of them resident in HBM), once as a rendered synthetic scene (a smooth moving background
under the overlay of time_render.py: 20 tracks with paths, detections, the line, counters) and once as noise, at quality 95 with one
restart interval per MCU row:
    (a) encode          dd_jpeg_encode of all frames into preallocated slots (two launches and the wait for the lengths): host clock
                        around --calls calls, each of which ends in a stream synchronise
    (b) d2d_memcpy      a device-to-device copy of the input frames, device events: the floor
    (c) raw_download    the frames to pinned host memory: what a caller without the encoder moves
    (d) encode_to_host  JpegEncoder.encode_to_host: encode, gather the bytes in use, one download, split
    (e) pillow_16       Image.save(quality=95, subsampling='4:2:0') of every frame over 16 CPU threads, for context
alternating, --reps times each, after a warm-up, with the mean file size.  Then one MultiStreamPipeline group of --frames streams of
640x480 with 20 injected detections a stream stepping --steps times with render(streams=range(16)) and with
render_jpeg(streams=range(16)) after every step, alternated likewise.  One JSON line per figure plus a summary line, appended to --out.
"""
import argparse
import ctypes
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GEOMETRIES = ((640, 480), (1280, 720))
QUALITY = 95


def scene(kind, N, W, H, ctx):
    """u8 [N, H, W, 3] on the device."""
    import torch
    if kind == 'noise':
        return torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device='cuda:0')
    from deepdish_amd.render import Renderer
    from time_render import overlay_of
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.stack([128 + 100 * np.sin(x / 37.0 + y / 53.0), 128 + 90 * np.cos(x / 71.0 - y / 29.0), 40 + 150 * (x + y) / (H + W)], axis=-1)
    frames = torch.empty((N, H, W, 3), dtype=torch.uint8, device='cuda:0')
    for i in range(N):                                            # the background drifts by a column a frame
        frames[i] = torch.from_numpy(np.clip(np.roll(base, i, axis=1), 0, 255).astype(np.uint8)).to('cuda:0')
    torch.cuda.synchronize()
    r = Renderer(H, W, context=ctx)
    out = r.draw(frames, [overlay_of(r, W, H)] * N)
    ctx.sync()
    return out


def kernel_rows(args):
    import torch
    from PIL import Image
    from deepdish_amd._lib import lib, check
    from deepdish_amd.jpeg import JpegEncoder
    from deepdish_amd.runtime import Context
    torch.cuda.set_device(0)
    ctx = Context(0)
    hip = ctypes.CDLL('libamdhip64.so')
    N = args.frames
    P = ctypes.c_void_p
    rows = []
    for (W, H) in GEOMETRIES:
        enc = JpegEncoder(H, W, quality=QUALITY, context=ctx)
        for kind in ('rendered', 'noise'):
            src = scene(kind, N, W, H, ctx)
            nbytes = N * H * W * 3
            dst = torch.empty_like(src)
            out = torch.empty((N, enc.default_capacity), dtype=torch.uint8, device='cuda:0')
            lengths = torch.empty(N, dtype=torch.int32, device='cuda:0')
            pinned = torch.empty((N, H, W, 3), dtype=torch.uint8).pin_memory()
            torch.cuda.synchronize()

            def encode():
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    check(lib().dd_jpeg_encode(enc._h, P(src.data_ptr()), N, P(out.data_ptr()), int(out.shape[1]), P(lengths.data_ptr()), None), 'dd_jpeg_encode')
                return 1e3 * (time.perf_counter() - t0) / args.calls

            def d2d():
                with torch.cuda.stream(ctx.torch_stream):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.calls):
                        hip.hipMemcpyAsync(P(dst.data_ptr()), P(src.data_ptr()), ctypes.c_size_t(nbytes), 3, P(ctx.stream_ptr))
                    e1.record()
                ctx.sync()
                return e0.elapsed_time(e1) / args.calls

            def download():
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    pinned.copy_(src, non_blocking=True)
                    torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0) / args.calls

            files = []

            def to_host():
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    files[:] = enc.encode_to_host(src)
                return 1e3 * (time.perf_counter() - t0) / args.calls

            def pillow():
                host = pinned.numpy()

                def one(i):
                    f = io.BytesIO()
                    Image.fromarray(host[i][..., ::-1]).save(f, 'JPEG', quality=QUALITY, subsampling='4:2:0')
                    return f.tell()
                t0 = time.perf_counter()
                with ThreadPoolExecutor(16) as ex:
                    list(ex.map(one, range(N)))
                return 1e3 * (time.perf_counter() - t0)

            calls = {'encode': encode, 'd2d_memcpy': d2d, 'raw_download': download, 'encode_to_host': to_host, 'pillow_16': pillow}
            keep, args.calls = args.calls, 2
            for v in ('encode', 'd2d_memcpy', 'raw_download', 'encode_to_host'):          # warm-up: code objects, scratch, the pinned pages
                calls[v]()
            args.calls = keep
            mean_bytes = float(np.mean([len(f) for f in files]))
            for rep in range(args.reps):
                for v, fn in calls.items():                           # alternating: a drift of the box hits all alike
                    ms = fn()
                    rows.append({'what': v, 'scene': kind, 'W': W, 'H': H, 'frames': N, 'quality': QUALITY, 'rep': rep, 'calls': 1 if v == 'pillow_16' else args.calls,
                                 'ms': round(ms, 4), 'frames_per_s': round(N / ms * 1e3, 1), 'mean_file_bytes': round(mean_bytes, 1), 'raw_frame_bytes': H * W * 3,
                                 'path': enc.path})
                    print(json.dumps(rows[-1]), flush=True)
            del src, dst, out, pinned
    return rows


def pipeline_rows(args):
    import torch
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import Context
    from time_render import N_OBJ
    ctx = Context(0)
    S, W, H = args.frames, 640, 480
    frames = [torch.randint(0, 256, (S, H, W, 3), dtype=torch.uint8, device='cuda:0') for _ in range(2)]
    pipes = {opt: MultiStreamPipeline(S, input_size=(W, H), context=ctx) for opt in ('render', 'render_jpeg')}
    out = torch.empty((16, H, W, 3), dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    count = {opt: 0 for opt in pipes}

    def injected(pipe, f):
        boxes = [(float((20 + 58 * (i % 10) + 5 * f) % 580), float(40 + 200 * (i // 10)), 30.0, 90.0) for i in range(N_OBJ)]
        return pipe.pack_injected([(boxes, ['person'] * N_OBJ, [0.9] * N_OBJ)] * S)

    def run(opt, steps):
        pipe = pipes[opt]
        for _ in range(steps):
            f = count[opt]
            count[opt] += 1
            pipe.step(frames[f & 1], injected(pipe, f))
            if opt == 'render':
                pipe.render(frames[f & 1], streams=range(16), out=out)
            else:
                pipe.render_jpeg(frames[f & 1], streams=range(16))
        ctx.sync()
        torch.cuda.synchronize()

    rows = []
    for opt in pipes:
        run(opt, 4)                                               # tracks confirmed, paths begun
    for rep in range(args.reps):
        for opt in pipes:
            t0 = time.perf_counter()
            run(opt, args.steps)
            ms = 1e3 * (time.perf_counter() - t0) / args.steps
            rows.append({'what': 'pipeline_step', 'output_16_streams': opt, 'streams': S, 'W': W, 'H': H, 'rep': rep, 'steps': args.steps,
                         'ms_per_step': round(ms, 3), 'frames_per_s': round(S / ms * 1e3, 1)})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--no-pipeline', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r14_jpeg.jsonl'))
    args = ap.parse_args()
    rows = kernel_rows(args)
    summary = {'what': 'summary', 'frames': args.frames, 'quality': QUALITY}
    for (W, H) in GEOMETRIES:
        for kind in ('rendered', 'noise'):
            sel = [r for r in rows if (r['W'], r['H'], r['scene']) == (W, H, kind)]
            s = {v: float(np.median([r['ms'] for r in sel if r['what'] == v])) for v in ('encode', 'd2d_memcpy', 'raw_download', 'encode_to_host', 'pillow_16')}
            s['mean_file_bytes'] = sel[0]['mean_file_bytes']
            summary['%dx%d_%s_ms_median' % (W, H, kind)] = s
    if not args.no_pipeline:
        rows += pipeline_rows(args)
        for opt in ('render', 'render_jpeg'):
            t = [r['ms_per_step'] for r in rows if r['what'] == 'pipeline_step' and r['output_16_streams'] == opt]
            summary['pipeline_%s' % opt] = {'ms_per_step_min': min(t), 'ms_per_step_max': max(t), 'ms_per_step_median': float(np.median(t))}
    rows.append(summary)
    print(json.dumps(summary), flush=True)
    with open(args.out, 'a') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
