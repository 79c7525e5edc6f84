#!/usr/bin/env python3
"""time_letterbox.py -- the letterboxed detector input beside the stretch it replaces, in one process.

    python scripts/time_letterbox.py [--frames 256] [--launches 50] [--reps 3] [--steps 8] [--out profiles/r12_letterbox.jsonl]

For 1280x720 and 640x480 BGR frames (--frames of them resident in HBM) into the 640x640 canvas, device-event time per launch of
    (a) stretch        dd_resize_lanczos_batch -- the existing path (a different picture: 640 output rows are resampled, not 360 / 480)
    (b) letterbox      dd_resize_lanczos_letterbox as the process runs it by default
    (c) two_launch     the same call in a child process under DD_LETTERBOX_FUSED=0 (the switch is read once per process)
    (d) d2d_memcpy     a device-to-device copy of the bytes (b) reads plus writes: the floor
The variants of the parent alternate, --reps times each, after a warm-up of every shape; every figure is events around --launches
launches.  Then one MultiStreamPipeline YOLOv5 group of --frames streams of 640x480 stepping --steps times with detector_letterbox
off and on (empty injected detections: the detector chain runs, the tracker idles), alternated likewise.  One JSON line per figure
plus a summary line, appended to --out.  `letterbox_not_slower_than_two_launch` is true when (b)'s slowest repetition is no slower than
(c)'s fastest plus the spread of (c)'s repetitions, at both geometries -- the condition under which the one-launch form stays the default.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NET = 640
GEOMETRIES = ((1280, 720), (640, 480))


def kernel_rows(args, variants):
    import torch
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import Context
    torch.cuda.set_device(0)
    ctx = Context(0)
    hip = ctypes.CDLL('libamdhip64.so')
    N, n = args.frames, args.launches
    rows = []
    for (W, H) in GEOMETRIES:
        src = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device='cuda:0')
        dst = torch.empty((N, NET, NET, 3), dtype=torch.uint8, device='cuda:0')
        moved = N * (H * W * 3 + NET * NET * 3)                   # read + written: 2 764 800 + 1 228 800 B per 720p frame, 921 600 + 1 228 800 per 480p
        half = moved // 2                                         # a copy of `half` bytes reads and writes `moved` bytes in all
        a, b = torch.empty(half, dtype=torch.uint8, device='cuda:0'), torch.empty(half, dtype=torch.uint8, device='cuda:0')
        torch.cuda.synchronize()
        P = ctypes.c_void_p
        path = ctypes.c_int(-1)
        check(lib().dd_resize_lanczos_letterbox_plan(None, H, W, 3, 1, NET, NET, N, ctypes.byref(path), None))
        calls = {
            'stretch': lambda: check(lib().dd_resize_lanczos_batch(ctx.handle, P(src.data_ptr()), N, H, W, 3, 1, P(dst.data_ptr()), NET, NET, None)),
            'letterbox': lambda: check(lib().dd_resize_lanczos_letterbox(ctx.handle, P(src.data_ptr()), N, H, W, 3, 1, P(dst.data_ptr()), NET, NET, 114, None)),
            'd2d_memcpy': lambda: hip.hipMemcpyAsync(P(b.data_ptr()), P(a.data_ptr()), ctypes.c_size_t(half), 3, P(ctx.stream_ptr)),
        }

        def timed(fn):
            with torch.cuda.stream(ctx.torch_stream):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    fn()
                e1.record()
            ctx.sync()
            return e0.elapsed_time(e1) / n                        # ms per launch

        for v in variants:                                        # warm-up: tables, scratch, clocks
            for _ in range(5):
                calls[v]()
        ctx.sync()
        for rep in range(args.reps):
            for v in variants:                                    # alternating: a drift of the box hits all alike
                ms = timed(calls[v])
                name = 'two_launch' if (v == 'letterbox' and args.child) else v
                rows.append({'what': name, 'W': W, 'H': H, 'net': NET, 'frames': N, 'rep': rep, 'launches': n, 'ms': round(ms, 4),
                             'bytes_read_plus_written': moved, 'TB_per_s': round(moved / ms / 1e9, 3), 'letterbox_path': path.value})
                print(json.dumps(rows[-1]), flush=True)
        del src, dst, a, b
    return rows


def pipeline_rows(args):
    import torch
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import Context
    ctx = Context(0)
    S, W, H = args.frames, 640, 480
    frames = [torch.randint(0, 256, (S, H, W, 3), dtype=torch.uint8, device='cuda:0') for _ in range(2)]
    pipes = {opt: MultiStreamPipeline(S, 'synthetic-yolov5s-fp16.tflite', input_size=(W, H), context=ctx, detector_letterbox=opt) for opt in (False, True)}
    empty = pipes[False].pack_injected([([], [], [])] * S)
    torch.cuda.synchronize()
    import time

    def run(pipe, steps):
        for f in range(steps):
            pipe.step(frames[f & 1], empty, frames[(f + 1) & 1] if f + 1 < steps else None)
        torch.cuda.synchronize()

    rows = []
    for opt in (False, True):
        run(pipes[opt], 3)
    for rep in range(args.reps):
        for opt in (False, True):
            t0 = time.perf_counter()
            run(pipes[opt], args.steps)
            ms = 1e3 * (time.perf_counter() - t0) / args.steps
            rows.append({'what': 'pipeline_step', 'detector_letterbox': opt, 'streams': S, 'W': W, 'H': H, 'rep': rep, 'steps': args.steps,
                         'ms_per_step': round(ms, 3), 'frames_per_s': round(S / ms * 1e3, 1)})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--no-pipeline', action='store_true')
    ap.add_argument('--child', action='store_true', help='internal: print the letterbox launch\'s figures as `two_launch` rows and exit')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r12_letterbox.jsonl'))
    args = ap.parse_args()
    assert args.launches >= 50
    if args.child:
        kernel_rows(args, ('letterbox',))
        return
    # the child first: its process must be gone before the parent opens the GPU's memory for 256 frames of its own
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--frames', str(args.frames), '--launches', str(args.launches),
                        '--reps', str(args.reps)], env=dict(os.environ, DD_LETTERBOX_FUSED='0'), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{')]
    for row in rows:
        print(json.dumps(row), flush=True)
    rows += kernel_rows(args, ('stretch', 'letterbox', 'd2d_memcpy'))
    summary = {'what': 'summary', 'frames': args.frames}
    ok = True
    for (W, H) in GEOMETRIES:
        ms = {v: [r['ms'] for r in rows if r['what'] == v and (r['W'], r['H']) == (W, H)] for v in ('stretch', 'letterbox', 'two_launch', 'd2d_memcpy')}
        summary['%dx%d' % (W, H)] = {v: {'ms_min': min(t), 'ms_max': max(t), 'ms_median': float(np.median(t))} for v, t in ms.items()}
        ok = ok and max(ms['letterbox']) <= min(ms['two_launch']) + (max(ms['two_launch']) - min(ms['two_launch']))
    summary['letterbox_not_slower_than_two_launch'] = bool(ok)
    if not args.no_pipeline:
        rows += pipeline_rows(args)
        for opt in (False, True):
            t = [r['ms_per_step'] for r in rows if r['what'] == 'pipeline_step' and r['detector_letterbox'] == opt]
            summary['pipeline_letterbox_%s' % ('on' if opt else 'off')] = {'ms_per_step_min': min(t), 'ms_per_step_max': max(t), 'ms_per_step_median': float(np.median(t))}
    rows.append(summary)
    print(json.dumps(summary), flush=True)
    with open(args.out, 'a') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
