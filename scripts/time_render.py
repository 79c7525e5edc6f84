#!/usr/bin/env python3
"""time_render.py -- the overlay launch (csrc/render.hip) beside a copy of the same bytes, and a group step with and without it.

    python scripts/time_render.py [--frames 256] [--launches 50] [--reps 3] [--steps 8] [--out profiles/r13_render.jsonl]

For 640x480 and 1280x720 BGR frames (--frames of them resident in HBM), each carrying the overlay of 20 tracks with 32-point paths, 20
detections, the count line and one label's counters (686 records a frame), device-event time per launch of
    (a) render         dd_render_draw of all frames
    (b) render_empty   the same launch without a record: the kernel as a copy
    (c) d2d_memcpy     a device-to-device copy of the frames: the floor (both read and write every frame byte once)
alternating, --reps times each, after a warm-up; every figure is events around --launches launches.  (a) includes the check and the
upload of the records (21 952 bytes a frame), as every draw does.  Then one MultiStreamPipeline group of --frames streams of 640x480 with
20 injected detections a stream stepping --steps times, with and without render(streams=range(16)) after every step, alternated
likewise.  One JSON line per figure plus a summary line, appended to --out.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GEOMETRIES = ((640, 480), (1280, 720))
N_OBJ, N_PATH = 20, 32


def overlay_of(r, W, H):
    """20 tracks spread over the frame, each with a 32-point path, their detections, the line and one label's counters."""
    from deepdish_amd import render as rd
    rng = np.random.default_rng(W)
    x0 = rng.uniform(0, W - 80, N_OBJ)
    y0 = rng.uniform(0, H - 160, N_OBJ)
    tlbr = np.stack([x0, y0, x0 + 60, y0 + 150], axis=1)
    steps = np.cumsum(rng.uniform(-6, 6, (N_OBJ, N_PATH, 2)), axis=1)
    paths = np.stack([x0 + 30, y0 + 150], axis=1)[:, None, :] - steps[:, ::-1, :] + steps[:, -1:, :]
    return rd.overlay_primitives(r, [W / 2, 0, W / 2, H], np.arange(1, N_OBJ + 1), ['person'] * N_OBJ, tlbr, paths.reshape(-1, 2), [N_PATH] * N_OBJ,
                                 paths[:2, -2:, :].reshape(-1, 4), tlbr + 1.5, [('person', 12, 34)], 'label')


def kernel_rows(args):
    import torch
    from deepdish_amd._lib import lib, check
    from deepdish_amd.render import Renderer, EMPTY, pack
    from deepdish_amd.runtime import Context
    torch.cuda.set_device(0)
    ctx = Context(0)
    hip = ctypes.CDLL('libamdhip64.so')
    N, n = args.frames, args.launches
    P = ctypes.c_void_p
    rows = []
    for (W, H) in GEOMETRIES:
        src = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device='cuda:0')
        dst = torch.empty_like(src)
        r = Renderer(H, W, context=ctx)
        prims = overlay_of(r, W, H)
        nbytes = N * H * W * 3
        torch.cuda.synchronize()
        streams = np.arange(N, dtype=np.int32)
        packed = {'render': pack([prims] * N), 'render_empty': pack([EMPTY] * N)}      # packed once: the figures are the C call's, not numpy's

        def draw(which):
            recs, off = packed[which]
            check(lib().dd_render_draw(r._h, P(src.data_ptr()), N, P(streams.ctypes.data), N, P(recs.ctypes.data) if len(recs) else P(None),
                                       P(off.ctypes.data), P(dst.data_ptr()), None), 'dd_render_draw')

        calls = {
            'render': lambda: draw('render'),
            'render_empty': lambda: draw('render_empty'),
            'd2d_memcpy': lambda: hip.hipMemcpyAsync(P(dst.data_ptr()), P(src.data_ptr()), ctypes.c_size_t(nbytes), 3, P(ctx.stream_ptr)),
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

        for v in calls:                                           # warm-up: code objects, the record block, clocks
            for _ in range(5):
                calls[v]()
        ctx.sync()
        for rep in range(args.reps):
            for v in calls:                                       # alternating: a drift of the box hits all alike
                ms = timed(calls[v])
                rows.append({'what': v, 'W': W, 'H': H, 'frames': N, 'records_per_frame': len(prims) if v == 'render' else 0, 'rep': rep, 'launches': n,
                             'ms': round(ms, 4), 'bytes_read_plus_written': 2 * nbytes, 'TB_per_s': round(2 * nbytes / ms / 1e9, 3)})
                print(json.dumps(rows[-1]), flush=True)
        del src, dst
    return rows


def pipeline_rows(args):
    import torch
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import Context
    ctx = Context(0)
    S, W, H = args.frames, 640, 480
    frames = [torch.randint(0, 256, (S, H, W, 3), dtype=torch.uint8, device='cuda:0') for _ in range(2)]
    pipes = {opt: MultiStreamPipeline(S, input_size=(W, H), context=ctx) for opt in (False, True)}
    out = torch.empty((16, H, W, 3), dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    count = {False: 0, True: 0}

    def injected(pipe, f):
        k = np.arange(N_OBJ)
        boxes = [(float((20 + 58 * (i % 10) + 5 * f) % 580), float(40 + 200 * (i // 10)), 30.0, 90.0) for i in k]
        return pipe.pack_injected([(boxes, ['person'] * N_OBJ, [0.9] * N_OBJ)] * S)

    def run(opt, steps):
        pipe = pipes[opt]
        for _ in range(steps):
            f = count[opt]
            count[opt] += 1
            pipe.step(frames[f & 1], injected(pipe, f))
            if opt:
                pipe.render(frames[f & 1], streams=range(16), out=out)
        ctx.sync()
        torch.cuda.synchronize()

    rows = []
    for opt in (False, True):
        run(opt, 4)                                               # tracks confirmed, paths begun
    for rep in range(args.reps):
        for opt in (False, True):
            t0 = time.perf_counter()
            run(opt, args.steps)
            ms = 1e3 * (time.perf_counter() - t0) / args.steps
            rows.append({'what': 'pipeline_step', 'render_16_streams': opt, 'streams': S, 'W': W, 'H': H, 'rep': rep, 'steps': args.steps,
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r13_render.jsonl'))
    args = ap.parse_args()
    rows = kernel_rows(args)
    summary = {'what': 'summary', 'frames': args.frames}
    for (W, H) in GEOMETRIES:
        ms = {v: [r['ms'] for r in rows if r['what'] == v and (r['W'], r['H']) == (W, H)] for v in ('render', 'render_empty', 'd2d_memcpy')}
        summary['%dx%d' % (W, H)] = {v: {'ms_min': min(t), 'ms_max': max(t), 'ms_median': float(np.median(t))} for v, t in ms.items()}
        summary['%dx%d' % (W, H)]['render_over_copy'] = round(float(np.median(ms['render'])) / float(np.median(ms['d2d_memcpy'])), 3)
    if not args.no_pipeline:
        rows += pipeline_rows(args)
        for opt in (False, True):
            t = [r['ms_per_step'] for r in rows if r['what'] == 'pipeline_step' and r['render_16_streams'] == opt]
            summary['pipeline_render_%s' % ('on' if opt else 'off')] = {'ms_per_step_min': min(t), 'ms_per_step_max': max(t), 'ms_per_step_median': float(np.median(t))}
    rows.append(summary)
    print(json.dumps(summary), flush=True)
    with open(args.out, 'a') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
