#!/usr/bin/env python3
"""time_topdown.py -- the ground-plane launch (csrc/ground.hip) beside a copy of the same bytes, and the overlay launch with and without
the top-down panel.

    python scripts/time_topdown.py [--points 2097152] [--cameras 3072] [--frames 256] [--launches 50] [--point-launches 2000] [--reps 3] [--out profiles/r17_topdown.jsonl]

Device-event time per launch, alternating, --reps times each, after a warm-up; every figure is events around --launches launches of
(c) and (d) and --point-launches launches of (a) and (b), which take microseconds each:
    (a) ground_points   dd_ground_from_image on device arrays: --points points (f64 [n][2], 32 MB at the default) over --cameras cameras,
                        a stream's points behind one another (the index is uniform in runs of points / cameras)
    (b) d2d_memcpy      a device-to-device copy of the points: the floor for reading and writing 16 bytes a point (the kernel reads four
                        bytes of index a point on top)
    (c) render_panel    dd_render_draw of --frames 640x480 frames, each with the overlay of 20 tracks with 32-point paths, 20 detections, the
                        line, one label's counters AND the top-down panel with 20 markers and ground paths
    (d) render          the same without the panel
The arrays of (a) and (b), 72 MB together, stay in the 256 MiB last-level cache from one launch to the next: these are not HBM figures.
(c) and (d) include the check and the upload of the records, as every draw does.  One JSON line per figure plus a summary line, appended
to --out.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H = 640, 480
N_OBJ, N_PATH = 20, 32


def overlays(r, cam):
    """time_render.py's scene (20 tracks with 32-point paths, their detections, the line, one label's counters), with and without the panel."""
    from deepdish_amd import render as rd
    rng = np.random.default_rng(W)
    x0 = rng.uniform(0, W - 80, N_OBJ)
    y0 = rng.uniform(120, H - 160, N_OBJ)
    tlbr = np.stack([x0, y0, x0 + 60, y0 + 150], axis=1)
    steps = np.cumsum(rng.uniform(-6, 6, (N_OBJ, N_PATH, 2)), axis=1)
    paths = (np.stack([x0 + 30, y0 + 150], axis=1)[:, None, :] - steps[:, ::-1, :] + steps[:, -1:, :]).reshape(-1, 2)
    args = (r, [W / 2, 0, W / 2, H], np.arange(1, N_OBJ + 1), ['person'] * N_OBJ, tlbr, paths, [N_PATH] * N_OBJ, paths.reshape(N_OBJ, N_PATH, 2)[:2, -2:, :].reshape(-1, 4),
            tlbr + 1.5, [('person', 12, 34)], 'label')
    scale = np.array([W / 4, H / 4]) / np.array([20.0, 10.0])
    return {'render': rd.overlay_primitives(*args), 'render_panel': rd.overlay_primitives(*args, topdown=(W / 4, H / 4, cam.space_from_image(paths), scale))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=2 * 1024 * 1024)
    ap.add_argument('--cameras', type=int, default=3072)
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--point-launches', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r17_topdown.jsonl'))
    args = ap.parse_args()
    import torch
    from deepdish_amd._lib import lib, check
    from deepdish_amd.ground import GroundPlane
    from deepdish_amd.render import Renderer, pack
    from deepdish_amd.runtime import Context
    torch.cuda.set_device(0)
    ctx = Context(0)
    hip = ctypes.CDLL('libamdhip64.so')
    P = ctypes.c_void_p
    n, n_launch = args.points, args.launches

    rng = np.random.default_rng(17)
    table = GroundPlane.stack([GroundPlane(3.6, sensor_mm=(6.17, 4.55), image=(W, H), elevation_m=float(rng.uniform(2.5, 8.0)), tilt_deg=float(rng.uniform(30.0, 75.0)),
                                           roll_deg=float(rng.uniform(-5.0, 5.0)), context=ctx) for _ in range(args.cameras)], context=ctx)
    d_table = ctx.to_device(table.table)
    d_pts = ctx.to_device(np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], axis=1))
    d_idx = ctx.to_device((np.arange(n, dtype=np.int64) * args.cameras // n).astype(np.int32))
    d_out = torch.empty_like(d_pts)
    src = torch.randint(0, 256, (args.frames, H, W, 3), dtype=torch.uint8, device='cuda:0')
    dst = torch.empty_like(src)
    r = Renderer(H, W, context=ctx, records=2)
    prims = overlays(r, table)
    packed = {k: pack([v] * args.frames) for k, v in prims.items()}      # packed once: the figures are the C call's, not numpy's
    streams = np.arange(args.frames, dtype=np.int32)
    torch.cuda.synchronize()

    def ground():
        check(lib().dd_ground_from_image(ctx.handle, P(d_table.data_ptr()), args.cameras, P(d_idx.data_ptr()), P(d_pts.data_ptr()), n, P(d_out.data_ptr()), 1, None),
              'dd_ground_from_image')

    def draw(which):
        recs, off = packed[which]
        check(lib().dd_render_draw(r._h, P(src.data_ptr()), args.frames, P(streams.ctypes.data), args.frames, P(recs.ctypes.data), P(off.ctypes.data),
                                   P(dst.data_ptr()), None), 'dd_render_draw')

    calls = {
        'ground_points': ground,
        'd2d_memcpy': lambda: hip.hipMemcpyAsync(P(d_out.data_ptr()), P(d_pts.data_ptr()), ctypes.c_size_t(16 * n), 3, P(ctx.stream_ptr)),
        'render_panel': lambda: draw('render_panel'),
        'render': lambda: draw('render'),
    }

    def timed(fn, n_launch):
        with torch.cuda.stream(ctx.torch_stream):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n_launch):
                fn()
            e1.record()
        ctx.sync()
        return e0.elapsed_time(e1) / n_launch                     # ms per launch

    for v in calls:                                               # warm-up: code objects, the record block, clocks
        for _ in range(5):
            calls[v]()
    ctx.sync()
    rows = []
    for rep in range(args.reps):
        for v in calls:                                           # alternating: a drift of the box hits all alike
            k = args.point_launches if v in ('ground_points', 'd2d_memcpy') else n_launch
            ms = timed(calls[v], k)
            row = {'what': v, 'rep': rep, 'launches': k, 'ms': round(ms, 5)}
            if v in ('ground_points', 'd2d_memcpy'):
                row.update(points=n, cameras=args.cameras, bytes_read_plus_written=32 * n, TB_per_s=round(32 * n / ms / 1e9, 3))
            else:
                row.update(W=W, H=H, frames=args.frames, records_per_frame=len(prims[v]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    summary = {'what': 'summary', 'points': n, 'cameras': args.cameras, 'frames': args.frames}
    for v in calls:
        t = [r_['ms'] for r_ in rows if r_['what'] == v]
        summary[v] = {'ms_min': min(t), 'ms_max': max(t), 'ms_median': float(np.median(t))}
    summary['ground_over_copy'] = round(summary['ground_points']['ms_median'] / summary['d2d_memcpy']['ms_median'], 3)
    summary['panel_over_plain'] = round(summary['render_panel']['ms_median'] / summary['render']['ms_median'], 3)
    rows.append(summary)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as fh:
        for r_ in rows:
            fh.write(json.dumps(r_) + '\n')


if __name__ == '__main__':
    main()
