#!/usr/bin/env python3
"""time_skip_frames.py -- bench.py's default configuration run with --object-detector-skip-frames N.

    python scripts/time_skip_frames.py [--ns 0,1,3] [--steps 20] [--warmup 5] [--split-steps 8] [--streams 3072] [--groups 2]

The workload is bench.py's headline: uint8 SSD-MobileNet-v1 + MARS + deep_sort, 640x480 frames resident in HBM, injected detections,
two worker groups of 1 536 streams, each stepping in its own thread with the look-ahead on.  For each N a fresh set of pipelines is
built with MultiStreamPipeline(..., object_detector_skip_frames=N) (the schedule counts from the first warm-up step) and timed as
bench.py times its steps.  A second pass of --split-steps steps then reads stage_ms() after every step of group 0 and reports the GPU
stage milliseconds and the host milliseconds of detector steps and skip steps apart (those reads wait for the step's last events, so
this pass is not the timed one).  One JSON line per N on stdout.
"""
import argparse
import gc
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ns', default='0,1,3', help='comma-separated values of N')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--split-steps', type=int, default=8)
    ap.add_argument('--streams', type=int, default=3072)
    ap.add_argument('--groups', type=int, default=2)
    args = ap.parse_args()
    ns = [int(v) for v in args.ns.split(',')]
    cfg = bench.CONFIGS[2]
    W, H, model = cfg['W'], cfg['H'], cfg['model'] + '-uint8'
    G = args.groups
    pool = bench.start_gen_pool(1, args.streams)              # before anything touches the GPU
    os.environ.setdefault('DD_HOST_THREADS', str(bench.host_threads(1, G)))
    import torch
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import Context
    torch.cuda.set_device(0)
    n_frames = args.warmup + args.steps + args.split_steps
    period = min(n_frames, bench.FRAME_PERIOD)
    bounds = [round(g * args.streams / G) for g in range(G + 1)]
    dev_frames = [torch.empty((period, bounds[g + 1] - bounds[g], H, W, 3), dtype=torch.uint8, device='cuda:0') for g in range(G)]
    dets = bench.make_inputs_rendered(pool, 0, args.streams, period, W, H, dev_frames, bounds, 'cuda:0')
    ctxs = [Context(0) for _ in range(G)]

    for n in ns:
        pipes = [MultiStreamPipeline(bounds[g + 1] - bounds[g], model=model, input_size=(W, H), context=ctxs[g],
                                     object_detector_skip_frames=n) for g in range(G)]
        injected = [[pipes[g].pack_injected([dets[s][f] for s in range(bounds[g], bounds[g + 1])]) for f in range(period)]
                    for g in range(G)]
        split = {True: [], False: []}                           # detector step? -> per-step stage deltas of group 0

        def run(g, f0, f1, record):
            torch.cuda.set_device(0)
            p = pipes[g]
            last = None
            for f in range(f0, f1):
                p.step(dev_frames[g][f % period], injected[g][f % period], dev_frames[g][(f + 1) % period] if f + 1 < f1 else None)
                if record:
                    sm = p.stage_ms()
                    tot = {k: sm[k] * sm['steps'] for k in ('objd', 'nms', 'feat', 'trak', 'host', 'wall')}
                    if last is not None:
                        det_step = n <= 0 or f % (n + 1) == 0
                        split[det_step].append({k: tot[k] - last[k] for k in tot})
                    last = tot

        def all_groups(f0, f1, record=False):
            th = [threading.Thread(target=run, args=(g, f0, f1, record and g == 0)) for g in range(G)]
            for t in th:
                t.start()
            for t in th:
                t.join()
            torch.cuda.synchronize()

        all_groups(0, args.warmup)
        t0 = time.perf_counter()
        all_groups(args.warmup, args.warmup + args.steps)
        dt = time.perf_counter() - t0
        # the first step of this pass only sets the baseline of the deltas
        all_groups(args.warmup + args.steps, n_frames, record=True)
        out = {'object_detector_skip_frames': n, 'frames_per_s': args.steps * args.streams / dt, 'ms_per_step': 1e3 * dt / args.steps,
               'steps': args.steps, 'warmup': args.warmup, 'streams': args.streams, 'groups': G, 'model': model,
               'stage_ms_per_step_group0': {}}
        for det_step, rows in split.items():
            if rows:
                out['stage_ms_per_step_group0']['detector_steps' if det_step else 'skip_steps'] = dict(
                    {k: round(float(np.mean([r[k] for r in rows])), 4) for k in rows[0]}, count=len(rows))
        print(json.dumps(out), flush=True)
        del pipes, injected
        gc.collect()
        torch.cuda.synchronize()


if __name__ == '__main__':
    main()
