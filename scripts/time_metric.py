#!/usr/bin/env python3
"""time_metric.py -- one worker group of bench.py's default workload stepped under the cosine and under the euclidean metric.

    python scripts/time_metric.py [--metrics cosine,euclidean] [--steps 20] [--warmup 5] [--streams 1536]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/time_metric.py     # tracker_assoc_k<0> / <1> apart

The workload is one group of bench.py's headline: uint8 SSD-MobileNet-v1 + MARS + deep_sort, 640x480 frames resident in HBM, injected
detections, 1 536 streams stepping with the look-ahead on.  For each metric a fresh MultiStreamPipeline(..., metric=...) is built over
the same frames and timed as bench.py times its steps; the threshold is the default max_cosine_distance for both (the encoder's rows
are unit vectors, so the euclidean metric then admits half the cosine distance).  One JSON line per metric on stdout.  In a kernel
trace the association launches carry the metric in their name (tracker_assoc_k<0> cosine, <1> euclidean), and normalize_rows_k runs
under the cosine metric only.
"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--metrics', default='cosine,euclidean')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--streams', type=int, default=1536)
    args = ap.parse_args()
    cfg = bench.CONFIGS[2]
    W, H, model = cfg['W'], cfg['H'], cfg['model'] + '-uint8'
    pool = bench.start_gen_pool(1, args.streams)              # before anything touches the GPU
    os.environ.setdefault('DD_HOST_THREADS', str(bench.host_threads(1, 1)))
    import torch
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import Context
    torch.cuda.set_device(0)
    n_frames = args.warmup + args.steps
    period = min(n_frames, bench.FRAME_PERIOD)
    bounds = [0, args.streams]
    dev_frames = [torch.empty((period, args.streams, H, W, 3), dtype=torch.uint8, device='cuda:0')]
    dets = bench.make_inputs_rendered(pool, 0, args.streams, period, W, H, dev_frames, bounds, 'cuda:0')
    ctx = Context(0)
    for metric in args.metrics.split(','):
        p = MultiStreamPipeline(args.streams, model=model, input_size=(W, H), context=ctx, metric=metric)
        injected = [p.pack_injected([dets[s][f] for s in range(args.streams)]) for f in range(period)]

        def run(f0, f1):
            for f in range(f0, f1):
                p.step(dev_frames[0][f % period], injected[f % period], dev_frames[0][(f + 1) % period] if f + 1 < f1 else None)
            torch.cuda.synchronize()

        run(0, args.warmup)
        t0 = time.perf_counter()
        run(args.warmup, n_frames)
        dt = time.perf_counter() - t0
        sm = p.stage_ms()
        live = sum(len(p.tracker(z).table()[0]) for z in range(0, args.streams, max(1, args.streams // 64)))
        print(json.dumps({'metric': metric, 'frames_per_s': args.steps * args.streams / dt, 'ms_per_step': 1e3 * dt / args.steps,
                          'steps': args.steps, 'warmup': args.warmup, 'streams': args.streams, 'groups': 1, 'model': model,
                          'stage_ms_per_step': {k: round(float(sm[k]), 4) for k in ('objd', 'nms', 'feat', 'trak', 'host', 'wall')},
                          'live_tracks_in_64_sampled_streams': live, 'counts_pos_neg_int_del': p.counts().sum(axis=(0, 1)).tolist()}),
              flush=True)
        del p, injected
        gc.collect()
        torch.cuda.synchronize()


if __name__ == '__main__':
    main()
