#!/usr/bin/env python3
"""time_association.py -- one worker group of bench.py's default workload stepped with the association decided on the host and on the device.

    python scripts/time_association.py [--streams 1536] [--associations host,device] [--reps 3] [--steps 10] [--warmup 5] [--out FILE]

profiles/r11_association.jsonl was recorded with exactly these four commands, in this order (the defaults are the recorded settings):

    python scripts/time_association.py --streams 1536
    python scripts/time_association.py --streams 8
    python scripts/time_association.py --streams 1
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/time_association.py --streams 1536 --associations device --reps 1 --out /dev/null
    python scripts/time_association.py --kernel-stats OUT --streams 1536      # assoc_match_k's time out of that trace, appended as one more line

The workload is one group of bench.py's headline (scripts/time_metric.py's): uint8 SSD-MobileNet-v1 + MARS + deep_sort, 640x480 frames
resident in HBM, injected detections, the look-ahead on.  For each setting one MultiStreamPipeline(..., association=...) is built over the
same frames, warmed up, and timed --reps times over --steps steps each, both settings in this one process.  One JSON line per setting and
repetition, appended to --out (profiles/r11_association.jsonl) and printed: ms per step, the stage table (GPU milliseconds per stage,
`host`, `wall`, and `host_wall`, the host-side stopwatch whose `trak` is what the host waits and works through the tracker update), the bytes
per step the decisions copied device-to-host, and the group's association counters.  The kernel's own time comes from a kernel trace taken
in a run of its own (the rocprofv3 command; `--output-format csv` is what --kernel-stats reads): tracing slows the host side, so that run's
step times are not recorded.
"""
import argparse
import csv
import gc
import glob
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def emit(path, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if path and path != '/dev/null':
        with open(path, 'a') as f:
            f.write(line + '\n')


def kernel_stats(args):
    rows = {}
    for fn in glob.glob(os.path.join(args.kernel_stats, '**', '*kernel_stats.csv'), recursive=True):
        for r in csv.DictReader(open(fn)):
            if 'assoc_match_k' in r['Name'] or 'tracker_assoc_k' in r['Name'] or 'tracker_apply_k' in r['Name']:
                rows[re.search(r'(\w+_k(<\d+>)?)\(', r['Name']).group(1)] = dict(calls=int(r['Calls']), average_us=float(r['AverageNs']) / 1e3,
                                                      min_us=float(r['MinNs']) / 1e3, max_us=float(r.get('MaxNs') or 'nan') / 1e3)
    emit(args.out, {'kernel_trace': rows, 'streams': args.streams, 'association': 'device'})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--associations', default='host,device')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--streams', type=int, default=1536)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r11_association.jsonl'))
    ap.add_argument('--kernel-stats', default=None, help='directory of a rocprofv3 --kernel-trace --stats run of this script: record its kernel times')
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args)
    cfg = bench.CONFIGS[2]
    W, H, model = cfg['W'], cfg['H'], cfg['model'] + '-uint8'
    pool = bench.start_gen_pool(1, args.streams)              # before anything touches the GPU
    os.environ.setdefault('DD_HOST_THREADS', str(bench.host_threads(1, 1)))
    import torch
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import Context
    from deepdish_amd.deep_sort.tracker import _association_stats
    torch.cuda.set_device(0)
    n_frames = args.warmup + args.reps * args.steps
    period = min(n_frames, bench.FRAME_PERIOD)
    bounds = [0, args.streams]
    dev_frames = [torch.empty((period, args.streams, H, W, 3), dtype=torch.uint8, device='cuda:0')]
    dets = bench.make_inputs_rendered(pool, 0, args.streams, period, W, H, dev_frames, bounds, 'cuda:0')
    ctx = Context(0)
    for assoc in args.associations.split(','):
        p = MultiStreamPipeline(args.streams, model=model, input_size=(W, H), context=ctx, association=assoc)
        injected = [p.pack_injected([dets[s][f] for s in range(args.streams)]) for f in range(period)]

        def run(f0, f1):
            for f in range(f0, f1):
                p.step(dev_frames[0][f % period], injected[f % period], dev_frames[0][(f + 1) % period] if f + 1 < f1 else None)
            torch.cuda.synchronize()

        run(0, args.warmup)
        h0 = p.tracker(0)._h
        for rep in range(args.reps):
            f0 = args.warmup + rep * args.steps
            before, b0 = p.stage_ms(), _association_stats(h0, d2h_bytes=True)
            t0 = time.perf_counter()
            run(f0, f0 + args.steps)
            dt = time.perf_counter() - t0
            after, b1 = p.stage_ms(), _association_stats(h0, d2h_bytes=True)

            def per_step(get):          # the stage table is cumulative over the pipeline's steps: this repetition's share
                return round(float((get(after) * after['steps'] - get(before) * before['steps']) / args.steps), 4)
            emit(args.out, {'association': assoc, 'rep': rep, 'streams': args.streams, 'steps': args.steps, 'warmup': args.warmup,
                            'model': model, 'groups': 1, 'ms_per_step': round(1e3 * dt / args.steps, 4),
                            'frames_per_s': round(args.steps * args.streams / dt, 1),
                            'stage_ms_per_step': {k: per_step(lambda s, k=k: s[k]) for k in ('objd', 'nms', 'feat', 'trak', 'host', 'wall')},
                            'host_wall_ms_per_step': {k: per_step(lambda s, k=k: s['host_wall'][k]) for k in ('objd', 'nms', 'feat', 'trak')},
                            'assoc_d2h_bytes_per_step': (b1 - b0) // args.steps,
                            'association_stats': p.association_stats(),
                            'counts_pos_neg_int_del': p.counts().sum(axis=(0, 1)).tolist()})
        del p, injected
        gc.collect()
        torch.cuda.synchronize()


if __name__ == '__main__':
    main()
