"""What per-stream parameters cost (MultiStreamPipeline(line=, max_age=, max_cosine_distance=, max_iou_distance=, nms_max_overlap= with one
value per stream)): one 1 536-stream worker group of bench.py's workload built with scalars and built with values that alternate between
two settings from stream to stream, so that every step launches nms_small_streams_k and, with association on the device,
assoc_match_streams_k.  Other settings are other work (other boxes kept, other matches, other track counts), so a third pipeline
(`per_stream_eps`) alternates between values that differ in the last digits only -- nms 0.6 / 0.6 + 1e-9, the distances likewise,
max_age 60 / 61: the variants run, the work is the scalar pipeline's.  Each pipeline is stepped with the association decided on the host
and on the device.

One process, the variants interleaved inside each repetition.  Prints one JSON line per measurement and appends them to --out.

    python scripts/time_stream_params.py --out profiles/r23_stream_params.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=1536)
    ap.add_argument('--steps', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--period', type=int, default=8, help='distinct frames per stream resident in HBM')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import bench
    S = args.streams
    cfg = dict(bench.CONFIGS[2])
    model = cfg['model'] + ('-uint8' if bench.DEFAULT_DETECTOR_DTYPE == 'i8' else '')
    W, H = cfg['W'], cfg['H']
    pool = bench.start_gen_pool(1, S)                        # before this process touches the GPU
    os.environ.setdefault('DD_HOST_THREADS', str(bench.host_threads(1, 1)))
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    from deepdish_amd._lib import lib, check
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import Context

    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    dev = torch.empty((args.period, S, H, W, 3), dtype=torch.uint8, device='cuda:0')
    dets = bench.make_inputs_rendered(pool, 0, S, args.period, W, H, [dev], [0, S], 'cuda:0')
    odd = np.arange(S) % 2 == 1
    per_stream = dict(line=np.where(odd[:, None], [0., H / 2, W, H / 2], [W / 2, 0., W / 2, H]),
                      max_age=np.where(odd, 30, 60), max_cosine_distance=np.where(odd, 0.25, 0.2),
                      max_iou_distance=np.where(odd, 0.6, 0.7), nms_max_overlap=np.where(odd, 0.5, 0.6))
    eps = dict(max_age=np.where(odd, 61, 60), max_cosine_distance=np.where(odd, 0.2 + 1e-9, 0.2),
               max_iou_distance=np.where(odd, 0.7 + 1e-9, 0.7), nms_max_overlap=np.where(odd, 0.6 + 1e-9, 0.6))
    # (the order matters and is part of the record: in both runs so far the pipeline built SECOND stepped 1.2-1.4 x slower than the others,
    # whichever settings it had -- README, "Per-stream parameters and reset")
    pipes = {'scalar': MultiStreamPipeline(S, model=model, input_size=(W, H), context=Context(0)),
             'per_stream_eps': MultiStreamPipeline(S, model=model, input_size=(W, H), context=Context(0), **eps),
             'per_stream': MultiStreamPipeline(S, model=model, input_size=(W, H), context=Context(0), **per_stream)}
    inj = {k: [p.pack_injected([dets[s][f] for s in range(S)]) for f in range(args.period)] for k, p in pipes.items()}
    torch.cuda.synchronize()
    variants = [(k, where) for where in ('host', 'device') for k in pipes]

    def run(key, n_steps):
        p = pipes[key]
        for f in range(n_steps):
            a, b = f % args.period, (f + 1) % args.period
            p.step(dev[a], inj[key][a], dev[b] if f + 1 < n_steps else None)

    per = {v: [] for v in variants}
    for rep in range(args.reps):
        for key, where in variants:
            check(lib().dd_pipeline_association(pipes[key]._h, int(where == 'device')), 'dd_pipeline_association')      # between steps
            run(key, args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(key, args.steps)
            ms = 1e3 * (time.perf_counter() - t0) / args.steps
            per[(key, where)].append(ms)
            emit(what='step_ms', variant=key, association=where, streams=S, rep=rep, steps=args.steps, warmup=args.warmup,
                 ms_per_step=round(ms, 4))
    med = {v: statistics.median(t) for v, t in per.items()}
    emit(what='step_ms_median', **{'%s_%s' % v: round(t, 4) for v, t in med.items()},
         **{'%s_%s_range' % v: [round(min(t), 4), round(max(t), 4)] for v, t in per.items()},
         **{'%s_over_scalar_%s' % (k, w): round(med[(k, w)] / med[('scalar', w)], 4) for k in pipes if k != 'scalar' for w in ('host', 'device')},
         stats={k: p.stream_param_stats() for k, p in pipes.items()}, association={k: p.association_stats() for k, p in pipes.items()},
         tracks={k: int(sum(len(p.tracker(z).table()[0]) for z in range(0, S, 64))) for k, p in pipes.items()})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for l in lines:
                f.write(json.dumps(l) + '\n')


if __name__ == '__main__':
    main()
