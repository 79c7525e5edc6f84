"""What a masked step costs (MultiStreamPipeline.step(..., present=)): one 1 536-stream worker group of bench.py's workload stepped with
present=None, an all-ones mask, every second and every fourth stream, beside pipelines BUILT with 768 and 384 streams; and
frames_gather_k alone beside a device-to-device copy of the same bytes (768 of 1 536 frames), timed with device events.

One process, the variants interleaved inside each repetition.  Prints one JSON line per measurement and appends them to --out.

    python scripts/time_present.py --out profiles/r19_present.jsonl
"""
import argparse
import ctypes
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
    sizes = {'pipe%d' % S: S, 'pipe%d' % (S // 2): S // 2, 'pipe%d' % (S // 4): S // 4}
    pipes = {k: MultiStreamPipeline(n, model=model, input_size=(W, H), context=Context(0)) for k, n in sizes.items()}
    inj = {k: [p.pack_injected([dets[s][f] for s in range(p.S)]) for f in range(args.period)] for k, p in pipes.items()}
    torch.cuda.synchronize()
    full = 'pipe%d' % S
    masks = {'none': None, 'ones': np.ones(S, np.uint8), 'every2nd': (np.arange(S) % 2 == 0).astype(np.uint8),
             'every4th': (np.arange(S) % 4 == 0).astype(np.uint8)}
    variants = [(m, full, masks[m]) for m in masks] + [(k, k, None) for k in sizes if k != full]

    def run(pipe_key, mask, n_steps):
        p = pipes[pipe_key]
        for f in range(n_steps):
            a, b = f % args.period, (f + 1) % args.period
            nxt = dev[b][:p.S] if f + 1 < n_steps else None
            p.step(dev[a][:p.S], inj[pipe_key][a], nxt, present=mask, present_next=mask if nxt is not None else None)

    per = {v[0]: [] for v in variants}
    for rep in range(args.reps):
        for name, key, mask in variants:
            run(key, mask, args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(key, mask, args.steps)
            ms = 1e3 * (time.perf_counter() - t0) / args.steps
            per[name].append(ms)
            emit(what='step_ms', variant=name, pipeline_streams=pipes[key].S, present=int(mask.sum()) if mask is not None else pipes[key].S,
                 rep=rep, steps=args.steps, warmup=args.warmup, ms_per_step=round(ms, 4))
    med = {k: statistics.median(v) for k, v in per.items()}
    emit(what='step_ms_median', **{k: round(v, 4) for k, v in med.items()},
         ones_over_none=round(med['ones'] / med['none'], 4),
         every2nd_over_half_pipeline=round(med['every2nd'] / med['pipe%d' % (S // 2)], 4),
         every4th_over_quarter_pipeline=round(med['every4th'] / med['pipe%d' % (S // 4)], 4),
         present_stats=pipes[full].present_stats())

    # frames_gather_k against the copy floor: every second of S frames, on one stream between device events
    ctx = pipes[full].ctx
    ts = torch.cuda.Stream()
    idx = np.ascontiguousarray(np.arange(0, S, 2), dtype=np.int32)
    n, fb = len(idx), H * W * 3
    dst = torch.empty((n, H, W, 3), dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    t_gather, t_copy = [], []
    for it in range(9):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        with torch.cuda.stream(ts):
            e[0].record(ts)
            check(lib().dd_gather_frames(ctx.handle, ctypes.c_void_p(dev[0].data_ptr()), S, fb, idx.ctypes.data_as(ctypes.c_void_p), n,
                                         ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(ts.cuda_stream)), 'dd_gather_frames')
            e[1].record(ts)
            e[2].record(ts)
            dst.copy_(dev[1][:n])
            e[3].record(ts)
        ts.synchronize()
        if it >= 2:                                          # the first two passes warm up
            t_gather.append(e[0].elapsed_time(e[1]))
            t_copy.append(e[2].elapsed_time(e[3]))
    ok = bool(torch.equal(dst, dev[1][:n]))
    check(lib().dd_gather_frames(ctx.handle, ctypes.c_void_p(dev[0].data_ptr()), S, fb, idx.ctypes.data_as(ctypes.c_void_p), n,
                                 ctypes.c_void_p(dst.data_ptr()), None), 'dd_gather_frames')
    ctx.sync()
    ok = ok and bool(torch.equal(dst, dev[0][::2]))
    g, c = statistics.median(t_gather), statistics.median(t_copy)
    emit(what='gather_vs_copy', frames=n, of=S, bytes_moved=2 * n * fb, gather_ms_median=round(g, 4), gather_ms_min=round(min(t_gather), 4),
         copy_ms_median=round(c, 4), copy_ms_min=round(min(t_copy), 4), gather_over_copy=round(g / c, 4),
         gather_GBps=round(2 * n * fb / g / 1e6, 1), copy_GBps=round(2 * n * fb / c / 1e6, 1), results_checked=ok,
         note='the gather interval includes the upload of its %d-int index list' % n)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for l in lines:
                f.write(json.dumps(l) + '\n')


if __name__ == '__main__':
    main()
