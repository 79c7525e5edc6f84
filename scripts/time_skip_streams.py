"""What per-stream detector-skip counters cost and buy (MultiStreamPipeline(object_detector_skip_frames=[...], object_detector_skip_phase=[...])):
one 1 536-stream worker group of bench.py's workload, for N = 1 and N = 3, stepped as
  (a) int         the pipeline-wide counter: every stream detects on the same step, none on the next N;
  (b) seq         the sequence form with equal N and no phase: the same schedule through the per-stream path and its store;
  (c) staggered   the sequence form with phase = z mod (N + 1): S / (N + 1) streams detect on every step;
  (d) staggered, every second stream present (a mask; with N = 1 the present streams all have phase 0 and so detect together);
mean and LARGEST step time and frames/s per variant, and feature_rows_carry_k alone (device events, median of seven) beside a
device-to-device copy that moves the same bytes.

The measuring runs in one child process under its own `timeout`, the variants interleaved inside each repetition.  Prints one JSON line
per measurement and appends them to --out.

    python scripts/time_skip_streams.py --out profiles/r20_skip_streams.jsonl
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(args):
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
    half = (np.arange(S) % 2 == 0).astype(np.uint8)
    inj, ctx = None, Context(0)

    def run(p, mask, n_steps, times=None):
        for f in range(n_steps):
            a, b = f % args.period, (f + 1) % args.period
            nxt = dev[b] if f + 1 < n_steps else None
            t0 = time.perf_counter()
            p.step(dev[a], inj[a], nxt, present=mask, present_next=mask if nxt is not None else None)
            if times is not None:
                times.append(1e3 * (time.perf_counter() - t0))

    for N in (1, 3):                                         # the four pipelines of one N live together; those of the other N come after
        phase = [z % (N + 1) for z in range(S)]
        variants = []
        for name, kw, mask in (('int', dict(object_detector_skip_frames=N), None),
                               ('seq', dict(object_detector_skip_frames=[N] * S), None),
                               ('staggered', dict(object_detector_skip_frames=[N] * S, object_detector_skip_phase=phase), None),
                               ('staggered_half', dict(object_detector_skip_frames=[N] * S, object_detector_skip_phase=phase), half)):
            variants.append(('%s_n%d' % (name, N), MultiStreamPipeline(S, model=model, input_size=(W, H), context=ctx, **kw), mask))
        if inj is None:
            inj = [variants[0][1].pack_injected([dets[s][f] for s in range(S)]) for f in range(args.period)]
        torch.cuda.synchronize()
        summary = {v[0]: [] for v in variants}
        for rep in range(args.reps):
            for name, p, mask in variants:
                run(p, mask, args.warmup)
                torch.cuda.synchronize()
                times = []
                run(p, mask, args.steps, times)
                present = int(mask.sum()) if mask is not None else S
                mean, worst = statistics.mean(times), max(times)
                summary[name].append((mean, worst))
                emit(what='step_ms', variant=name, n=N, present=present, rep=rep, steps=args.steps, warmup=args.warmup, mean_ms=round(mean, 4),
                     max_ms=round(worst, 4), min_ms=round(min(times), 4), frames_per_s=round(present * 1e3 / mean, 1))
        for name, p, mask in variants:
            means, worsts = [m for m, _ in summary[name]], [w for _, w in summary[name]]
            present = int(mask.sum()) if mask is not None else S
            emit(what='step_ms_summary', variant=name, n=N, present=present, mean_ms_median=round(statistics.median(means), 4),
                 mean_ms_range=[round(min(means), 4), round(max(means), 4)], max_ms_median=round(statistics.median(worsts), 4),
                 max_ms_range=[round(min(worsts), 4), round(max(worsts), 4)], frames_per_s=round(present * 1e3 / statistics.median(means), 1),
                 skip_stats={k: v for k, v in p.skip_stats().items() if k != 'skipped'})
        del variants, p
        torch.cuda.synchronize()

    # feature_rows_carry_k alone: a staggered N = 3 step of S streams with bench.N_OBJ rows each -- every fourth stream brings fresh rows,
    # the others pair with their retained rows, everything is carried into the next store -- beside a copy that moves the same bytes
    R = int(bench.N_OBJ)
    table, fr, so, o = [], 0, 0, 0
    for z in range(S):
        fresh = z % 4 == 0
        table.append([0 if fresh else 1, fr if fresh else so, R, o, R, o])
        fr, so, o = fr + (R if fresh else 0), so + (0 if fresh else R), o + R
    table = np.ascontiguousarray(table, dtype=np.int32)
    g = torch.Generator(device='cuda:0').manual_seed(1)
    src_f = torch.randn((fr, 128), device='cuda:0', generator=g)
    src_s = torch.randn((so, 128), device='cuda:0', generator=g)
    out, new = torch.zeros((o, 128), device='cuda:0'), torch.zeros((o, 128), device='cuda:0')
    rows_moved = (fr + so) + 2 * o                          # rows read + rows written
    a, b = torch.randn((rows_moved // 2, 128), device='cuda:0', generator=g), torch.empty((rows_moved // 2, 128), device='cuda:0')
    ts = torch.cuda.Stream()
    P = ctypes.c_void_p
    # the entry checks its table on the host before it queues anything: a copy of ~0.5 GB goes in front of each timed interval, so that the
    # stream is still busy while the host prepares and the interval holds device work only (the table's upload and the kernel)
    busy_src, busy_dst = dev[0][:512], torch.empty_like(dev[0][:512])
    torch.cuda.synchronize()
    t_carry, t_copy = [], []
    for it in range(9):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        with torch.cuda.stream(ts):
            busy_dst.copy_(busy_src)
            e[0].record(ts)
            check(lib().dd_feature_rows_carry(ctx.handle, P(src_f.data_ptr()), fr, P(src_s.data_ptr()), so, P(out.data_ptr()), o, P(new.data_ptr()), o,
                                              table.ctypes.data_as(P), S, P(ts.cuda_stream)), 'dd_feature_rows_carry')
            e[1].record(ts)
            busy_dst.copy_(busy_src)
            e[2].record(ts)
            b.copy_(a)
            e[3].record(ts)
        ts.synchronize()
        if it >= 2:                                          # the first two passes warm up
            t_carry.append(e[0].elapsed_time(e[1]))
            t_copy.append(e[2].elapsed_time(e[3]))
    want = torch.empty_like(out)
    sel = torch.from_numpy(table[:, 0]).cuda().bool().repeat_interleave(R)
    want[~sel], want[sel] = src_f, src_s
    ok = bool(torch.equal(out, want)) and bool(torch.equal(new, want))
    c, d = statistics.median(t_carry), statistics.median(t_copy)
    nbytes = rows_moved * 512
    emit(what='carry_vs_copy', streams=S, rows_per_stream=R, rows_read=fr + so, rows_written=2 * o, bytes_moved=nbytes, carry_ms_median=round(c, 4),
         carry_ms_min=round(min(t_carry), 4), copy_ms_median=round(d, 4), copy_ms_min=round(min(t_copy), 4), carry_over_copy=round(c / d, 4),
         carry_GBps=round(nbytes / c / 1e6, 1), copy_GBps=round(nbytes / d / 1e6, 1), results_checked=ok,
         note='the carry interval includes the upload of its %d-entry table; both buffers of either side fit the Infinity Cache' % S)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for l in lines:
                f.write(json.dumps(l) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=1536)
    ap.add_argument('--steps', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--period', type=int, default=8, help='distinct frames per stream resident in HBM')
    ap.add_argument('--limit', type=int, default=900, help='seconds the measuring process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return measure(args)
    cmd = ['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--child'] + sys.argv[1:]
    sys.exit(subprocess.run(cmd, cwd=ROOT).returncode)


if __name__ == '__main__':
    main()
