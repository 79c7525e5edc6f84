"""What the motion gate costs and buys (MultiStreamPipeline(motion_gate=0)): one worker group of bench.py's background-subtraction
workload (bench.py --background-subtraction 0.25 --streams 768 runs two groups of 384), with a share f = 0, 0.5, 0.9, 1.0 of the
streams showing an unchanging picture (their first frame, every step), stepped as
  (a) off          no gate, frames_next given: the look-ahead detector run overlaps the step;
  (b) off_nolook   the same pipeline without frames_next: what losing the look-ahead alone costs;
  (c) gate         motion_gate=0, frames_next given (a gated pipeline queues nothing ahead);
mean, smallest and largest step time per repetition, the variants interleaved inside each repetition, every stream reset before each
share so that MOG2 starts over.  A third, ungated pipeline is built first and discarded, so that neither measured one is the second
built.  Then mask_stream_count_k over the group's mask planes through dd_mask_stream_count (device events around the call: memset,
kernel, the copy of the counts and the host's wake-up) beside a device-to-device copy of the same mask bytes.

The measuring runs in one child process under its own `timeout`.  Prints one JSON line per measurement and appends them to --out.

    python scripts/time_motion_gate.py --out profiles/r27_motion_gate.jsonl
"""
import argparse
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
    from deepdish_amd.background import mask_stream_count
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import Context

    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    moving = torch.empty((args.period, S, H, W, 3), dtype=torch.uint8, device='cuda:0')
    dets = bench.make_inputs_rendered(pool, 0, S, args.period, W, H, [moving], [0, S], 'cuda:0')
    dev = torch.empty_like(moving)
    ctx = Context(0)
    kw = dict(model=model, input_size=(W, H), context=ctx, background_subtraction_ratio=args.ratio)
    first = MultiStreamPipeline(S, **kw)                     # built first and discarded: neither measured pipeline is "the second built"
    inj = [first.pack_injected([dets[s][f] for s in range(S)]) for f in range(args.period)]
    first.step(moving[0], inj[0])
    torch.cuda.synchronize()
    del first
    off, gate = MultiStreamPipeline(S, **kw), MultiStreamPipeline(S, motion_gate=0, **kw)
    variants = (('off', off, True), ('off_nolook', off, False), ('gate', gate, True))

    def run(p, look, n_steps, times=None):
        for f in range(n_steps):
            a, b = f % args.period, (f + 1) % args.period
            nxt = dev[b] if look and f + 1 < n_steps else None
            t0 = time.perf_counter()
            p.step(dev[a], inj[a], nxt)
            if times is not None:
                times.append(1e3 * (time.perf_counter() - t0))

    for share in args.shares:
        n_still = int(round(share * S))
        dev.copy_(moving)
        if n_still:
            dev[:, :n_still] = moving[0:1, :n_still]         # an unchanging picture: the stream's first frame, every step
        torch.cuda.synchronize()
        summary = {v[0]: [] for v in variants}
        for p in (off, gate):
            p.reset(range(S))                                # MOG2, trackers and counters start over for this share
        for rep in range(args.reps):
            for name, p, look in variants:
                g0, s0 = p.gate_stats(), p.skip_stats()
                run(p, look, args.warmup)
                torch.cuda.synchronize()
                times = []
                run(p, look, args.steps, times)
                g1, s1 = p.gate_stats(), p.skip_stats()
                mean = statistics.mean(times)
                summary[name].append(mean)
                emit(what='step_ms', share_still=share, streams_still=n_still, variant=name, rep=rep, steps=args.steps, warmup=args.warmup,
                     mean_ms=round(mean, 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4), frames_per_s=round(S * 1e3 / mean, 1),
                     gated_stream_steps=g1['gated_stream_steps'] - g0['gated_stream_steps'],
                     detector_stream_steps=s1['detector_stream_steps'] - s0['detector_stream_steps'], stream_steps=S * (args.steps + args.warmup))
        for name, p, look in variants:
            m = summary[name]
            emit(what='step_ms_summary', share_still=share, variant=name, mean_ms_median=round(statistics.median(m), 4),
                 mean_ms_range=[round(min(m), 4), round(max(m), 4)], frames_per_s=round(S * 1e3 / statistics.median(m), 1))
        lo_g, hi_o = min(summary['gate']), max(summary['off'])
        emit(what='gate_vs_off', share_still=share, gate_over_off=round(statistics.median(summary['gate']) / statistics.median(summary['off']), 4),
             ranges_overlap=bool(lo_g <= hi_o and min(summary['off']) <= max(summary['gate'])),
             gate_wholly_above_off=bool(lo_g > hi_o), gate_wholly_below_off=bool(max(summary['gate']) < min(summary['off'])))

    # mask_stream_count_k alone over the group's planes beside a device-to-device copy of the same bytes
    mask = torch.from_numpy(np.random.default_rng(1).choice(np.array([0, 127, 255], np.uint8), size=(S, H, W), p=[0.9, 0.03, 0.07])).cuda()
    want = [int(v) for v in (mask != 0).sum(dim=(1, 2)).cpu()]
    dst = torch.empty_like(mask)
    busy_src, busy_dst = moving[0][:256], torch.empty_like(moving[0][:256])
    ts = ctx.torch_stream                                    # the entry runs on its context's stream
    torch.cuda.synchronize()
    t_count, t_copy, ok = [], [], True
    for it in range(9):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        with torch.cuda.stream(ts):
            busy_dst.copy_(busy_src)                         # keeps the stream busy while the host prepares: the interval holds device work
            e[0].record(ts)
            got = mask_stream_count(mask, context=ctx)
            e[1].record(ts)
            busy_dst.copy_(busy_src)
            e[2].record(ts)
            dst.copy_(mask)
            e[3].record(ts)
        ts.synchronize()
        ok = ok and got.tolist() == want
        if it >= 2:                                          # the first two passes warm up
            t_count.append(e[0].elapsed_time(e[1]))
            t_copy.append(e[2].elapsed_time(e[3]))
    c, d = statistics.median(t_count), statistics.median(t_copy)
    nbytes = S * H * W
    emit(what='count_vs_copy', streams=S, mask_bytes=nbytes, count_ms_median=round(c, 4), count_ms_min=round(min(t_count), 4),
         copy_ms_median=round(d, 4), copy_ms_min=round(min(t_copy), 4), count_GBps_read=round(nbytes / c / 1e6, 1),
         copy_GBps_read_plus_written=round(2 * nbytes / d / 1e6, 1), results_checked=bool(ok),
         note='the count interval holds the memset of the counters, the kernel, the copy of %d counts to the host and the host wake-up of '
              'the entry\'s synchronise; the mask fits the Infinity Cache' % S)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for l in lines:
                f.write(json.dumps(l) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=384)
    ap.add_argument('--ratio', type=float, default=0.25)
    ap.add_argument('--shares', type=float, nargs='+', default=[0.0, 0.5, 0.9, 1.0])
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
