#!/usr/bin/env python3
"""time_mars_sizes.py -- the MARS encoder at the three crop sizes the reference ships (64x32, 128x64, 256x128).

    python scripts/time_mars_sizes.py SIZE CROPS [--reps 20] [--warmup 5] [--runs 3] [--jsonl FILE] [--tag TEXT]
    python scripts/time_mars_sizes.py sweep SIZE [--counts 8,16,...] [--reps 20]

One configuration per process: DD_STEM_WIDE=1 for the one-launch front of the larger sizes, DD_STEM_WIDE=0 (the default dispatch until
the kernel has been priced) for the three launches.  Per run: `warmup` untimed forwards, then `reps` forwards bracketed by HIP events on the launch stream (whole-forward time), then
`reps` forwards with the engine's per-op events on, from which the FRONT of the network -- everything up to and including the first max
pool: conv1_1, conv1_2, pool -- is summed.  `runs` repeats of that in one process give the run-to-run spread.  One JSON line per
process on stdout (and appended to --jsonl): mean / min / max over runs of the per-run means, the engine's activation bytes, the
launches that ran, and a digest of the pooled tensor and of the features (sha, for A/B comparisons of the bits).

The script also runs on a checkout without sized synthetic weights (it then builds an fc1 of the right shape itself, as
tests/test_gpu_nets.py does): that is how the parent commit's front is priced at 128 x 64.

`sweep` runs SIZE at each crop count twice in child processes -- fused from one crop (DD_STEM_WIDE=1 DD_STEM_WIDE_MIN=1) and DD_STEM_WIDE=0 -- and prints
the front times side by side: the crossover is the engine's threshold.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def weights(hw):
    from deepdish_amd import nets
    try:
        return nets.synthetic_mars_weights(1234, hw)
    except TypeError:                                         # a checkout with 64 x 32 weights only
        wd = nets.synthetic_mars_weights(1234)
        k = (hw[0] // 8) * (hw[1] // 8) * 128
        wd['fc1/weights'] = (np.random.default_rng(5).standard_normal((k, 128)) * np.sqrt(2.0 / k)).astype(np.float32)
        return wd


def measure(args):
    import torch
    from deepdish_amd import nets
    from deepdish_amd.engine import Net
    from deepdish_amd._lib import lib, check
    from deepdish_amd.profile import net_op_times, net_op_launches, OPK_NAMES
    hw = tuple(int(v) for v in args.size.split('x')[:2])
    n = args.crops
    prog = nets.compile_mars(weights(hw), *hw)
    net = Net(prog, max_batch=n, shared=args.shared)
    x = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (n,) + hw + (3,), dtype=np.uint8)).cuda()
    ts = net.ctx.torch_stream
    pool_t = prog.meta['tensors']['pool1']
    front_ops = 1 + max(i for i, op in enumerate(prog.ops) if op[2] == pool_t)
    fwd, front = [], []
    for _ in range(args.runs):
        for _ in range(args.warmup):
            net.forward(x)
        net.ctx.sync()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
        ev[0].record(ts)
        for r in range(args.reps):
            net.forward(x)
            ev[r + 1].record(ts)
        net.ctx.sync()
        fwd.append(float(np.mean([ev[r].elapsed_time(ev[r + 1]) for r in range(args.reps)])))
        check(lib().dd_net_profile(net._h, 1), 'dd_net_profile')
        acc = 0.0
        for r in range(args.reps + 2):
            net.forward(x)
            net.ctx.sync()
            if r >= 2:
                acc += float(np.sum(net_op_times(net)[:front_ops]))
        check(lib().dd_net_profile(net._h, 0), 'dd_net_profile')
        front.append(acc / args.reps)
    net.forward(x)
    net.ctx.sync()
    feats = net.read()
    sha = hashlib.sha256(np.ascontiguousarray(feats).tobytes())
    sha_pool = None
    if not args.shared:                                       # an engine with overlaid buffers reads its output only
        sha_pool = hashlib.sha256(np.ascontiguousarray(net.read(tensor=pool_t)).tobytes()).hexdigest()[:16]
    out = dict(size='%dx%d' % hw, crops=n, reps=args.reps, runs=args.runs, tag=args.tag,
               forward_ms=dict(mean=float(np.mean(fwd)), min=float(np.min(fwd)), max=float(np.max(fwd))),
               front_ms=dict(mean=float(np.mean(front)), min=float(np.min(front)), max=float(np.max(front))),
               front_ops=front_ops, engine_activation_gb=net.activation_bytes() / 1e9, shared=bool(args.shared),
               launches=sorted({OPK_NAMES[int(c)] for c in net_op_launches(net) if int(c) in OPK_NAMES}),
               switches={k: v for k, v in os.environ.items() if k.startswith('DD_STEM')},
               sha_pool=sha_pool, sha=sha.hexdigest()[:16])
    line = json.dumps(out)
    print(line)
    print('sha %s' % out['sha'])
    if args.jsonl:
        with open(args.jsonl, 'a') as f:
            f.write(line + '\n')


def sweep(args):
    print('%s: crops  front ms fused (min..max)  front ms three launches (min..max)  ratio' % args.size)
    for n in (int(v) for v in args.counts.split(',')):
        res = []
        for env in ({'DD_STEM_WIDE': '1', 'DD_STEM_WIDE_MIN': '1'}, {'DD_STEM_WIDE': '0'}):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), args.size, str(n), '--reps', str(args.reps), '--runs', str(args.runs)],
                               capture_output=True, text=True, env=dict(os.environ, **env), timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                sys.exit(r.returncode)                        # nothing more is started after a failed run
            res.append(json.loads(r.stdout.splitlines()[0]))
        a, b = res[0]['front_ms'], res[1]['front_ms']
        assert res[0]['sha_pool'] == res[1]['sha_pool'] and res[0]['sha'] == res[1]['sha'], (n, res)
        print('%6d  %8.4f (%.4f..%.4f)  %8.4f (%.4f..%.4f)  %.2f' % (n, a['mean'], a['min'], a['max'], b['mean'], b['min'], b['max'], b['mean'] / a['mean']),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('size', help="64x32 | 128x64 | 256x128, or 'sweep'")
    ap.add_argument('crops', help='crops per forward (sweep: the size)')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--shared', action='store_true', help='activation buffers overlaid by lifetime, as the pipeline builds its encoder')
    ap.add_argument('--jsonl', default=None)
    ap.add_argument('--tag', default='')
    ap.add_argument('--counts', default='8,16,32,64,128,256,512,1024')
    args = ap.parse_args()
    if args.size == 'sweep':
        args.size = args.crops
        sweep(args)
    else:
        args.crops = int(args.crops)
        measure(args)


if __name__ == '__main__':
    main()
