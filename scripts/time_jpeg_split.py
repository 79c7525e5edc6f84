#!/usr/bin/env python3
"""time_jpeg_split.py -- the split entropy stage (JpegDecoder(..., split=True), jpeg_split_entropy_k) against the default decoder, timed.

    python scripts/time_jpeg_split.py [--frames 256,1536] [--reps 3] [--out profiles/r22_jpeg_split.jsonl]
    python scripts/time_jpeg_split.py --ring [--streams 1536] [--steps 12] [--warmup 3] [--slots 3] [--reps 3]

Default mode: one process, device events through profile().  The rendered-looking 640 x 480 scenes of scripts/time_ingest_jpeg.py (4:2:0,
64 distinct pictures, repeated) at quality 75 and 95, 256 and 1536 files, without restart markers ('none') and with one interval per MCU
row ('row1'), on a default decoder, on a split decoder as it comes ('split': 64 bytes, doubled per file until a lane has one subsequence)
and on split decoders whose subsequences are fixed at 64, 128, 256 and 512 bytes (DD_JPEGDEC_SPLIT_BYTES is read when a decoder is made).
Three repetitions; within a repetition the variants follow each other on the same files, so a drift of the machine hits all alike.  Per row: jpeg_markers_k, clearing + entropy, pixels in ms, the frames/s of those kernels, and split_stats().  The
summary says whether the split decoder's clear + entropy range at 1536 marker-less files lies wholly below the default decoder's (the
ranges over the repetitions do not overlap).  Every split decode's frames are compared with the default decoder's once, in the warm-up.

--ring: the --ingest-host loop of scripts/time_ingest_jpeg.py on one worker group, JPEG slots holding this build's own encoder's files at
quality 95 with one interval per file, with and without jpeg_split, alternating.

One JSON line per run, appended to --out.  No figure here is asserted anywhere."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'scripts')):
    if p not in sys.path:
        sys.path.insert(0, p)

from time_ingest_jpeg import H, THREADS, W, scene_files  # noqa: E402

SIZES = (64, 128, 256, 512)


def _split_decoder(B, **kw):
    from deepdish_amd.jpeg import JpegDecoder
    keep = os.environ.pop('DD_JPEGDEC_SPLIT_BYTES', None)
    os.environ['DD_JPEGDEC_SPLIT_BYTES'] = str(B)
    try:
        return JpegDecoder(H, W, split=True, **kw)
    finally:
        del os.environ['DD_JPEGDEC_SPLIT_BYTES']
        if keep is not None:
            os.environ['DD_JPEGDEC_SPLIT_BYTES'] = keep


def kernel_mode(args):
    import torch
    from deepdish_amd.jpeg import JpegDecoder
    from deepdish_amd.runtime import Context
    torch.cuda.set_device(0)
    ctx = Context(0)
    counts = [int(v) for v in args.frames.split(',')]
    kw = dict(max_frames=max(counts), max_bytes=max(counts) * 131072, context=ctx)
    variants = [('default', JpegDecoder(H, W, **kw)), ('split', JpegDecoder(H, W, split=True, **kw))] + [('split%d' % B, _split_decoder(B, **kw)) for B in SIZES]
    for _, dec in variants:
        dec.profile(True)
    out = torch.empty((max(counts), H, W, 3), dtype=torch.uint8, device='cuda:0')
    want = torch.empty_like(out)
    status = torch.empty(max(counts), dtype=torch.int32, device='cuda:0')
    torch.cuda.synchronize()
    rows = []
    for quality in (75, 95):
        for restart in ('none', 'row1'):
            base = scene_files(quality, restart)
            for n in counts:
                files = [base[i % len(base)] for i in range(n)]
                nbytes = sum(len(f) for f in files)
                for rep in range(-1, args.reps):              # rep -1 warms up and compares the frames
                    for name, dec in variants:
                        dst = want if (rep < 0 and name == 'default') else out
                        dec.decode(files, out=dst[:n], status=status[:n])
                        ms = dec.kernel_ms()
                        ctx.sync()
                        if rep < 0:
                            assert int(status[:n].abs().sum().item()) == 0
                            if name != 'default':
                                assert torch.equal(out[:n], want[:n]), '%s differs from the default decoder' % name
                            continue
                        dev_ms = ms['markers'] + ms['entropy'] + ms['pixels']
                        rows.append({'what': 'decode', 'variant': name, 'quality': quality, 'restart': restart, 'frames': n, 'rep': rep, 'file_bytes_mean': nbytes // n,
                                     'ms_markers': round(ms['markers'], 3), 'ms_entropy': round(ms['entropy'], 3), 'ms_pixels': round(ms['pixels'], 3),
                                     'kernels_frames_per_s': round(1e3 * n / dev_ms, 1), 'split_stats': dec.split_stats()})
                        print(json.dumps(rows[-1]), flush=True)
    summary = {'what': 'summary', 'frames': max(counts)}
    for quality in (75, 95):
        def span(name, restart='none'):
            v = [r['ms_entropy'] for r in rows if r['variant'] == name and r['quality'] == quality and r['restart'] == restart and r['frames'] == max(counts)]
            return [min(v), max(v)]
        d = span('default')
        summary['q%d' % quality] = {'default_ms_entropy': d, 'default_row1_ms_entropy': span('default', 'row1')}
        for name in ['split'] + ['split%d' % B for B in SIZES]:
            s = span(name)
            summary['q%d' % quality][name] = {'ms_entropy': s, 'wholly_below_default': s[1] < d[0], 'row1_ms_entropy': span(name, 'row1')}
    rows.append(summary)
    print(json.dumps(summary), flush=True)
    return rows


def ring_mode(args):
    import bench
    cfg = bench.CONFIGS[2]
    assert (cfg['W'], cfg['H']) == (W, H)
    model = cfg['model'] + '-uint8'
    S, K = args.streams, args.slots
    pool = bench.start_gen_pool(1, S)                         # before anything touches the GPU
    os.environ.setdefault('DD_HOST_THREADS', str(bench.host_threads(1, 1)))
    import torch
    from deepdish_amd.ingest import FrameIngest
    from deepdish_amd.jpeg import JpegEncoder
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import Context
    torch.cuda.set_device(0)
    dev = torch.empty((K, S, H, W, 3), dtype=torch.uint8, device='cuda:0')
    dets = bench.make_inputs_rendered(pool, 0, S, K, W, H, [dev], [0, S], 'cuda:0')
    ctx = Context(0)
    pipe = MultiStreamPipeline(S, model=model, input_size=(W, H), context=ctx)
    injected = [pipe.pack_injected([dets[s][f] for s in range(S)]) for f in range(K)]
    enc = JpegEncoder(H, W, quality=95, restart_rows=(H + 15) // 16, context=ctx)          # one interval per file
    files = [[] for _ in range(K)]
    for f in range(K):
        for z0 in range(0, S, 64):
            files[f] += enc.encode_to_host(dev[f, z0:z0 + 64])
    largest = max(sum((len(d) + 63) & ~63 for d in files[f]) for f in range(K))
    formats = ('jpeg1', 'jpeg1_split')
    rings = {fmt: FrameIngest(S, (W, H), slots=K, context=ctx, pixel_format='jpeg', jpeg_slot_bytes=largest + 64, jpeg_split=fmt.endswith('split')) for fmt in formats}
    del dev
    torch.cuda.synchronize()
    det_stream = pipe.detector_stream()
    threads = ThreadPoolExecutor(THREADS)

    def fill(fmt, slot):
        ring, data = rings[fmt], files[slot]
        chunk = (S + THREADS - 1) // THREADS

        def work(t):
            for z in range(t * chunk, min(S, (t + 1) * chunk)):
                ring.put(slot, z, data[z])
        list(threads.map(work, range(THREADS)))

    def run(fmt, f0, f1):                                     # bench.py's --ingest-host loop, slots reused round-robin
        ring = rings[fmt]
        fill(fmt, f0 % K)
        ring.submit(f0 % K)
        for f in range(f0, f1):
            if f + 1 < f1:
                fill(fmt, (f + 1) % K)
                ring.submit((f + 1) % K)                      # the next step's upload and decode run under this step's kernels
            nxt = ring.frames((f + 1) % K, stream=det_stream) if f + 1 < f1 else None
            pipe.step(ring.frames(f % K), injected[f % K], nxt)
            ring.release(f % K)
        torch.cuda.synchronize()

    rows = []
    for fmt in formats:
        run(fmt, 0, args.warmup)
        assert int(np.abs(rings[fmt].status((args.warmup - 1) % K)).sum()) == 0
    for rep in range(args.reps):
        for fmt in formats:                                   # alternating: a drift of the machine hits all alike
            t0 = time.perf_counter()
            run(fmt, 0, args.steps)
            dt = time.perf_counter() - t0
            rows.append({'what': 'ring', 'pixel_format': fmt, 'rep': rep, 'frames_per_s': round(args.steps * S / dt, 1), 'ms_per_step': round(1e3 * dt / args.steps, 3),
                         'slot_bytes': sum(len(d) for d in files[0]), 'streams': S, 'steps': args.steps, 'slots': K, 'model': model})
            print(json.dumps(rows[-1]), flush=True)
    summary = {'what': 'ring_summary', 'streams': S, 'steps': args.steps}
    for fmt in formats:
        v = [r['frames_per_s'] for r in rows if r['pixel_format'] == fmt]
        summary[fmt] = {'frames_per_s_min': min(v), 'frames_per_s_max': max(v), 'frames_per_s_median': float(np.median(v))}
    summary['split_faster'] = summary['jpeg1_split']['frames_per_s_min'] > summary['jpeg1']['frames_per_s_max']
    rows.append(summary)
    print(json.dumps(summary), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ring', action='store_true', help='time the ingest ring with and without jpeg_split (see the module docstring)')
    ap.add_argument('--streams', type=int, default=1536)
    ap.add_argument('--steps', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--slots', type=int, default=3, help='slots per ring (>= 2), reused round-robin')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--frames', default='256,1536')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r22_jpeg_split.jsonl'))
    args = ap.parse_args()
    assert args.slots >= 2
    rows = ring_mode(args) if args.ring else kernel_mode(args)
    with open(args.out, 'a') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
