#!/usr/bin/env python3
"""time_ingest_raw8.py -- the ingest ring fed BGR, NV12, 8-bit Bayer and 8-bit monochrome frames from pinned host memory, in one process.

    python scripts/time_ingest_raw8.py [--streams 1536] [--steps 12] [--warmup 3] [--slots 3] [--reps 3] [--formats bgr,nv12,bayer_rggb,gray]
                                       [--out profiles/r26_ingest_raw8.jsonl]
    python scripts/time_ingest_raw8.py --kernels [--streams 1536] [--resize-streams 256]

Default mode: the loop of scripts/time_ingest_yuv.py (bench.py's --ingest-host loop on ONE worker group: uint8 SSD-MobileNet-v1 + MARS +
deep_sort on 640x480 frames with injected detections; the pinned slots of every ring filled before the timed region and reused
round-robin; the formats timed alternately, --reps times each).  Per run: frames/s and the host-to-device GB/s the slots' bytes amount
to.  One JSON line per run plus one summary line, appended to --out.  --formats names the rings and the order in which their pinned slots
are allocated and timed (where a slot lands in host memory shows in its upload rate): run it twice, the second time reversed.

--kernels: on frames already in HBM, at 640x480 (--streams frames) and 1280x720 (--resize-streams frames), device-event times over ten
calls of raw8_to_bgr per layout beside a device-to-device hipMemcpyAsync of the same output bytes; and the ring's transform to 640x480
(from 640x480 with a flip, from 1280x720 without) fused and as two launches (DD_INGEST_YUV_FUSED=0): host times of upload + transform,
2 x --reps of them.  The ring's launches run on its private copy stream: run this mode under `rocprofv3 --kernel-trace --stats` for the
per-kernel device times of the fused launch and of the two it replaces.

The mosaics sample the rendered BGR scenes (deepdish_amd.synth.to_bayer / to_gray on the device): synthetic input, it pins nothing.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import bench  # noqa: E402
from time_ingest_yuv import to_yuv420_dev  # noqa: E402

FORMATS = ('bgr', 'nv12', 'bayer_rggb', 'gray')
BAYER = ('bayer_rggb', 'bayer_grbg', 'bayer_gbrg', 'bayer_bggr')


def to_bayer_dev(bgr, pattern):
    """u8 [N, H, W, 3] BGR device tensor -> u8 [N, H, W] (synth.to_bayer on the device)."""
    import torch
    out = torch.empty(bgr.shape[:3], dtype=torch.uint8, device=bgr.device)
    for k, colour in enumerate(pattern[6:]):
        y, x = k >> 1, k & 1
        out[:, y::2, x::2] = bgr[:, y::2, x::2, 'bgr'.index(colour)]
    return out


def to_gray_dev(bgr):
    """u8 [N, H, W, 3] BGR device tensor -> u8 [N, H, W] (synth.to_gray on the device)."""
    import torch
    f = bgr.to(torch.int32)
    return ((1868 * f[..., 0] + 9617 * f[..., 1] + 4899 * f[..., 2] + 8192) >> 14).to(torch.uint8)


def to_slot_dev(bgr, fmt):
    return bgr if fmt == 'bgr' else to_yuv420_dev(bgr, fmt) if fmt == 'nv12' else to_gray_dev(bgr) if fmt == 'gray' else to_bayer_dev(bgr, fmt)


def ring_mode(args):
    cfg = bench.CONFIGS[2]
    W, H, model = cfg['W'], cfg['H'], cfg['model'] + '-uint8'
    S, K = args.streams, args.slots
    formats = tuple(args.formats.split(','))
    assert 'bgr' in formats and set(formats) <= set(('bgr', 'nv12', 'gray') + BAYER), formats
    pool = bench.start_gen_pool(1, S)                         # before anything touches the GPU
    os.environ.setdefault('DD_HOST_THREADS', str(bench.host_threads(1, 1)))
    import torch
    from deepdish_amd.ingest import FrameIngest
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.runtime import Context
    torch.cuda.set_device(0)
    dev = torch.empty((K, S, H, W, 3), dtype=torch.uint8, device='cuda:0')
    dets = bench.make_inputs_rendered(pool, 0, S, K, W, H, [dev], [0, S], 'cuda:0')
    ctx = Context(0)
    pipe = MultiStreamPipeline(S, model=model, input_size=(W, H), context=ctx)
    injected = [pipe.pack_injected([dets[s][f] for s in range(S)]) for f in range(K)]
    rings = {}
    for fmt in formats:
        ring = FrameIngest(S, (W, H), slots=K, context=ctx, pixel_format=fmt)
        for f in range(K):
            torch.from_numpy(ring.host(f)).copy_(to_slot_dev(dev[f], fmt))
        rings[fmt] = ring
    del dev
    torch.cuda.synchronize()
    det_stream = pipe.detector_stream()

    def run(ring, f0, f1):                                    # bench.py's --ingest-host loop, slots reused round-robin
        ring.submit(f0 % K)
        for f in range(f0, f1):
            if f + 1 < f1:
                ring.submit((f + 1) % K)                      # the next step's upload runs under this step's kernels
            nxt = ring.frames((f + 1) % K, stream=det_stream) if f + 1 < f1 else None
            pipe.step(ring.frames(f % K), injected[f % K], nxt)
            ring.release(f % K)
        torch.cuda.synchronize()

    rows = []
    for fmt in formats:
        run(rings[fmt], 0, args.warmup)
    for rep in range(args.reps):
        for fmt in formats:                                   # alternating: a drift of the box hits all of them alike
            t0 = time.perf_counter()
            run(rings[fmt], 0, args.steps)
            dt = time.perf_counter() - t0
            nbytes = rings[fmt].host(0).nbytes
            rows.append({'what': 'ring', 'pixel_format': fmt, 'rep': rep, 'frames_per_s': round(args.steps * S / dt, 1),
                         'h2d_GB_per_s': round(args.steps * nbytes / dt / 1e9, 2), 'ms_per_step': round(1e3 * dt / args.steps, 3),
                         'slot_bytes': nbytes, 'streams': S, 'steps': args.steps, 'slots': K, 'model': model})
            print(json.dumps(rows[-1]), flush=True)
    summary = {'what': 'ring_summary', 'streams': S, 'steps': args.steps, 'formats': list(formats)}
    for fmt in formats:
        v = [r['frames_per_s'] for r in rows if r['pixel_format'] == fmt]
        summary[fmt] = {'frames_per_s_min': min(v), 'frames_per_s_max': max(v), 'frames_per_s_median': float(np.median(v))}
    # faster only when the gap exceeds the spread of the repetitions of each
    for fmt in formats:
        if fmt != 'bgr':
            summary[fmt + '_faster_than_bgr'] = summary[fmt]['frames_per_s_min'] > summary['bgr']['frames_per_s_max']
    rows.append(summary)
    print(json.dumps(summary), flush=True)
    return rows


def kernel_mode(args):
    import ctypes
    import torch
    from deepdish_amd.ingest import FrameIngest, raw8_to_bgr
    from deepdish_amd.runtime import Context
    torch.cuda.set_device(0)
    ctx = Context(0)
    hip = ctypes.CDLL('libamdhip64.so')
    n = 10
    rows = []
    layouts = ('bayer_rggb', 'bayer_grbg', 'gray')            # a red-first and a green-first mosaic: the other two swap R and B

    def timed(fn):
        with torch.cuda.stream(ctx.torch_stream):
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
        ctx.sync()
        return e0.elapsed_time(e1) / n                        # ms per call

    # (source size, frames, the ring's flip): 640x480 -> 640x480 needs the flip to have a transform at all
    for (W, H), N, flip in (((640, 480), args.streams, True), ((1280, 720), args.resize_streams, False)):
        out = torch.empty((N, H, W, 3), dtype=torch.uint8, device='cuda:0')
        twin = torch.empty_like(out)
        torch.cuda.synchronize()

        def d2d():
            rc = hip.hipMemcpyAsync(ctypes.c_void_p(twin.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_size_t(out.numel()), 3,
                                    ctypes.c_void_p(ctx.stream_ptr))
            assert rc == 0
        for rep in range(args.reps):
            ms_copy = timed(d2d)                              # the floor: the converter's output bytes read once and written once
            rows.append({'what': 'd2d_memcpy_of_output', 'src': [W, H], 'frames': N, 'rep': rep, 'bytes': out.numel(), 'ms': round(ms_copy, 4),
                         'TB_per_s_read_plus_written': round(2 * out.numel() / ms_copy / 1e9, 3)})
            for layout in layouts:
                src = torch.randint(0, 256, (N * H * W,), dtype=torch.uint8, device='cuda:0')
                torch.cuda.synchronize()
                ms = timed(lambda: raw8_to_bgr(src, H, W, layout, out=out, context=ctx))
                moved = src.numel() + out.numel()
                rows.append({'what': 'to_bgr', 'layout': layout, 'src': [W, H], 'frames': N, 'rep': rep, 'bytes_read_plus_written': moved,
                             'ms': round(ms, 4), 'TB_per_s': round(moved / ms / 1e9, 3), 'times_d2d_memcpy_of_output': round(ms / ms_copy, 3)})
                del src
        del out, twin
        R = args.resize_streams
        for layout in layouts:
            for fused in (True, False):
                os.environ['DD_INGEST_YUV_FUSED'] = '1' if fused else '0'         # read when the ring is created
                ring = FrameIngest(R, (W, H), (640, 480), slots=1, flip=flip, context=ctx, pixel_format=layout)
                ring.host(0)[...] = np.random.default_rng(1).integers(0, 256, ring.host(0).shape, dtype=np.uint8)
                # submit = upload + transform on the ring's copy stream; both forms upload the same bytes
                ring.submit(0)
                ring.acquire(0)
                ctx.sync()
                t = []
                for _ in range(2 * args.reps):
                    t0 = time.perf_counter()
                    ring.submit(0)
                    ring.acquire(0)
                    ctx.sync()
                    t.append(round(1e3 * (time.perf_counter() - t0), 3))
                rows.append({'what': 'ring_submit', 'layout': layout, 'src': [W, H], 'dst': [640, 480], 'flip': flip, 'fused': fused, 'frames': R,
                             'host_ms_upload_plus_transform': t, 'host_ms_min': min(t)})
                del ring
        del os.environ['DD_INGEST_YUV_FUSED']
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=1536)
    ap.add_argument('--steps', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--slots', type=int, default=3, help='pinned slots per ring (>= 2), reused round-robin')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--formats', default=','.join(FORMATS), help='the rings of the default mode, in allocation and timing order')
    ap.add_argument('--kernels', action='store_true', help='time the conversion kernels alone (see the module docstring)')
    ap.add_argument('--resize-streams', type=int, default=256)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r26_ingest_raw8.jsonl'))
    args = ap.parse_args()
    assert args.slots >= 2
    rows = kernel_mode(args) if args.kernels else ring_mode(args)
    with open(args.out, 'a') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
