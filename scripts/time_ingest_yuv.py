#!/usr/bin/env python3
"""time_ingest_yuv.py -- the ingest ring fed BGR, NV12, I420, YUY2 and UYVY frames from pinned host memory, in one process.

    python scripts/time_ingest_yuv.py [--streams 1536] [--steps 12] [--warmup 3] [--slots 3] [--reps 3] [--formats bgr,nv12,i420,yuy2,uyvy]
                                      [--out profiles/r16_ingest_yuv.jsonl]
    python scripts/time_ingest_yuv.py --kernels [--streams 1536] [--resize-streams 256]

Default mode: the --ingest-host loop of bench.py (look-ahead upload, the next frames acquired for the detector stream) on ONE worker
group: uint8 SSD-MobileNet-v1 + MARS + deep_sort on 640x480 frames with injected detections.  The pinned slots of all five rings
are filled before the timed region (a decoder would write there directly) and reused round-robin, so the same pipeline steps over
the same pictures whatever the slot format; the formats are timed alternately, --reps times each.  Per run: frames/s and the
host-to-device GB/s the slots' bytes amount to.  One JSON line per run plus one summary line, appended to --out.  --formats names the
rings and the order in which their pinned slots are allocated and timed (where a slot lands in host memory shows in its upload rate).

--kernels: the conversion alone on frames already in HBM, at 640x480 (--streams frames) and 1280x720 (--resize-streams frames) --
device-event times of yuv420_to_bgr / yuv422_to_bgr per layout beside a device-to-device hipMemcpyAsync of the same output bytes --
and the ring's transform to 640x480 (from 640x480 with a flip, from 1280x720 without) fused and as two launches
(DD_INGEST_YUV_FUSED=0): host times of upload + transform, --reps of them.  Run it under `rocprofv3 --kernel-trace --stats` for the
per-kernel figures of the ring's launches; the event times printed here include the launch gaps.

The YUV frames are a float BT.601 forward transform of the rendered BGR scenes done on the device (the arithmetic of
deepdish_amd.synth.to_yuv420 / to_yuv422 in float32): synthetic input, it pins nothing.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402

FORMATS = ('bgr', 'nv12', 'i420', 'yuy2', 'uyvy')
PLANAR, PACKED = ('nv12', 'i420'), ('yuy2', 'uyvy')


def to_yuv420_dev(bgr, layout):
    """u8 [N, H, W, 3] BGR device tensor -> u8 [N, H * 3 // 2, W] (synth.to_yuv420 on the device, float32)."""
    import torch
    N, H, W, _ = bgr.shape
    f = bgr.float()
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    y = 16.0 + (65.481 * r + 128.553 * g + 24.966 * b) / 255.0
    u = 128.0 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255.0
    v = 128.0 + (112.0 * r - 93.786 * g - 18.214 * b) / 255.0
    sub = lambda p: p.reshape(N, H // 2, 2, W // 2, 2).mean(dim=(2, 4))         # noqa: E731
    q = lambda p: p.round().clamp(0, 255).to(torch.uint8)                        # noqa: E731
    out = torch.empty((N, H * 3 // 2, W), dtype=torch.uint8, device=bgr.device)
    out[:, :H] = q(y)
    cu, cv = q(sub(u)), q(sub(v))
    if layout == 'nv12':
        out[:, H:] = torch.stack([cu, cv], dim=-1).reshape(N, H // 2, W)
    else:
        out[:, H:] = torch.cat([cu.reshape(N, H // 4, W), cv.reshape(N, H // 4, W)], dim=1)
    return out


def to_yuv422_dev(bgr, order):
    """u8 [N, H, W, 3] BGR device tensor -> u8 [N, H, W, 2] (synth.to_yuv422 on the device, float32)."""
    import torch
    N, H, W, _ = bgr.shape
    f = bgr.float()
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    y = 16.0 + (65.481 * r + 128.553 * g + 24.966 * b) / 255.0
    u = 128.0 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255.0
    v = 128.0 + (112.0 * r - 93.786 * g - 18.214 * b) / 255.0
    sub = lambda p: p.reshape(N, H, W // 2, 2).mean(dim=3)                      # noqa: E731
    q = lambda p: p.round().clamp(0, 255).to(torch.uint8)                        # noqa: E731
    out = torch.empty((N, H, W, 2), dtype=torch.uint8, device=bgr.device)
    luma, chroma = (0, 1) if order == 'yuy2' else (1, 0)
    out[..., luma] = q(y)
    out[:, :, 0::2, chroma], out[:, :, 1::2, chroma] = q(sub(u)), q(sub(v))
    return out


def to_slot_dev(bgr, fmt):
    return bgr if fmt == 'bgr' else to_yuv420_dev(bgr, fmt) if fmt in PLANAR else to_yuv422_dev(bgr, fmt)


def ring_mode(args):
    cfg = bench.CONFIGS[2]
    W, H, model = cfg['W'], cfg['H'], cfg['model'] + '-uint8'
    S, K = args.streams, args.slots
    formats = tuple(args.formats.split(','))
    assert formats[0] == 'bgr' and set(formats) <= set(FORMATS), formats
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
    for fmt in formats[1:]:
        summary[fmt + '_faster_than_bgr'] = summary[fmt]['frames_per_s_min'] > summary['bgr']['frames_per_s_max']
    rows.append(summary)
    print(json.dumps(summary), flush=True)
    return rows


def kernel_mode(args):
    import ctypes
    import torch
    from deepdish_amd.ingest import FrameIngest, yuv420_to_bgr, yuv422_to_bgr
    from deepdish_amd.runtime import Context
    torch.cuda.set_device(0)
    ctx = Context(0)
    hip = ctypes.CDLL('libamdhip64.so')
    n = 10
    rows = []

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
            for layout in PLANAR + PACKED:
                bpp = 1.5 if layout in PLANAR else 2.0
                src = torch.randint(0, 256, (int(N * H * W * bpp),), dtype=torch.uint8, device='cuda:0')
                torch.cuda.synchronize()
                conv = yuv420_to_bgr if layout in PLANAR else yuv422_to_bgr
                ms = timed(lambda: conv(src, H, W, layout, out=out, context=ctx))
                moved = src.numel() + out.numel()
                rows.append({'what': 'to_bgr', 'layout': layout, 'src': [W, H], 'frames': N, 'rep': rep, 'bytes_read_plus_written': moved,
                             'ms': round(ms, 4), 'TB_per_s': round(moved / ms / 1e9, 3), 'times_d2d_memcpy_of_output': round(ms / ms_copy, 3)})
                del src
        del out, twin
        R = args.resize_streams
        for layout in PLANAR + PACKED:
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
    ap.add_argument('--formats', default=','.join(FORMATS), help="the rings of the default mode, in allocation and timing order; 'bgr' first")
    ap.add_argument('--kernels', action='store_true', help='time the conversion kernels alone (see the module docstring)')
    ap.add_argument('--resize-streams', type=int, default=256)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r16_ingest_yuv.jsonl'))
    args = ap.parse_args()
    assert args.slots >= 2
    rows = kernel_mode(args) if args.kernels else ring_mode(args)
    with open(args.out, 'a') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
