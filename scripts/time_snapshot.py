"""What a stream snapshot costs (MultiStreamPipeline.snapshot / restore): one worker group of bench.py's workload is stepped until its
galleries hold some rows, then, three repetitions each, in one process:

  * the two gallery kernels alone (dd_chunk_rows_gather / dd_chunk_rows_scatter: table upload + chunk_rows_gather_k / chunk_rows_scatter_k)
    on a layout with the group's row counts -- every track's chunks drawn at random from 64 MiB arenas -- between device events, beside a
    device-to-device copy of the same bytes, the floor of a pure copy;
  * snapshot() and restore() of the whole group on the host clock, without background, and of a small group of --bg-streams streams with subtraction on,
    with and without its background model (about 31 MB per 640 x 480 stream), with the blob sizes.

Nothing is asserted; the figures are the record.  Prints one JSON line per measurement and appends them to --out.

    python scripts/time_snapshot.py --out profiles/r24_snapshot.jsonl
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
    ap.add_argument('--steps', type=int, default=16, help='steps before the snapshot')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--period', type=int, default=8, help='distinct frames per stream resident in HBM')
    ap.add_argument('--bg-streams', type=int, default=32, help='streams snapshotted with their background model')
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
    from deepdish_amd.runtime import Context, default_context, ptr

    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    dev = torch.empty((args.period, S, H, W, 3), dtype=torch.uint8, device='cuda:0')
    dets = bench.make_inputs_rendered(pool, 0, S, args.period, W, H, [dev], [0, S], 'cuda:0')
    kw = dict(model=model, input_size=(W, H))
    src, dst = MultiStreamPipeline(S, context=Context(0), **kw), MultiStreamPipeline(S, context=Context(0), **kw)
    # the background model is timed on a small group of its own, with subtraction on (bench's workload runs with it off, as the reference's does)
    B = min(args.bg_streams, S)
    srcb, dstb = (MultiStreamPipeline(B, context=Context(0), background_subtraction_ratio=0.25, **kw) for _ in range(2))
    injb = [srcb.pack_injected([dets[s][f] for s in range(B)]) for f in range(args.period)]
    inj = [src.pack_injected([dets[s][f] for s in range(S)]) for f in range(args.period)]
    torch.cuda.synchronize()
    for f in range(args.steps):
        a, b = f % args.period, (f + 1) % args.period
        src.step(dev[a], inj[a], dev[b] if f + 1 < args.steps else None)
        srcb.step(dev[a][:B].contiguous(), injb[a])
    # ---- snapshot / restore on the host clock
    for what, one, two, background in (('group', src, dst, False), ('small_group_without_background', srcb, dstb, False),
                                       ('small_group_with_background', srcb, dstb, True)):
        t_snap, t_rest, size, info = [], [], 0, None
        for rep in range(args.reps):
            t0 = time.perf_counter()
            snap = one.snapshot(None, background=background)
            t1 = time.perf_counter()
            two.restore(snap)
            t2 = time.perf_counter()
            t_snap.append(1e3 * (t1 - t0)); t_rest.append(1e3 * (t2 - t1))
            size, info = sum(i['bytes'] for i in snap.info), snap.info
        emit(what='snapshot_restore_ms', case=what, streams=len(info), background=background, blob_bytes=size, tracks=sum(i['n_tracks'] for i in info),
             gallery_rows=sum(i['gallery_rows'] for i in info), snapshot_ms=[round(t, 3) for t in t_snap], restore_ms=[round(t, 3) for t in t_rest],
             snapshot_ms_median=round(statistics.median(t_snap), 3), restore_ms_median=round(statistics.median(t_rest), 3))
    # ---- the kernels alone, on a layout with the group's row counts: tracks of rows / tracks rows each, chunks drawn at random
    full = src.snapshot(None, background=False)
    n_tracks = max(1, sum(i['n_tracks'] for i in full.info))
    rows_total = max(n_tracks, sum(i['gallery_rows'] for i in full.info))
    per = [rows_total // n_tracks + (k < rows_total % n_tracks) for k in range(n_tracks)]
    ARENA_ROWS = 131072
    n_chunks = sum((r + 31) // 32 for r in per)
    n_arenas = max(2, -(-n_chunks * 32 // ARENA_ROWS) + 1)
    arenas = [torch.randn((ARENA_ROWS, 128), dtype=torch.float32, device='cuda:0') for _ in range(n_arenas)]
    rng = np.random.default_rng(1)
    chunks = np.ascontiguousarray(rng.permutation(n_arenas * (ARENA_ROWS // 32))[:n_chunks], dtype=np.int32)
    table, c0, r0 = np.zeros((n_tracks, 3), np.int64), 0, 0
    for k, r in enumerate(per):
        table[k] = (c0, r, r0)
        c0 += (r + 31) // 32
        r0 += r
    dense, other = torch.zeros((rows_total, 128), dtype=torch.float32, device='cuda:0'), torch.zeros((rows_total, 128), dtype=torch.float32, device='cuda:0')
    ptrs = (ctypes.c_void_p * n_arenas)(*[a.data_ptr() for a in arenas])
    ctx = default_context()
    side = torch.cuda.Stream()                               # the calls and the events that bracket them share this stream
    stream = ctypes.c_void_p(side.cuda_stream)
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            e0.record()
            fn()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def kernel(name):
        return lambda: check(getattr(lib(), name)(ctx.handle, ptrs, n_arenas, ARENA_ROWS, ptr(chunks), n_chunks, ptr(table), n_tracks, ptr(dense), rows_total,
                                                  stream), name)
    ms = {'gather': [], 'scatter': [], 'copy': []}
    for rep in range(args.reps + 1):                         # the first repetition warms up and is dropped
        for key, fn in (('gather', kernel('dd_chunk_rows_gather')), ('scatter', kernel('dd_chunk_rows_scatter')), ('copy', lambda: other.copy_(dense))):
            t = timed(fn)
            if rep:
                ms[key].append(t)
    nbytes = rows_total * 512
    emit(what='chunk_rows_ms', tracks=n_tracks, rows=rows_total, bytes=nbytes, arenas=n_arenas,
         **{k + '_ms': [round(t, 4) for t in v] for k, v in ms.items()}, **{k + '_ms_median': round(statistics.median(v), 4) for k, v in ms.items()},
         **{k + '_gb_s': round(2 * nbytes / (1e6 * statistics.median(v)), 1) for k, v in ms.items()})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for l in lines:
                f.write(json.dumps(l) + '\n')


if __name__ == '__main__':
    main()
