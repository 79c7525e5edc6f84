#!/usr/bin/env python3
"""time_regular_nms.py -- the post-process op's two NMS modes side by side: the fast class-agnostic path (ssd_decode_k +
nms_greedy_f32_k + ssd_gather_k) and the per-class path a model file with use_regular_nms = true selects (ssd_regular_nms_k,
csrc/post_regular.hip), on the same inputs in the same process.

    python scripts/time_regular_nms.py [--out profiles/r09_regular_nms.jsonl] [--frames 768,1536] [--reps 12] [--streams 1536]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/time_regular_nms.py --reps 3 --steps 6

1. The stage alone, device events around each call, the two modes alternating: seeded synthetic head tensors of the detector's shape
   (1 917 anchors, 91 columns, max_detections 10, detections_per_class 100, nms_score_threshold 1e-8).  f32 head matrix: dd_ssd_decode +
   dd_ssd_postprocess_decoded against dd_ssd_postprocess_regular.  uint8 head tensors: dd_ssd_postprocess_regular_u8; the fast path's
   uint8 first stage (q_ssd_decode_k) is an op of the engine and has no entry of its own -- its time is in the kernel trace of part 2,
   the second stage (nms_greedy_f32_k + ssd_gather_k on decoded arrays) is timed here.
2. One worker group of bench.py's headline (uint8 SSD-MobileNet-v1 + MARS + deep_sort, injected detections, look-ahead on) stepped
   with a fast-NMS and a regular-NMS copy of the same synthetic model file, alternating.
3. The f32 engine: the same with the float model at --f32-streams streams, and the fast mode once more with the head layers' decode
   epilogue off (DD_SSD_DEC=0: the head matrix is written, ssd_decode_k reads it) -- what switching the epilogue off costs by itself.
One JSON line per measurement, on stdout and appended to --out.
"""
import argparse
import gc
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402

A, NC, MAX_DET, PER_CLASS, THR, IOU = 1917, 91, 10, 100, 1e-8, 0.6


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, 'a') as f:
            f.write(line + '\n')


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def time_stage(args, out):
    import numpy as np
    import torch
    from deepdish_amd import nets, quantize
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import Context, ptr
    ctx = Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    anchors = torch.from_numpy(np.ascontiguousarray(nets.ssd_anchors(300)[0], dtype=np.float32)).cuda()
    qm = quantize.synthetic_ssd_quant_model(1234)
    Lb, Lc, Lo = qm['layers']['box0'], qm['layers']['cls0'], qm['logistic']
    lut = torch.from_numpy(quantize.logistic_table(Lc['out_scale'], Lc['out_zp'], Lo['out_scale'], Lo['out_zp'])).cuda()
    quant = np.array([Lb['out_scale'], Lb['out_zp'], Lo['out_scale'], Lo['out_zp']], np.float32)

    def timed(fn, reps, warmup=3):
        for _ in range(warmup):
            fn()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    for n in [int(v) for v in args.frames.split(',')]:
        g = torch.Generator(device='cuda').manual_seed(9)
        raw = torch.empty((n, A, 4 + NC), dtype=torch.float32, device='cuda')
        raw[..., :4] = torch.randn((n, A, 4), generator=g, device='cuda') * 0.5
        raw[..., 4:] = torch.randn((n, A, NC), generator=g, device='cuda') * 2.0 - 4.0        # mostly small scores, a few large: a detector's head
        box_q = torch.randint(int(Lb['out_zp']) - 30, int(Lb['out_zp']) + 31, (n, A, 4), generator=g, device='cuda').clamp(0, 255).to(torch.uint8)
        cls_q = torch.randint(0, 256, (n, A, 96), generator=g, device='cuda').to(torch.uint8)
        db, dsc, dk = (torch.empty((n, A, 4), dtype=torch.float32, device='cuda'), torch.empty((n, A), dtype=torch.float32, device='cuda'),
                       torch.empty((n, A), dtype=torch.float32, device='cuda'))
        dcl = torch.empty((n, A), dtype=torch.int32, device='cuda')
        outs = (torch.empty((n, MAX_DET, 4), dtype=torch.float32, device='cuda'), torch.empty((n, MAX_DET), dtype=torch.float32, device='cuda'),
                torch.empty((n, MAX_DET), dtype=torch.float32, device='cuda'), torch.empty((n,), dtype=torch.int32, device='cuda'))
        po = [ptr(o) for o in outs]

        def fast_f32():
            check(lib().dd_ssd_decode(ctx.handle, ptr(raw), ptr(anchors), A, NC, THR, ptr(db), ptr(dsc), ptr(dcl), ptr(dk), n, stream), 'dd_ssd_decode')
            check(lib().dd_ssd_postprocess_decoded(ctx.handle, ptr(db), ptr(dsc), ptr(dcl), ptr(dk), A, MAX_DET, THR, IOU, *po, n, stream),
                  'dd_ssd_postprocess_decoded')

        def fast_second_stage():
            check(lib().dd_ssd_postprocess_decoded(ctx.handle, ptr(db), ptr(dsc), ptr(dcl), ptr(dk), A, MAX_DET, THR, IOU, *po, n, stream),
                  'dd_ssd_postprocess_decoded')

        def regular_f32():
            check(lib().dd_ssd_postprocess_regular(ctx.handle, ptr(raw), ptr(anchors), A, NC, MAX_DET, PER_CLASS, THR, IOU, *po, n, stream),
                  'dd_ssd_postprocess_regular')

        def regular_u8():
            check(lib().dd_ssd_postprocess_regular_u8(ctx.handle, ptr(box_q), ptr(cls_q), 96, ptr(lut), ptr(quant), ptr(anchors), A, NC, MAX_DET,
                                                      PER_CLASS, THR, IOU, *po, n, stream), 'dd_ssd_postprocess_regular_u8')

        res = {k: [] for k in ('fast_f32', 'regular_f32', 'fast_second_stage', 'regular_u8')}
        for _ in range(args.rounds):                                  # the modes alternate: drift shows up in both
            for name, fn in (('fast_f32', fast_f32), ('regular_f32', regular_f32), ('fast_second_stage', fast_second_stage), ('regular_u8', regular_u8)):
                res[name] += timed(fn, args.reps)
        rows = int(outs[3].sum().item())
        for name, ms in res.items():
            emit(out, dict(part='stage', what=name, frames=n, anchors=A, columns=NC, max_detections=MAX_DET, detections_per_class=PER_CLASS,
                           nms_score_threshold=THR, us_per_frame=round(1e3 * statistics.median(ms) / n, 4), **spread(ms)))
        emit(out, dict(part='stage', what='rows_of_last_call', frames=n, rows=rows))
        del raw, box_q, cls_q, db, dsc, dk, dcl, outs
        gc.collect()
        torch.cuda.empty_cache()
    return ctx


def make_frames(args, pool):
    """The frames and injected detections of one worker group, resident in HBM (bench.py's own generator)."""
    import torch
    cfg = bench.CONFIGS[2]
    W, H = cfg['W'], cfg['H']
    period = min(args.warmup + args.steps, bench.FRAME_PERIOD)
    dev_frames = [torch.empty((period, args.streams, H, W, 3), dtype=torch.uint8, device='cuda:0')]
    dets = bench.make_inputs_rendered(pool, 0, args.streams, period, W, H, dev_frames, [0, args.streams], 'cuda:0')
    return dev_frames[0], dets, period, (W, H)


def step_group(args, out, ctx, inputs, tag, models, streams):
    """models: [(name, path, environment)]: one MultiStreamPipeline each over the first `streams` streams of the same frames and injected
    detections, timed as bench.py times its steps; args.rounds times over, alternating."""
    import torch
    from deepdish_amd.multipipe import MultiStreamPipeline
    frames, dets, period, size = inputs
    n_frames = args.warmup + args.steps
    for rnd in range(args.rounds):
        for name, path, env in models:
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            p = MultiStreamPipeline(streams, model=path, input_size=size, context=ctx)
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
            injected = [p.pack_injected([dets[s][f] for s in range(streams)]) for f in range(period)]

            def run(f0, f1):
                for f in range(f0, f1):
                    p.step(frames[f % period][:streams], injected[f % period], frames[(f + 1) % period][:streams] if f + 1 < f1 else None)
                torch.cuda.synchronize()

            run(0, args.warmup)
            t0 = time.perf_counter()
            run(args.warmup, n_frames)
            dt = time.perf_counter() - t0
            sm = p.stage_ms()
            emit(out, dict(part=tag, what=name, round=rnd, streams=streams, steps=args.steps, warmup=args.warmup, detector=p.det_dtype,
                           frames_per_s=round(args.steps * streams / dt, 1), ms_per_step=round(1e3 * dt / args.steps, 3),
                           stage_ms_per_step={k: round(float(sm[k]), 4) for k in ('objd', 'nms', 'feat', 'trak', 'host', 'wall')}))
            del p, injected
            gc.collect()
            torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--frames', default='768,1536')
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--steps', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--streams', type=int, default=1536)
    ap.add_argument('--f32-streams', type=int, default=384)
    ap.add_argument('--parts', default='stage,pipeline,f32')
    args = ap.parse_args()
    parts = args.parts.split(',')
    pool = bench.start_gen_pool(1, args.streams) if ('pipeline' in parts or 'f32' in parts) else None      # before anything touches the GPU
    os.environ.setdefault('DD_HOST_THREADS', str(bench.host_threads(1, 1)))
    import torch
    from deepdish_amd import nets, quantize
    from deepdish_amd.runtime import Context
    from deepdish_amd.tools import tflite_writer
    torch.cuda.set_device(0)
    ctx = time_stage(args, args.out) if 'stage' in parts else Context(0)
    regular = dict(use_regular_nms=True, detections_per_class=PER_CLASS)
    inputs = make_frames(args, pool) if 'pipeline' in parts or 'f32' in parts else None
    with tempfile.TemporaryDirectory() as tmp:
        if 'pipeline' in parts:
            qm = quantize.synthetic_ssd_quant_model(1234)
            fast, reg = os.path.join(tmp, 'ssd_mobilenet_v1_uint8_fast.tflite'), os.path.join(tmp, 'ssd_mobilenet_v1_uint8_regular.tflite')
            tflite_writer.write_ssd_mobilenet(qm, fast)
            tflite_writer.write_ssd_mobilenet(qm, reg, post=regular)
            step_group(args, args.out, ctx, inputs, 'pipeline_uint8', [('fast', fast, {}), ('regular', reg, {})], args.streams)
        if 'f32' in parts:
            folded = {}
            for name, kind, w, b, stride, act in quantize.folded_ssd_layers(nets.synthetic_ssd_weights(1234)):
                folded[name + '/weights'] = w if kind == 'conv' else w[:, :, :, None]
                folded[name + '/biases'] = b
            fast, reg = os.path.join(tmp, 'ssd_mobilenet_v1_f32_fast.tflite'), os.path.join(tmp, 'ssd_mobilenet_v1_f32_regular.tflite')
            tflite_writer.write_ssd_mobilenet(folded, fast)
            tflite_writer.write_ssd_mobilenet(folded, reg, post=regular)
            step_group(args, args.out, ctx, inputs, 'pipeline_f32', [('fast', fast, {}), ('fast_epilogue_decode_off', fast, {'DD_SSD_DEC': '0'}), ('regular', reg, {})],
                       min(args.f32_streams, args.streams))


if __name__ == '__main__':
    main()
