"""The cases of the launch-plan fixture (tests/golden/launch_plan.json) and the one routine that runs them: shared by the recorder
(scripts/record_launch_plan.py) and the test that holds the executor to the record (tests/test_gpu_launch_plan.py).

A case is (model, engine max_batch, batch, switches).  The models are the model programs themselves, compiled from their synthetic_* weights with
seed 1234 -- the executor's matchers key on exact model geometry, nothing smaller exercises them -- and the batches are each fold threshold of the
executor and the value just below it.  Switches: 'ssd_decode' / 'yolo_decode' turn the decoding epilogues on (dd_net_ssd_decode,
dd_net_yolo_decode); an upper-case name is an environment variable the executor reads on every forward."""
import hashlib
import os

import numpy as np

MARS_BATCHES = (1, 159, 160, 255, 256, 511, 512, 1023, 1024)
SSD_THR = 0.3


def cases():
    out = [('mars64x32', 1024, b, {}) for b in MARS_BATCHES]
    out.append(('mars64x32', 1, 1, {}))                                           # an engine of one crop: split-K on
    for size in ('mars128x64', 'mars256x128'):
        out += [(size, 64, b, {}) for b in (1, 63, 64)]
        out.append((size, 64, 64, {'DD_STEM_WIDE': '1'}))
    for b in (1, 15, 16, 95, 96, 159, 160):
        out += [('ssd', 160, b, {}), ('ssd', 160, b, {'ssd_decode': 1})]
    for b in (1, 8):
        out += [('yolov5s', 8, b, {}), ('yolov5s', 8, b, {'yolo_decode': 1})]
    for q in ('ssd_u8_v1', 'ssd_u8_v2'):
        out += [(q, 24, b, {}) for b in (1, 23, 24)]
    return out


def case_id(case):
    model, max_batch, batch, sw = case
    return '%s/max%d/b%d%s' % (model, max_batch, batch, ''.join('/%s=%s' % kv for kv in sorted(sw.items())))


def _program(model):
    from deepdish_amd import nets, netsq, quantize
    if model.startswith('mars'):
        hw = tuple(int(v) for v in model[4:].split('x'))
        return nets.compile_mars(nets.synthetic_mars_weights(1234, hw), *hw)
    if model == 'ssd':
        return nets.compile_ssd_mobilenet(nets.synthetic_ssd_weights(1234))
    if model == 'yolov5s':
        return nets.compile_yolov5s(nets.synthetic_yolov5s_weights(1234))
    make = quantize.synthetic_ssd_quant_model if model == 'ssd_u8_v1' else quantize.synthetic_ssd_v2_quant_model
    return netsq.compile_ssd_mobilenet_quant(make(1234))


_engines = {}


def _engine(model, max_batch):
    """One engine per (model, max_batch), kept for the process: the MARS encoders with their buffers overlaid by lifetime, as the pipelines
    create them."""
    from deepdish_amd.engine import Net
    if (model, max_batch) not in _engines:
        _engines[(model, max_batch)] = Net(_program(model), max_batch=max_batch, shared=model.startswith('mars'))
    return _engines[(model, max_batch)]


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run(case):
    """One forward of the case on a seeded input -> dict(launches, variants, output | decoded): the full dd_net_op_launches and
    dd_net_op_variants vectors, the sha256 of the engine's output tensor, or of the decoded arrays where a decoding epilogue replaces it."""
    import torch
    from deepdish_amd.profile import net_op_launches
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import ptr
    import ctypes
    model, max_batch, batch, sw = case
    net = _engine(model, max_batch)
    prog = net.program
    env = {k: v for k, v in sw.items() if k.isupper()}
    saved = {k: os.environ.get(k) for k in env}
    x = np.random.default_rng(1234).integers(0, 256, (batch, prog.in_h, prog.in_w, 3), dtype=np.uint8)
    decode = bool(sw.get('ssd_decode') or sw.get('yolo_decode'))
    if decode != getattr(net, '_plan_decode', False):
        if model == 'ssd':
            net.ssd_decode(prog.meta['anchors'], SSD_THR, enable=decode)
        else:
            net.yolo_decode(decode)
        net._plan_decode = decode
    os.environ.update(env)
    try:
        net.forward(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    n = len(prog.ops)
    variants = np.zeros(n, dtype=np.int32)
    check(lib().dd_net_op_variants(net._h, ptr(variants), n, ctypes.byref(ctypes.c_int(0))), 'dd_net_op_variants')
    got = dict(launches=[int(v) for v in net_op_launches(net)], variants=[int(v) for v in variants])
    if sw.get('ssd_decode'):
        got['decoded'] = _sha(*net.ssd_decoded())
    elif sw.get('yolo_decode'):
        got['decoded'] = _sha(*net.yolo_decoded())
    elif 'box_tensor' in prog.meta:                       # the uint8 detectors: the class head is the output tensor, the box head beside it
        got['output'] = _sha(net.read(), net.read(tensor=prog.meta['box_tensor']))
    else:
        got['output'] = _sha(net.read())
    return got
