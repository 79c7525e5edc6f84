"""CPU: the uint8 SSD-MobileNet-v2 model form -- writer -> reader round trip, the reader's refusals, v1 files unchanged, TFLite's uint8
ADD restated against hand-worked cases, and the compiled program (residual ADDs, 24 channels stored as 32, v1's program untouched)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quant_v2_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def qm():
    from deepdish_amd import quantize
    return quantize.synthetic_ssd_v2_quant_model(1234)


def _same_layer(a, b, where):
    assert sorted(a) == sorted(b), where
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert v.dtype == b[k].dtype and np.array_equal(v, b[k]), (where, k)
        else:
            assert v == b[k] and type(v) is type(b[k]), (where, k, v, b[k])


def _write(qm, tmp_path, name='ssdmobilenetv2.tflite', edit=None):
    from deepdish_amd.tools import tflite_writer
    g = tflite_writer.ssd_mobilenet_v2_graph(qm)
    if edit is not None:
        edit(g)
    path = str(tmp_path / name)
    with open(path, 'wb') as f:
        f.write(g.tobytes())
    return path


def test_model_form(qm):
    from deepdish_amd import quantize
    assert qm['kind'] == 'ssd_mobilenet_v2_uint8'
    assert sorted(qm['add']) == sorted('b%d' % i for i in (2, 4, 5, 7, 8, 9, 11, 12, 14, 15))
    assert 'b0_expand' not in qm['layers'] and qm['layers']['b1_project']['w'].shape == (1, 1, 96, 24)
    assert all(qm['layers'][f'b{i}_project']['act'] == 'none' for i in range(17))
    assert qm['layers']['b13_expand']['w'].shape[3] == 576 and qm['layers']['conv_last']['w'].shape == (1, 1, 320, 1280)
    for a in qm['add'].values():
        assert set(a) == {'in1_scale', 'in1_zp', 'in2_scale', 'in2_zp', 'out_scale', 'out_zp', 'lo', 'hi'}
        m1, e1, m2, e2, mo, eo = quantize.add_multipliers(a)
        assert [(m1, -e1), (m2, -e2), (mo, -eo)] == quant_v2_ref.add_params(a)       # the product's and the test's statements agree


def test_synthetic_names_resolve(qm):
    from deepdish_amd.tools.weights_io import load_ssd_model, ssd_post_options
    kind, m = load_ssd_model('synthetic-ssd_mobilenet_v2-uint8')
    assert kind == 'uint8' and m['kind'] == 'ssd_mobilenet_v2_uint8'
    _same_layer(m['layers']['b2_project'], qm['layers']['b2_project'], 'b2_project')
    kind, s = load_ssd_model('synthetic-ssd_mobilenet_v2-uint8-sym')
    assert s['kind'] == 'ssd_mobilenet_v2_uint8' and all(L['w_zp'] == 128 for L in s['layers'].values())
    kind, v1 = load_ssd_model('synthetic-ssd_mobilenet_v1-uint8')
    assert v1['kind'] == 'ssd_mobilenet_v1_uint8'
    assert ssd_post_options(dict(m, post=dict(max_detections=20)))['max_detections'] == 20


def test_writer_reader_round_trip(qm, tmp_path):
    from deepdish_amd.tools import tflite_reader
    kind, r = tflite_reader.load_ssd_mobilenet(_write(qm, tmp_path))
    assert kind == 'uint8' and r['kind'] == 'ssd_mobilenet_v2_uint8'
    assert r['order'] == qm['order'] and r['input'] == qm['input'] and r['logistic'] == qm['logistic']
    assert sorted(r['layers']) == sorted(qm['layers'])
    for name in qm['layers']:
        _same_layer(qm['layers'][name], r['layers'][name], name)
    assert sorted(r['add']) == sorted(qm['add'])
    for b in qm['add']:
        _same_layer(qm['add'][b], r['add'][b], b)


def test_a_v1_file_reads_as_before(tmp_path):
    from deepdish_amd import quantize
    from deepdish_amd.tools import tflite_reader, tflite_writer
    v1 = quantize.synthetic_ssd_quant_model(1234)
    path = str(tmp_path / 'ssdmobilenetv1.tflite')
    tflite_writer.write_ssd_mobilenet(v1, path)
    kind, r = tflite_reader.load_ssd_mobilenet(path)
    assert kind == 'uint8' and r['kind'] == 'ssd_mobilenet_v1_uint8' and 'add' not in r
    assert r['order'] == v1['order']
    for name in v1['layers']:
        _same_layer(v1['layers'][name], r['layers'][name], name)


def _op(g, kind, output_name):
    ti = next(i for i, t in enumerate(g.tensors) if t['name'] == output_name)
    return next(o for o in g.ops if o['kind'] == kind and ti in o['outputs'])


def test_refusals_name_their_operator(qm, tmp_path, monkeypatch):
    from deepdish_amd.tools import tflite_reader, tflite_writer
    from deepdish_amd.tools.tflite_reader import UnsupportedModel

    def refused(model, edit=None):
        with pytest.raises(UnsupportedModel) as e:
            tflite_reader.load_ssd_mobilenet(_write(model, tmp_path, edit=edit))
        return str(e.value)

    # a depthwise extra layer (SSDLite)
    L = qm['layers']['extra1_2']
    c = L['w'].shape[2]
    dw = dict(L, kind='dw', w=np.full((3, 3, c), L['w_zp'], np.uint8), bias=np.zeros(c, np.int32))
    msg = refused(dict(qm, layers=dict(qm['layers'], extra1_2=dw)))
    assert 'DEPTHWISE_CONV_2D' in msg and 'SSDLite' in msg, msg
    # a 3x3 predictor
    Lb = qm['layers']['box1']
    msg = refused(dict(qm, layers=dict(qm['layers'], box1=dict(Lb, w=np.resize(Lb['w'], (3, 3) + Lb['w'].shape[2:])))))
    assert 'CONV_2D' in msg and '3x3 predictor' in msg, msg
    # a requantisation multiplier >= 1
    Lp = qm['layers']['b5_project']
    msg = refused(dict(qm, layers=dict(qm['layers'], b5_project=dict(Lp, out_scale=np.float32(1e-9)))))
    assert 'CONV_2D' in msg and 'multiplier >= 1' in msg, msg
    # a fused activation on ADD
    orig = tflite_writer.GraphWriter._options

    def relu6_add(self, b, kind, o):
        if kind == 'ADD' and o.get('act'):
            return b.table({0: ('i8', tflite_writer.ACT[o['act']]), 1: ('i8', 0)})
        return orig(self, b, kind, o)
    monkeypatch.setattr(tflite_writer.GraphWriter, '_options', relu6_add)
    msg = refused(qm, edit=lambda g: _op(g, 'ADD', 'b8/add')['options'].update(act='relu6'))
    assert 'ADD' in msg and 'relu6' in msg, msg
    monkeypatch.setattr(tflite_writer.GraphWriter, '_options', orig)
    # per-channel filters
    Lx = qm['layers']['b3_expand']
    cout = Lx['w'].shape[3]
    msg = refused(qm, edit=lambda g: next(t for t in g.tensors if t['name'] == 'b3_expand/weights').update(
        scale=np.full(cout, Lx['w_scale'], np.float32), zero_point=np.full(cout, Lx['w_zp'])))
    assert 'CONV_2D' in msg and 'per-channel' in msg, msg

    # a feature tap elsewhere: the first map's predictors on b12's expansion output (same shape as b13's)
    def retap(g):
        src = next(i for i, t in enumerate(g.tensors) if t['name'] == 'b13_expand')
        alt = next(i for i, t in enumerate(g.tensors) if t['name'] == 'b12_expand')
        for name in ('box0', 'cls0'):
            op = _op(g, 'CONV_2D', name)
            assert op['inputs'][0] == src
            op['inputs'][0] = alt
    msg = refused(qm, edit=retap)
    assert 'CUSTOM' in msg and 'b12_expand' in msg, msg


def test_add_restatement_against_hand_worked_cases():
    add = quant_v2_ref.add_u8
    # equal scales 1, output scale 2: (a - 128 + b - 128) / 2, halves away from zero
    eq = dict(in1_scale=1.0, in1_zp=128, in2_scale=1.0, in2_zp=128, out_scale=2.0, out_zp=128, lo=0, hi=255)
    assert quant_v2_ref.add_params(eq) == [(1 << 30, 0), (1 << 30, 0), (1 << 30, -19)]
    assert add(np.array([130]), np.array([131]), eq)[0] == 128 + 3                  # 5 / 2 = 2.5 -> 3
    assert add(np.array([125]), np.array([126]), eq)[0] == 128 - 3                  # -5 / 2 = -2.5 -> -3 (a negative sum)
    assert add(np.array([128]), np.array([128]), eq)[0] == 128
    assert add(np.array([255]), np.array([255]), eq)[0] == 255                      # 254 / 2 + 128 = 255
    assert add(np.array([255]), np.array([255]), dict(eq, out_zp=200))[0] == 255    # 327: clamped at 255
    assert add(np.array([0]), np.array([0]), dict(eq, out_zp=50))[0] == 0           # -78: clamped at 0
    # a 0.5 multiplier: s2 = s1 / 2, out scale 1 -> 3 * 1 + 3 * 0.5 = 4.5 -> 5
    half = dict(in1_scale=1.0, in1_zp=100, in2_scale=0.5, in2_zp=10, out_scale=1.0, out_zp=20, lo=0, hi=255)
    assert quant_v2_ref.add_params(half) == [(1 << 30, 0), (1 << 30, -1), (1 << 30, -18)]
    assert add(np.array([103]), np.array([13]), half)[0] == 25
    assert add(np.array([97]), np.array([7]), half)[0] == 15                        # -4.5 -> -5
    assert add(np.array([90]), np.array([0]), half)[0] == 5                         # -10 - 5 = -15
    # every pair of bytes: with power-of-two multipliers the fixed point is exact, i.e. the real sum rounded half away from zero
    a, b = np.meshgrid(np.arange(256), np.arange(256))
    out = add(a, b, half).astype(np.int64)
    exact = (a - 100) + 0.5 * (b - 10)
    away = np.where(exact >= 0, np.floor(exact + 0.5), np.ceil(exact - 0.5)).astype(np.int64)
    np.testing.assert_array_equal(out, np.clip(away + 20, 0, 255))


def test_compiled_v2_program(qm, monkeypatch):
    from deepdish_amd import netsq
    prog = netsq.compile_ssd_mobilenet_quant(qm)
    kinds = [int(o[0]) for o in prog.ops]
    assert netsq.OP_QDWPW not in kinds and netsq.OP_QADD not in kinds
    assert sum(1 for o in prog.ops if int(o[0]) == netsq.OP_QCONV and int(o[3]) >= 0) == 10
    assert prog.meta['kind'] == 'ssd_mobilenet_v2_uint8' and set(prog.meta) >= {'anchors', 'n_classes', 'box_tensor', 'cls_tensor', 'cls_row', 'feats', 'quant'}
    t = prog.tensors[prog.meta['layer_tensors']['b2']]
    assert (t['h'], t['w'], t['c']) == (75, 75, 32)                                  # 24 channels stored as two planes
    monkeypatch.setattr(netsq, 'ADD_FUSE', False)
    split = netsq.compile_ssd_mobilenet_quant(qm)
    assert sum(1 for o in split.ops if int(o[0]) == netsq.OP_QADD) == 10 and all(int(o[3]) < 0 for o in split.ops if int(o[0]) == netsq.OP_QCONV)


def test_phantom_rows_hold_the_zero_point(qm):
    """Channels 24..31 of a 24-channel tensor: filter rows = the weight zero point and bias 0, so the projection stores its zero point there;
    the next expansion's filter reads them with w = zw."""
    from deepdish_amd import netsq
    p = netsq.pad_channels(qm['layers']['b1_project'], cout=32)
    assert (p['w'][..., 24:] == qm['layers']['b1_project']['w_zp']).all() and (p['bias'][24:] == 0).all()
    e = netsq.pad_channels(qm['layers']['b2_expand'], cin=32)
    assert (e['w'][:, :, 24:, :] == qm['layers']['b2_expand']['w_zp']).all()
    from oracle import nets_quant
    x = np.random.default_rng(0).integers(0, 256, (1, 4, 4, 96), dtype=np.uint8)
    y = nets_quant.conv_u8(x, p)
    np.testing.assert_array_equal(y[..., :24], nets_quant.conv_u8(x, qm['layers']['b1_project']))
    assert (y[..., 24:] == p['out_zp']).all()


def _program_digest(env, expr):
    code = ('import hashlib, numpy as np; from deepdish_amd import quantize, netsq; P = netsq.compile_ssd_mobilenet_quant(%s); '
            'print(hashlib.sha256(np.concatenate([np.asarray(o) for o in P.ops]).tobytes() + bytes(P.blob)).hexdigest(), '
            'sum(int(o[0]) == netsq.OP_QADD for o in P.ops))' % expr)
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.split()


def test_v1_program_does_not_depend_on_the_add_switch():
    """v1's op words and weight blob are the same with DD_Q_ADD_FUSE=0 (read at compile time); v2's program takes the two-op form."""
    v1 = 'quantize.synthetic_ssd_quant_model(1234)'
    assert _program_digest({'DD_Q_ADD_FUSE': '1'}, v1) == _program_digest({'DD_Q_ADD_FUSE': '0'}, v1)
    v2 = 'quantize.synthetic_ssd_v2_quant_model(1234)'
    assert _program_digest({'DD_Q_ADD_FUSE': '0'}, v2)[1] == '10' and _program_digest({'DD_Q_ADD_FUSE': '1'}, v2)[1] == '0'
