"""The cases of tests/test_gpu_q_ops.py and tests/test_q_op_ref.py, as data: one small uint8 program each --
    frames -> first layer (q_conv0_k, 32 channels) -> feeder (1x1 q_conv_k to the op's input channels, its stride brings the map down)
           -> the op under test.
A case names shapes, seeds, zero points, clamps and activation; weights are `w_zp + small integers` (amplitude `amp`), so that the shifts
of real models (e <= 8) are reachable.  The numbers that make a case lively -- per layer (bias0, bias step, weight scale), chosen from
quantiles of the REFERENCE's accumulators -- and everything a case expects -- (M, e, lo, hi) per layer, the launch codes and the kernel
variants -- are literals in tests/q_op_tuned.py, written once by `python tests/q_op_cases.py --tune` (tune() / predict() below: the
reference alone and a reading of the dispatcher netq_run_op; nothing is ever taken from the device).  `want` in a case line is the branch
the case is there for, by hand; tests/test_q_op_ref.py holds the literal variant to it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q_op_ref as R  # noqa: E402

try:
    from q_op_tuned import TUNED
except ImportError:                                           # only while the table is being written
    TUNED = {}

RELU6 = np.float32(6.0 / 255.0)                               # [0, 6] on 0 .. 255: the byte clamp
OWN = np.float32(0.03)                                        # with zero point 6: lo = 6, hi = 206 (a clamp of the layer's own)
IN_SCALE = np.float32(1.0 / 128.0)

CASES = []


def case(id, kind, frames=2, hw=(5, 7), fs=3, cin=64, in_hw=None, c0=None, feed=None, want=None, **op):
    """hw: the map the op reads; fs: the feeder's stride; in_hw: the frame (default: 2 fs hw -- even sizes, so that a batch of any
    frame count is a whole number of dwords, which the first layer asks for); c0 / feed: overrides of the first layer's / feeder's parameters; op: the op's own."""
    CASES.append(dict(id=id, kind=kind, frames=frames, hw=hw, fs=fs, cin=cin, in_hw=in_hw or (2 * fs * hw[0], 2 * fs * hw[1]),
                      c0=c0 or {}, feed=feed or {}, want=want or {}, op=op))


# ---- first layer: the op under test is the first layer itself (no feeder)
for _id, _kw in [('33x33x4', dict(in_hw=(33, 33), frames=4)),                       # 3 267-byte frames, a 4-aligned batch; 17 x 17, pad 1; 1 156 pixels
                 ('32x40', dict(in_hw=(32, 40), frames=1)),                           # 16 x 20: pad_t = 0, the minimum width, non-square
                 ('31x34', dict(in_hw=(31, 34), frames=2)),
                 ('zw128', dict(in_hw=(32, 40), c0=dict(w_zp=128), want=dict(HL=False))),
                 ('zw0_w255', dict(in_hw=(32, 40), c0=dict(w_zp=0, w255=True, amp=3), want=dict(HL=False))),
                 ('inzp0', dict(in_hw=(33, 33), frames=4, c0=dict(in_zp=0))),
                 ('inzp255', dict(in_hw=(33, 33), frames=4, c0=dict(in_zp=255))),
                 ('inzp255_zw0', dict(in_hw=(33, 33), frames=4, c0=dict(in_zp=255, w_zp=0, w255=True))),
                 ('sat1', dict(in_hw=(32, 40), c0=dict(w_zp=122, amp=5, wofs=118), want=dict(SAT=1))),
                 ('own_clamp', dict(in_hw=(31, 34), c0=dict(out_zp=6, out_scale=OWN), want=dict(SAT=0))),
                 ('own_clamp_zw128', dict(in_hw=(31, 34), c0=dict(out_zp=6, out_scale=OWN, w_zp=128), want=dict(SAT=0, HL=False)))]:
    _kw.setdefault('want', {})
    case('conv0_' + _id, 'conv0', **dict(dict(frames=2), **_kw))

# ---- q_conv_k, bordered interleaved output (ReLU6, a multiple of 64 channels)
for _cin in (16, 32, 64, 80, 256):
    case('q16_1x1_cin%d' % _cin, 'conv', cin=_cin, k=1, cout=64, want=dict(kernel='q_conv_k', MQ=4, Q16N=False, ROWSUM=True))
case('q16_1x1_zw128', 'conv', cin=80, k=1, cout=64, w_zp=128, want=dict(ROWSUM=False))
case('q16_3x3_s1_5x7', 'conv', k=3, cout=64, want=dict(SPLIT=3))
case('q16_3x3_s2_6x4', 'conv', hw=(6, 4), fs=4, k=3, stride=2, cout=64, want=dict(SPLIT=3))       # even sizes: pad before 0
case('q16_3x3_s2_5x7', 'conv', k=3, stride=2, cout=64, want=dict(SPLIT=3))                         # odd sizes: pad before 1
case('q16_3x3_64to256', 'conv', k=3, cout=256, w_zp=128, want=dict(SPLIT=3, ROWSUM=False))
case('q16_3x3_own_clamp', 'conv', k=3, cout=64, out_zp=6, out_scale=OWN)
case('q16_map1x1', 'conv', hw=(1, 1), fs=16, k=3, cout=64, frames=3, want=dict(magic=False))
case('q16_map1x5', 'conv', hw=(1, 5), fs=16, k=3, cout=64)
case('q16_map2x2', 'conv', hw=(2, 2), fs=8, k=3, stride=2, cout=64, frames=3)
case('q16_1x1_m35', 'conv', hw=(5, 7), frames=1, k=1, cout=128)                                        # m % 32 = 3
case('q16_1x1_m48', 'conv', hw=(4, 4), fs=4, frames=3, k=1, cout=64)                                   # m % 32 = 16
case('q16_3x3_unsplit', 'conv', hw=(19, 19), fs=1, frames=23, k=3, cout=256, want=dict(SPLIT=1, PIPE=True))          # 4 * ceil(8303 / 32) = 1 040 items
case('q16_1x1_nopipe', 'conv', hw=(40, 40), fs=1, frames=21, cin=16, k=1, cout=512, want=dict(SPLIT=1, PIPE=False))  # 8 * 1 050 = 8 400 items

# ---- q_conv_k, natural output (any multiple of 16 channels; ReLU6 or linear; the residual ADD)
for _cout, _mq in ((16, 1), (32, 2), (48, 3), (80, 3), (112, 3)):
    for _act in ('relu6', 'none'):
        case('q16n_%d_%s' % (_cout, _act), 'conv', k=1, cout=_cout, act=_act, epi='q16n', out_zp=0 if _act == 'relu6' else 131,
             want=dict(Q16N=True, MQ=_mq))
case('q16n_64_none', 'conv', k=1, cout=64, act='none', epi='q16n', out_zp=120, want=dict(Q16N=True, MQ=2))
case('q16n_model24', 'conv', k=1, cout=24, act='none', epi='q16n', out_zp=140, want=dict(Q16N=True, MQ=2))          # 24 channels stored as 32: phantom channels
case('q16n_own_clamp', 'conv', k=1, cout=80, epi='q16n', out_zp=6, out_scale=OWN, want=dict(Q16N=True, MQ=3))       # (lo = zo = 6, hi = 206: ReLU6's lo is its zero point -- no layer TFLite writes has lo > zo; the clamp is the layer's own at both ends)
case('q16n_3x3_s2_112', 'conv', k=3, stride=2, cout=112, act='none', epi='q16n', out_zp=128, want=dict(Q16N=True, MQ=3, SPLIT=3))
ADDS = dict(equal=dict(r1=1.0, r2=1.0, lo=0, hi=255), one_to_8=dict(r1=1.0, r2=8.0, lo=0, hi=255), eight_to_1=dict(r1=8.0, r2=1.0, lo=0, hi=255),
            own_clamp=dict(r1=1.0, r2=2.0, lo=10, hi=200))
for _c, _a, _z1, _fz in ((16, 'equal', 128, 0), (80, 'one_to_8', 0, 0), (96, 'eight_to_1', 255, 0), (80, 'own_clamp', 128, 255), (16, 'one_to_8', 255, 255)):
    for _hw, _fs in (((3, 5), 4), ((1, 1), 16)):
        if _hw == (1, 1) and _c == 16:                          # (a 1 x 1 map of 16 channels is too few bytes to be lively)
            continue
        _feed = dict(act='none', out_zp=255) if _fz == 255 else {}
        _id = 'add_%d_%s_z%d_%d_%dx%d' % (_c, _a, _z1, _fz, _hw[0], _hw[1])
        case(_id, 'conv_add', hw=_hw, fs=_fs, frames=4, cin=_c, k=1, cout=_c, act='none', epi='q16n', out_zp=_z1, add=_a, feed=_feed,
             want=dict(Q16N=True, add=True))

# ---- rows output (the SSD heads).  Every rows tensor has slack the op must not touch (rows_layout below): `lead` anchors before the first
# map, `tail` behind the last, and with `pitch` a pixel pitch of a + pitch anchors of which a are stored (cout_store < row_bytes: the dead
# channels of a fragment -- 12 of 16 -- would land in the gap).  The tensors start out as FILL, a byte no zero-initialised buffer holds.
case('rows_box12', 'rows', cin=64, a=3, n_cols=4, pitch=1, want=dict(kernel='q_conv_k', MQ=1))
case('rows_box24', 'rows', cin=64, a=6, n_cols=4, want=dict(kernel='q_conv_k', MQ=2))
case('rows_cls3x91', 'rows', cin=64, a=3, n_cols=91, want=dict(kernel='q_conv_k', MQ=4))
case('rows_cls2', 'rows', cin=64, a=3, n_cols=2, w_zp=128, want=dict(MQ=3, ROWSUM=False))
case('rows_cls17', 'rows', cin=80, a=6, n_cols=17, pitch=1, want=dict(MQ=4))
case('rows_two_maps', 'rows', cin=64, a=6, n_cols=17, second_map=True)
case('heads_3x3', 'heads', hw=(3, 3), fs=6, cin=512, a=6, n_cols=91, zw_cls=97, zw_box=97, want=dict(kernel='q_conv_k', merged=True, launches=1))
case('heads_3x3_cls128', 'heads', hw=(3, 3), fs=6, cin=512, a=6, n_cols=91, pitch=1, zw_cls=128, zw_box=97, want=dict(kernel='q_conv_k', merged=True, ROWSUM=True))
case('heads_3x3_box128', 'heads', hw=(3, 3), fs=6, cin=512, a=6, n_cols=91, zw_cls=97, zw_box=128, want=dict(kernel='q_conv_k', merged=True, ROWSUM=True))
case('heads_19x19_pws', 'heads', hw=(19, 19), fs=1, frames=23, cin=512, a=3, n_cols=91, pitch=1, zw_cls=97, zw_box=97,
     want=dict(kernel='q_pws_k', K=512, MW=3, epi='rows', merged=True))
for _cout, _kw, _sat in ((128, dict(), 2), (512, dict(amp=90), 1), (128, dict(out_zp=6, out_scale=OWN), 0)):
    case('pws_512to%d_sat%d' % (_cout, _sat), 'conv', hw=(19, 19), fs=1, frames=23, cin=512, k=1, cout=_cout,
         want=dict(kernel='q_pws_k', K=512, MW=4, SAT=_sat, epi='q16'), **_kw)
case('pws_1024to256', 'conv', hw=(10, 10), fs=2, frames=82, cin=1024, k=1, cout=256, w_zp=128, want=dict(kernel='q_pws_k', K=1024, MW=2, ROWSUM=False))
case('pws_m8191', 'conv', hw=(1, 8191), fs=1, frames=1, in_hw=(2, 16382), cin=512, k=1, cout=128, want=dict(kernel='q_conv_k', PIPE=True))     # one pixel short of q_pws_k's 8 192
case('pws_below_8192', 'conv', hw=(19, 19), fs=1, frames=22, cin=512, k=1, cout=128, want=dict(kernel='q_conv_k', PIPE=True))          # 7 942 pixels

# ---- depthwise
for _c in (16, 32, 96, 144):
    case('dw_c%d_s1' % _c, 'dw', hw=(5, 3), fs=6, cin=_c, want=dict(kernel='q_dwm_k', magic=_c > 16))
case('dw_s2_odd', 'dw', hw=(5, 3), fs=6, cin=32, stride=2, want=dict(kernel='q_dwm_k'))
case('dw_s2_even', 'dw', hw=(6, 4), fs=4, cin=96, stride=2, want=dict(kernel='q_dwm_k'))
case('dw_map1x1', 'dw', hw=(1, 1), fs=16, frames=4, cin=96, want=dict(kernel='q_dwm_k', magic=False))
case('dw_map7x1', 'dw', hw=(7, 1), fs=16, cin=32, want=dict(kernel='q_dwm_k', magic=False))
case('dw_own_clamp', 'dw', hw=(5, 7), cin=96, out_zp=6, out_scale=OWN, want=dict(kernel='q_dwm_k', SAT=0))
case('dw_byte_clamp', 'dw', hw=(5, 7), cin=96, want=dict(kernel='q_dwm_k', SAT=1))
case('dw_w255', 'dw', hw=(5, 7), cin=32, w_zp=0, w255=True, want=dict(kernel='q_dw_k'))
case('dw_e0', 'dw', hw=(1, 3), fs=16, frames=3, cin=32, amp=1, want=dict(kernel='q_dw_k'))       # two or three taps inside, weights -1 .. 1: a multiplier >= 0.5

# ---- fused block (q_dwpw_k): every instantiation at a small non-square geometry the launcher takes, and one it does not
DWPW = [(32, 64, 1), (64, 128, 2), (128, 128, 1), (128, 256, 2), (256, 256, 1), (256, 512, 2), (512, 512, 1)]
for _cin, _cout, _s in DWPW:
    _wo = 20 if _cin == 256 and _s == 2 else 22 if _cin == 512 else 21        # (the smallest non-square map the launcher's rule takes: 256 -> 512 on 38 x 42 and 512 -> 512 on 19 x 21 are outside it)
    _in = [((19, _wo), 'odd'), ((19, _wo), 'even')] if _s == 2 else [((19, _wo), '')]
    for (_ho, _wo), _par in _in:
        _hw = (_ho * _s - (_par == 'odd'), _wo * _s - (_par == 'odd'))
        for _n in (1, 3):
            case('dwpw_%d_%d_s%d%s_n%d' % (_cin, _cout, _s, _par, _n), 'dwpw', hw=_hw, fs=1, frames=_n, cin=_cin, cout=_cout, stride=_s,
                 want=dict(kernel='q_dwpw_k', CIN=_cin, COUT=_cout, STRIDE=_s, QTT=128 if _cin == 32 else 64))
case('dwpw_32_plain', 'dwpw', hw=(19, 21), fs=1, cin=32, cout=64, pw_zp=128, want=dict(kernel='q_dwpw_k', form='plain'))
case('dwpw_64_plain_sat1', 'dwpw', hw=(38, 42), fs=1, cin=64, cout=128, stride=2, pw_zp=128, pw_amp=120, want=dict(kernel='q_dwpw_k', form='plain', SAT=1))
case('dwpw_128_own_clamp', 'dwpw', hw=(19, 21), fs=1, cin=128, cout=128, out_zp=6, out_scale=OWN, want=dict(kernel='q_dwpw_k', form='hilo', SAT=0))
case('dwpw_256_rowsum', 'dwpw', hw=(19, 21), fs=1, cin=256, cout=256, want=dict(kernel='q_dwpw_k', form='rowsum', SAT=2))
case('dwpw_32_dup', 'dwpw', hw=(19, 21), fs=1, cin=32, cout=64, want=dict(kernel='q_dwpw_k', form='dup'))
case('dwpw_64_hilo', 'dwpw', hw=(38, 42), fs=1, cin=64, cout=128, stride=2, want=dict(kernel='q_dwpw_k', form='hilo'))
# just outside launch_q_dwpw's rule (evaluated on the CPU: netsq.dwpw_fits): these compile to the two-op form
# (the first map outside it at 19 output rows, widths from 19 up; 512 -> 512 on 20 x 20 is a 320 x 320 model's block 12)
for (_cin, _cout, _s), _hw in zip(DWPW, [(19, 255), (38, 102), (19, 63), (38, 102), (19, 47), (38, 42), (19, 20)]):
    case('dwpw_%d_%d_s%d_outside_%dx%d' % (_cin, _cout, _s, _hw[0], _hw[1]), 'dwpw', hw=_hw, fs=1, frames=1, cin=_cin, cout=_cout, stride=_s, want=dict(kernel='q_dwm_k'))
case('dwpw_512_20x20_two_ops', 'dwpw', hw=(20, 20), fs=1, cin=512, cout=512, want=dict(kernel='q_dwm_k'))
case('dwpw_narrow_two_ops', 'dwpw', hw=(19, 18), fs=1, cin=128, cout=128, want=dict(kernel='q_dwm_k'))              # wo < 19

# ---- decode
for _ncls, _hw in ((2, (5, 7)), (16, (5, 7)), (17, (5, 7)), (91, (5, 7)), (128, (3, 5))):
    case('decode_%d' % _ncls, 'decode', hw=_hw, fs=3 if _hw == (5, 7) else 4, cin=64, a=3, n_cols=_ncls, tie=(1, 2) if _ncls > 2 else None)

BY_ID = {c['id']: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ------------------------------------------------------------------------------------------- layers from a case
def frames_of(c):
    h, w = c['in_hw']
    rng = np.random.default_rng(abs(hash_id(c['id'])) % (1 << 31))
    yy, xx = np.mgrid[0:h, 0:w]
    base = 96 + 80 * np.sin(yy / 3.0)[..., None] * np.cos(xx[..., None] / 4.0 + np.arange(3))          # [h][w][3]: neighbouring pixels alike
    fr = rng.integers(0, 256, (c['frames'], h, w, 3)).astype(np.float64) * 0.6 + base[None] * 0.4
    return np.clip(np.round(fr), 0, 255).astype(np.uint8)


def hash_id(s):
    v = 0
    for ch in s.encode():
        v = (v * 131 + ch) % 1000003
    return v


def make_layer(kind, shape, seed, tuned, in_zp=0, in_scale=RELU6, w_zp=97, amp=3, wofs=0, w255=False, act='relu6', stride=1, out_zp=0, out_scale=RELU6):
    """tuned: (bias0, bias step, weight scale) -- literals of q_op_tuned.py -- or None while they are being chosen (bias 0, scale 1)."""
    rng = np.random.default_rng(seed)
    # wofs: the filters of even / odd output channels lean to one sign (accumulators wide enough for a shift above 8)
    w = np.clip(w_zp + rng.integers(-amp, amp + 1, shape) + wofs * (1 - 2 * (np.arange(shape[-1]) % 2)), 0, 255).astype(np.uint8)
    if w255:
        w.reshape(-1)[rng.integers(0, w.size, max(1, w.size // 97))] = 255
    cout = shape[-1]
    b0, bstep, w_scale = tuned if tuned is not None else (0, 0, 1.0)
    bias = (b0 + ((np.arange(cout) * 37) % 17 - 8) * bstep).astype(np.int32)
    return dict(kind=kind, w=w, w_zp=int(w_zp), w_scale=np.float32(w_scale), bias=bias, stride=stride, act=act, in_scale=np.float32(in_scale), in_zp=int(in_zp),
                out_scale=np.float32(out_scale), out_zp=int(out_zp))


def _t(c, name, tuned):
    t = (tuned if tuned is not None else TUNED.get(c['id'], {})).get(name)
    return None if t is None else t['tune']


def layers_of(c, tuned=None):
    """{name: layer dict} of a case: conv0, feed, op (and op2 / box / cls / dw / pw where the kind has them) -- plus 'add' parameters."""
    sd = hash_id(c['id'])
    out = {}
    c0 = dict(dict(w_zp=97, in_zp=128, amp=3), **c['c0'])
    out['conv0'] = make_layer('conv', (3, 3, 3, 32), sd + 1, _t(c, 'conv0', tuned), in_scale=IN_SCALE, stride=2, **c0)
    if c['kind'] == 'conv0':
        return out
    z0, s0 = out['conv0']['out_zp'], out['conv0']['out_scale']
    feed = dict(dict(w_zp=97, amp=3), **c['feed'])
    out['feed'] = make_layer('conv', (1, 1, 32, c['cin']), sd + 2, _t(c, 'feed', tuned), in_zp=z0, in_scale=s0, stride=c['fs'], **feed)
    zf, sf = out['feed']['out_zp'], out['feed']['out_scale']
    op, kind, cin = c['op'], c['kind'], c['cin']
    std = lambda keys: {k: op[k] for k in keys if k in op}
    if kind in ('conv', 'conv_add'):
        out['op'] = make_layer('conv', (op['k'], op['k'], cin, op['cout']), sd + 3, _t(c, 'op', tuned), in_zp=zf, in_scale=sf,
                               **std(('w_zp', 'amp', 'wofs', 'act', 'stride', 'out_zp', 'out_scale', 'w255')))
    elif kind == 'dw':
        out['op'] = make_layer('dw', (3, 3, cin), sd + 3, _t(c, 'op', tuned), in_zp=zf, in_scale=sf, **std(('w_zp', 'amp', 'stride', 'out_zp', 'out_scale', 'w255')))
    elif kind == 'dwpw':
        out['dw'] = make_layer('dw', (3, 3, cin), sd + 3, _t(c, 'dw', tuned), in_zp=zf, in_scale=sf, w_zp=op.get('dw_zp', 110), amp=op.get('dw_amp', 12), stride=op.get('stride', 1))
        out['pw'] = make_layer('conv', (1, 1, cin, op['cout']), sd + 4, _t(c, 'pw', tuned), in_zp=0, in_scale=RELU6, w_zp=op.get('pw_zp', 97), amp=op.get('pw_amp', 3),
                               **std(('out_zp', 'out_scale')))
    elif kind == 'rows':
        out['op'] = make_layer('conv', (1, 1, cin, op['a'] * op['n_cols']), sd + 3, _t(c, 'op', tuned), in_zp=zf, in_scale=sf, act='none', out_zp=op.get('out_zp', 117),
                               **std(('w_zp', 'amp')))
        if op.get('second_map'):
            out['down'] = make_layer('conv', (1, 1, cin, cin), sd + 5, _t(c, 'down', tuned), in_zp=zf, in_scale=sf, stride=2)
            out['op2'] = make_layer('conv', (1, 1, cin, op['a'] * op['n_cols']), sd + 6, _t(c, 'op2', tuned), in_zp=0, in_scale=RELU6, act='none', out_zp=op.get('out_zp', 117),
                                    out_scale=out['op']['out_scale'])
    elif kind in ('heads', 'decode'):
        out['cls'] = make_layer('conv', (1, 1, cin, op['a'] * op['n_cols']), sd + 3, _t(c, 'cls', tuned), in_zp=zf, in_scale=sf, act='none', out_zp=op.get('cls_zp', 150),
                                w_zp=op.get('zw_cls', 97))
        out['box'] = make_layer('conv', (1, 1, cin, op['a'] * 4), sd + 4, _t(c, 'box', tuned), in_zp=zf, in_scale=sf, act='none', out_zp=op.get('box_zp', 125),
                                w_zp=op.get('zw_box', 97))
        if op.get('tie'):                                   # two classes with one filter and one bias (a raised one): they tie wherever they win
            a_, b_ = op['tie']
            t_cls = _t(c, 'cls', tuned)
            for an in range(op['a']):
                out['cls']['bias'][an * op['n_cols'] + a_] += 0 if t_cls is None else 25 * t_cls[1]
                out['cls']['w'][..., an * op['n_cols'] + b_] = out['cls']['w'][..., an * op['n_cols'] + a_]
                out['cls']['bias'][an * op['n_cols'] + b_] = out['cls']['bias'][an * op['n_cols'] + a_]
    return out


def add_params(c, layers, tuned=None):
    """The residual ADD of a conv_add case: in1 = the projection's output, in2 = the feeder's; scales r1 : r2, the output's from q_op_tuned."""
    a = ADDS[c['op']['add']]
    t = (tuned if tuned is not None else TUNED.get(c['id'], {})).get('add', dict(out_scale=1.0, out_zp=0))
    return dict(in1_scale=np.float32(a['r1'] * 0.02), in1_zp=layers['op']['out_zp'], in2_scale=np.float32(a['r2'] * 0.02), in2_zp=layers['feed']['out_zp'],
                out_scale=np.float32(t['out_scale']), out_zp=int(t['out_zp']), lo=a['lo'], hi=a['hi'])


def anchors_of(c):
    """Seeded anchors of a decode case (ycenter, xcenter, h, w), one row per (pixel, anchor)."""
    n = c['hw'][0] * c['hw'][1] * c['op']['a']
    rng = np.random.default_rng(hash_id(c['id']) + 9)
    return np.stack([rng.uniform(0.1, 0.9, n), rng.uniform(0.1, 0.9, n), rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)], axis=1).astype(np.float32)


LOGISTIC = dict(out_scale=np.float32(1.0 / 256.0), out_zp=0)


# ------------------------------------------------------------------------------------------- the reference of a case
FILL = 0xA5                                                   # what a rows tensor of a case holds before the forward


def rows_layout(c, rw, npix):
    """Where the maps of a rows case write in a tensor of anchors of rw bytes (4: boxes; the padded class row): `lead` anchors of slack, then
    per map npix pixels at a pitch of (a + pitch) anchors of which the first a are stored, then `tail` anchors of slack.  The decode reads every
    anchor of its tensors: no slack there."""
    op = c['op']
    lead, tail, pitch = (0, 0, 0) if c['kind'] == 'decode' else (op.get('lead', 2), op.get('tail', 3), op.get('pitch', 0))
    maps, off = [], lead * rw
    for p in npix:
        maps.append(dict(base_off=off, row_bytes=(op['a'] + pitch) * rw, cout_store=op['a'] * rw))
        off += p * (op['a'] + pitch) * rw
    return dict(n_rows=off // rw + tail, maps=maps)


def op_reference(c, layers, x, res=None, tuned=None):
    """The op under test on its input bytes x (u8 [n,h,w,c]: the chain's, or the device's read-back feeder) ->
    {tensor name: expected bytes}: 'out' bordered [n,ho,wo,C]; rows kinds 'box' / 'cls' [n, frame bytes] with 'box_mask' / 'cls_mask'
    (bytes the op writes); dwpw: 'out' (and 'mid', the depthwise bytes, where the case compiles to two ops)."""
    kind, op = c['kind'], c['op']
    if kind == 'conv':
        return dict(out=R.conv(x, layers['op']))
    if kind == 'conv_add':
        return dict(out=R.conv_add(x, layers['op'], x, add_params(c, layers, tuned)), proj=R.conv(x, layers['op']))
    if kind == 'dw':
        return dict(out=R.dw(x, layers['op']))
    if kind == 'dwpw':
        mid = R.dw(x, layers['dw'])
        return dict(mid=mid, out=R.conv(mid, layers['pw']))
    a, n_cols = op['a'], op['n_cols']
    n, h, w, _ = x.shape

    def write(maps, rw):
        # maps: [(input, layer)] -> (bytes [n, n_rows * rw] from FILL, the mask of the bytes the op writes)
        lay = rows_layout(c, rw, [v.shape[1] * v.shape[2] for v, _ in maps])
        buf = np.full((n, lay['n_rows'] * rw), FILL, np.uint8)
        mask = np.zeros(buf.shape, bool)
        for (v, L), g in zip(maps, lay['maps']):
            R.rows_write(buf, R.conv(v, L, (a * rw + 15) // 16 * 16), g['base_off'], g['row_bytes'], g['cout_store'])
            mask |= R.rows_mask(buf.shape, v.shape[1] * v.shape[2], g['base_off'], g['row_bytes'], g['cout_store'])
        return buf, mask

    if kind == 'rows':
        box = n_cols == 4
        L, row_cols = (layers['op'], 4) if box else R.rows_layer(layers['op'], a, n_cols)
        maps, out = [(x, L)], {}
        if op.get('second_map'):
            out['down'] = R.conv(x, layers['down'])
            maps.append((out['down'], layers['op2'] if box else R.rows_layer(layers['op2'], a, n_cols)[0]))
        out['rows'], out['rows_mask'] = write(maps, row_cols)
        return out
    # heads / decode: a class and a box predictor on one map
    Lc, row_cols = R.rows_layer(layers['cls'], a, n_cols)
    cls, cls_mask = write([(x, Lc)], row_cols)
    box, box_mask = write([(x, layers['box'])], 4)
    return dict(cls=cls, box=box, cls_mask=cls_mask, box_mask=box_mask, row_cols=row_cols)


def chain_reference(c, layers=None, tuned=None):
    """The whole chain of a case on its frames, by the reference alone: dict(frames, conv0, feed, **op_reference)."""
    layers = layers or layers_of(c, tuned)
    fr = frames_of(c)
    out = dict(frames=fr, conv0=R.conv(fr, layers['conv0']))
    if c['kind'] != 'conv0':
        out['feed'] = R.conv(out['conv0'], layers['feed'])
        out.update(op_reference(c, layers, out['feed'], tuned=tuned))
    return out


def tested_output(c, ref):
    """The bytes of the op under test whose liveliness a case answers for."""
    k = c['kind']
    return ref['conv0'] if k == 'conv0' else ref['rows'][ref['rows_mask']] if k == 'rows' else ref['cls'][ref['cls_mask']] if k in ('heads', 'decode') else ref['out']


# ------------------------------------------------------------------------------------------- the program of a case
def build_program(c, layers=None):
    """-> (Program, {name: tensor id}).  Compiled through netsq.QBuilder, as the model compilers' ops are."""
    from deepdish_amd import netsq
    from deepdish_amd.nets import Program
    layers = layers or layers_of(c)
    P = Program(*c['in_hw'])
    B = netsq.QBuilder(P, 'one-op program ' + c['id'])
    t = dict(conv0=B.conv0(layers['conv0']))
    P.out_tensor = t['conv0']
    if c['kind'] == 'conv0':
        return P, t
    op, kind = c['op'], c['kind']
    epi_of = lambda L, e=None: netsq.QEPI_Q16N if (e == 'q16n' or L['act'] != 'relu6' or L['w'].shape[3] % 64) else netsq.QEPI_Q16
    Bp = netsq.QBuilder(P, 'one-op program ' + c['id'], pad=True)                  # (phantom channels: 24 stored as 32)
    conv = lambda src, L, e=None, **kw: (Bp if L['w'].shape[3] % 16 else B).conv(src, L, epi=epi_of(L, e), **kw)
    x = t['feed'] = conv(t['conv0'], layers['feed'])
    if kind == 'conv':
        t['out'] = conv(x, layers['op'], op.get('epi'))
    elif kind == 'conv_add':
        add = add_params(c, layers)
        t['out'] = B.conv(x, layers['op'], epi=netsq.QEPI_Q16N, res=x, add=add)
        t['proj'] = conv(x, layers['op'], 'q16n')                                   # the same ADD unfused: q_add_k behind the projection
        t['out_unfused'] = B.add_op(t['proj'], x, add)
    elif kind == 'dw':
        t['out'] = B.dw(x, layers['op'])
    elif kind == 'dwpw':
        n0 = len(P.ops)
        t['out'] = B.dwpw(x, layers['dw'], layers['pw'])
        if len(P.ops) - n0 == 2:
            t['mid'] = int(P.ops[n0][2])
    else:
        from deepdish_amd.nets import DT_U8
        a, n_cols = op['a'], op['n_cols']
        h, w = P.T(x)['h'], P.T(x)['w']

        def rows_tensor(n_rows, cols, rw):                  # plain rows that start out as FILL
            return P.tensor(n_rows, 1, cols, cs=rw, buf=P.buffer(n_rows * rw, DT_U8, fill=FILL), dtype=DT_U8)

        if kind == 'rows':
            srcs = [('op', x)]
            if op.get('second_map'):
                t['down'] = conv(x, layers['down'])
                srcs.append(('op2', t['down']))
            rw = 4 if n_cols == 4 else (n_cols + 15) // 16 * 16
            lay = rows_layout(c, rw, [P.T(s)['h'] * P.T(s)['w'] for _, s in srcs])
            t['rows'] = rows_tensor(lay['n_rows'], n_cols, rw)
            for (name, src), g in zip(srcs, lay['maps']):
                args = B.head_args(t['rows'], t['rows'], a, n_cols, rw, 0)[0 if n_cols == 4 else 1]
                B.conv(src, layers[name], epi=netsq.QEPI_ROWS, **dict(args, **g))
        else:
            if kind == 'decode':
                box_t, cls_t, cls_row = B.rows_tensors(h * w * a, n_cols)
            else:
                cls_row = (n_cols + 15) // 16 * 16
                box_t = rows_tensor(rows_layout(c, 4, [h * w])['n_rows'], 4, 4)
                cls_t = rows_tensor(rows_layout(c, cls_row, [h * w])['n_rows'], n_cols, cls_row)
            box_args, cls_args = B.head_args(box_t, cls_t, a, n_cols, cls_row, 0)
            box_args.update(rows_layout(c, 4, [h * w])['maps'][0])
            cls_args.update(rows_layout(c, cls_row, [h * w])['maps'][0])
            if kind == 'heads':
                B.conv_heads(x, layers['cls'], layers['box'], cls_args, box_args)
            else:
                B.conv(x, layers['box'], epi=netsq.QEPI_ROWS, **box_args)
                B.conv(x, layers['cls'], epi=netsq.QEPI_ROWS, **cls_args)
                B.decode(box_t, cls_t, layers['box'], layers['cls'], LOGISTIC, n_cols, h * w * a, cls_row)
            t['box'], t['cls'] = box_t, cls_t
    P.out_tensor = t.get('out', t.get('rows', t.get('cls', -1)))
    return P, t


# ------------------------------------------------------------------------------------------- choosing the literals (run once)
def _fixed(L):
    m, shift, lo, hi = R.nq.layer_fixed_point(L)
    return (int(m), int(-shift), int(lo), int(hi))


def _tune_layer(acc, L):
    """(bias0, bias step, weight scale) from the reference's accumulators (bias 0) of this layer on its reference input: a ReLU-type layer
    puts its 12th / 88th percentiles on the clamp's ends, a linear one its 1st / 99th 90 bytes either side of the zero point."""
    acc = acc.reshape(-1).astype(np.float64)
    if L['act'] == 'none':
        p_lo, p_hi = np.percentile(acc, [1, 99])
        mid = np.median(acc)
        mult = 180.0 / max(p_hi - p_lo, 1.0)
        b0 = -int(round(mid))
    else:
        lo, hi = R.nq.layer_fixed_point(dict(L, w_scale=np.float32(1.0)))[2:]
        p_lo, p_hi = np.percentile(acc, [12, 88])
        mult = (hi - lo) / max(p_hi - p_lo, 1.0)
        b0 = -int(round(p_lo)) + int(round((lo - L['out_zp']) / mult))
    bstep = int(max(1, round((p_hi - p_lo) / 60.0)))
    w_scale = float(np.float32(mult * float(L['out_scale']) / float(L['in_scale'])))
    return (b0, bstep, w_scale)


def tune(c):
    """The literals of one case, layer by layer along the chain, each layer tuned on the REFERENCE output of the tuned layers before it."""
    tuned = {}
    fr = frames_of(c)

    def settle(name, x):
        L = layers_of(c, tuned)[name]
        if L.get('kind') == 'dw':
            acc = R.acc_conv(x, L)
        else:
            acc = R.acc_conv(x[..., :L['w'].shape[2]], L)
        tuned[name] = dict(tune=_tune_layer(acc, L))
        L = layers_of(c, tuned)[name]
        tuned[name]['fixed'] = _fixed(L)
        return R.dw(x, L) if L.get('kind') == 'dw' else R.conv(x, L)

    x = settle('conv0', fr)
    if c['kind'] == 'conv0':
        return tuned
    x = settle('feed', x)
    k = c['kind']
    if k in ('conv', 'dw'):
        settle('op', x)
    elif k == 'conv_add':
        y = settle('op', x)
        layers = layers_of(c, tuned)
        a = add_params(c, layers, tuned)
        s = float(a['in1_scale']) * (y.astype(np.float64) - a['in1_zp']) + float(a['in2_scale']) * (x.astype(np.float64) - a['in2_zp'])
        p_lo, p_hi = np.percentile(s, [12, 88])
        so = (p_hi - p_lo) / (a['hi'] - a['lo'])
        tuned['add'] = dict(out_scale=float(np.float32(so)), out_zp=int(np.clip(round(a['lo'] - p_lo / so), 0, 255)))
    elif k == 'dwpw':
        settle('pw', settle('dw', x))
    elif k == 'rows':
        settle('op', x)
        if c['op'].get('second_map'):
            settle('op2', settle('down', x))
    else:
        settle('cls', x)
        settle('box', x)
        if k == 'decode':
            ref = chain_reference(c, tuned=tuned)
            n_cols, a = c['op']['n_cols'], c['op']['a']
            cls = ref['cls'].reshape(c['frames'], -1, ref['row_cols'])[0, :, :n_cols]
            box = ref['box'].reshape(c['frames'], -1, 4)[0]
            layers = layers_of(c, tuned)
            score = R.decode(box, cls, layers['box'], layers['cls'], LOGISTIC, anchors_of(c), 0.0)[1]
            tuned['thr'] = float(np.float32(np.median(score)))
    return tuned


def predict(c, tuned):
    """(launch code, variant tuple) per op of the case's program after the first layer's, from a reading of netq_run_op -- written into
    q_op_tuned.py as literals."""
    from deepdish_amd import netsq
    layers = layers_of(c, tuned)
    saved = TUNED.get(c['id'])
    TUNED[c['id']] = tuned
    try:
        P, t = build_program(c, layers)
    finally:
        if saved is None:
            del TUNED[c['id']]
        else:
            TUNED[c['id']] = saved
    n = c['frames']
    out = []
    for o in P.ops:
        kind = int(o[0])
        req = dict(M=int(o[32]), e=int(o[33]), lo=int(o[36]), hi=int(o[37]), linear=int(o[41]))
        byte = req['lo'] == 0 and req['hi'] == 255
        if kind == netsq.OP_QCONV0:
            out.append((0, ('q_conv0_k', bool(o[18]), (2 if req['e'] <= 8 else 1) if byte else 0, 1)))
        elif kind == netsq.OP_QCONV:
            s = P.T(int(o[1]))
            ho, wo, m = int(o[26]), int(o[27]), n * int(o[26]) * int(o[27])
            n_mfrag, epi, nfa = int(o[12]) // 16, int(o[15]), int(o[14])
            zwc, zwc_b = int(o[38]), int(o[28]) if nfa else 0
            rsum = zwc != 0 or (nfa and zwc_b != 0)
            k = int(o[5])
            pws = (epi != netsq.QEPI_Q16N and k == 1 and int(o[7]) == 1 and s['cs'] in (512, 1024) and m >= 8192 and n_mfrag >= 8 and
                   (epi == netsq.QEPI_ROWS or (not req['linear'] and req['e'] >= 1)))
            if pws:
                mw = (3 if epi == netsq.QEPI_ROWS and (n_mfrag + 2) // 3 <= 8 and n_mfrag % 4 != 0 else 4) if s['cs'] == 512 else 2
                rows = epi == netsq.QEPI_ROWS
                if rows or mw != 3:
                    sat = (2 if req['e'] <= 8 else 1) if (not rows and byte) else 0
                    out.append((0, ('q_pws_k', s['cs'], mw, 'rows' if rows else 'q16', bool(rsum), sat, bool(nfa))))
                    continue
            if epi == netsq.QEPI_Q16:
                mq = 4
            elif epi == netsq.QEPI_Q16N:
                mq = 3 if n_mfrag % 3 == 0 else 2 if n_mfrag % 2 == 0 else min(3, n_mfrag)
            else:
                mq = min(4, nfa if nfa else n_mfrag)
            groups = -(-nfa // mq) + -(-(n_mfrag - nfa) // mq) if nfa else -(-n_mfrag // mq)
            items = groups * -(-m // 32)
            split = k == 3 and items < 1024
            magic = wo > 1 and m * ho * wo < (1 << 32)
            add = int(o[3]) >= 0
            out.append((21 if add else 0, ('q_conv_k', mq, bool(rsum), 2, bool(split or items < 8192), 3 if split else 1, epi == netsq.QEPI_Q16N, bool(nfa), bool(magic), add, 1)))
        elif kind == netsq.OP_QDW:
            ho, wo, c16 = int(o[26]), int(o[27]), int(o[10]) // 16
            if int(o[20]) and req['e'] >= 1:
                out.append((17, ('q_dwm_k', int(byte), not (wo < 2 or c16 < 2), 1)))
            else:
                out.append((0, ('q_dw_k', 0, False, 1)))
        elif kind == netsq.OP_QDWPW:
            cin, cout = int(o[10]), int(o[11])
            rd = dict(e=int(o[23]), lo=int(o[24]), hi=int(o[25]))
            form = 'hilo' if int(o[18]) else 'rowsum' if int(o[38]) else 'dup' if int(o[47]) else 'plain'
            sat = (2 if rd['e'] <= 8 and req['e'] <= 8 else 1) if byte and rd['lo'] == 0 and rd['hi'] == 255 else 0
            out.append((0, ('q_dwpw_k', cin, cout, int(o[7]), 128 if cin == 32 else 64, form, sat, 1)))
        elif kind == netsq.OP_QADD:
            out.append((22, ('q_add_k', 1)))
        elif kind == netsq.OP_QSSD_DECODE:
            out.append((0, ('q_ssd_decode_k', 1)))
    return out


if __name__ == '__main__' and '--tune' in sys.argv:
    only = [a for a in sys.argv[1:] if not a.startswith('--')]
    table = dict(TUNED)
    for c in CASES:
        if only and c['id'] not in only and c['id'] in table:
            continue
        tuned = tune(c)
        tuned['ops'] = predict(c, tuned)
        table[c['id']] = tuned
        print(c['id'], {k: v.get('fixed') for k, v in tuned.items() if isinstance(v, dict) and 'fixed' in v}, file=sys.stderr)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'q_op_tuned.py'), 'w') as f:
        f.write('"""Literals of tests/q_op_cases.py, written by `python tests/q_op_cases.py --tune` from the reference alone (see there): per case and layer\n'
                '`tune` = (bias0, bias step, weight scale) and `fixed` = the expected (M, e, lo, hi); `add` the ADD\'s output quantisation; `thr` the decode\'s\n'
                'score threshold; `ops` = per op of the program the expected (launch code, kernel variant)."""\n')
        f.write('TUNED = {\n')
        for c in CASES:
            f.write('    %r: {\n' % c['id'])
            for k, v in table[c['id']].items():
                f.write('        %r: %r,\n' % (k, v))
            f.write('    },\n')
        f.write('}\n')
