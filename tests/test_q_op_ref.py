"""CPU: the reference and the cases of tests/test_gpu_q_ops.py stand on their own --
  * tests/q_op_ref.py equals the whole-model restatements (oracle/nets_quant.ssd_quant_forward, tests/quant_v2_ref.ssd_v2_forward) on three
    layers of each synthetic model, and its explicit-loop statement (the one that takes mutants) equals conv_u8 / dwconv_u8;
  * every case is lively in the reference alone (a comparison of clamped or constant bytes would be empty);
  * the literals a case expects -- (M, e, lo, hi), the kernel variant -- agree with the compiler's words and with the branch the case
    is there for;
  * every mutant of the reference changes at least one byte in every case it applies to, the one aimed at an edge a byte at that edge."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q_op_ref as R  # noqa: E402
import q_op_cases as Q  # noqa: E402
import quant_v2_ref  # noqa: E402
from oracle import nets_quant as nq  # noqa: E402

IDS = [c['id'] for c in Q.CASES]
_refs = {}


def ref_of(cid):
    """The chain reference of a case, computed once and shared (read-only)."""
    if cid not in _refs:
        _refs[cid] = Q.chain_reference(Q.BY_ID[cid])
        for v in _refs[cid].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _refs[cid]


# ------------------------------------------------------------------------------------------- the reference against the model restatements
def test_reference_equals_v1_forward_on_three_layers():
    from deepdish_amd import quantize
    qm = quantize.synthetic_ssd_quant_model(1234)
    Ls = qm['layers']
    fr = quantize.calibration_frames(1, seed=5)
    box, cls, kept = nq.ssd_quant_forward(qm, fr, keep=('conv0', 'dw1', 'pw1', 'pw13', 'extra1_1', 'extra1_2', 'extra2_2', 'extra3_2', 'extra4_2', 'pw11'))
    np.testing.assert_array_equal(R.conv(fr, Ls['conv0']), kept['conv0'])
    np.testing.assert_array_equal(R.conv(R.dw(kept['conv0'], Ls['dw1']), Ls['pw1']), kept['pw1'])
    np.testing.assert_array_equal(R.conv_slow(kept['extra1_1'], Ls['extra1_2']), kept['extra1_2'])          # 3x3 stride 2
    np.testing.assert_array_equal(R.conv_slow(kept['conv0'], Ls['dw1']), kept['dw1'])
    # the heads as rows: six maps into one tensor at their own offsets
    feats = [kept[f] for f in nq.FEATURE_LAYERS]
    n_cls = 91
    buf_c, buf_b, base = np.zeros((1, 1917 * 96), np.uint8), np.zeros((1, 1917 * 4), np.uint8), 0
    for k, (f, a) in enumerate(zip(feats, nq.ANCHORS_PER_MAP)):
        Lc, row_cols = R.rows_layer(Ls['cls%d' % k], a, n_cls)
        R.rows_write(buf_c, R.conv(f, Lc, (a * row_cols + 15) // 16 * 16), base * 96, a * 96, a * 96)
        R.rows_write(buf_b, R.conv(f, Ls['box%d' % k], (4 * a + 15) // 16 * 16), base * 4, a * 4, a * 4)
        base += f.shape[1] * f.shape[2] * a
    np.testing.assert_array_equal(buf_c.reshape(1, 1917, 96)[:, :, :91], cls)
    np.testing.assert_array_equal(buf_b.reshape(1, 1917, 4), box)


def test_reference_equals_v2_forward_on_three_layers():
    from deepdish_amd import quantize
    qm = quantize.synthetic_ssd_v2_quant_model(1234)
    Ls = qm['layers']
    fr = quantize.calibration_frames(1, seed=5)
    _, _, kept = quant_v2_ref.ssd_v2_forward(qm, fr, keep=('conv0', 'b1', 'b2_expand', 'b2_dw', 'b2_project', 'b2', 'b1_expand', 'b1_dw', 'b1_project'))
    np.testing.assert_array_equal(R.conv(kept['b1'], Ls['b2_expand'])[..., :kept['b2_expand'].shape[3]], kept['b2_expand'])
    np.testing.assert_array_equal(R.dw(kept['b2_expand'], Ls['b2_dw']), kept['b2_dw'])
    # the projection of 24 channels stored as 32 and the residual ADD behind it: the phantom channels hold the zero points
    res = R.phantom(kept['b1'], 32, qm['add']['b2']['in2_zp'])
    got = R.conv_add(kept['b2_dw'], Ls['b2_project'], res, qm['add']['b2'])
    np.testing.assert_array_equal(got[..., :24], kept['b2'])
    assert (got[..., 24:] == R.add_u8(np.uint8(qm['add']['b2']['in1_zp']), np.uint8(qm['add']['b2']['in2_zp']), qm['add']['b2'])).all()
    np.testing.assert_array_equal(R.conv_slow(kept['b1_expand'], Ls['b1_dw']), kept['b1_dw'])          # stride 2


# ------------------------------------------------------------------------------------------- the literals
@pytest.mark.parametrize('cid', IDS)
def test_fixed_point_literals_are_the_compilers_words(cid):
    """(M, e, lo, hi) of q_op_tuned.py (written from oracle/nets_quant.layer_fixed_point) = what deepdish_amd.quantize derives, layer by layer."""
    from deepdish_amd import quantize
    c = Q.BY_ID[cid]
    for name, L in Q.layers_of(c).items():
        m, shift = quantize.conv_multiplier(L)
        lo, hi = quantize.activation_range(L)
        assert (m, -shift, lo, hi) == Q.TUNED[cid][name]['fixed'], (cid, name)
        assert Q._fixed(L) == Q.TUNED[cid][name]['fixed'], (cid, name)


VARIANT_FIELDS = {'q_conv_k': 'kernel MQ ROWSUM NPF PIPE SPLIT Q16N merged magic add launches', 'q_pws_k': 'kernel K MW epi ROWSUM SAT merged', 'q_dw_k': 'kernel SAT magic chunks',
                  'q_dwm_k': 'kernel SAT magic chunks', 'q_dwpw_k': 'kernel CIN COUT STRIDE QTT form SAT chunks', 'q_conv0_k': 'kernel HL SAT chunks',
                  'q_add_k': 'kernel chunks', 'q_ssd_decode_k': 'kernel chunks'}


def op_index(c):
    """Which op of the case's program is the one under test (0 = the first layer, 1 = the feeder)."""
    return 0 if c['kind'] == 'conv0' else 2


@pytest.mark.parametrize('cid', IDS)
def test_expected_variant_is_the_branch_the_case_is_for(cid):
    """The literal variant of the op under test has the fields the case line names by hand (`want`), and the tuple has the shape
    profile.q_variant decodes."""
    from deepdish_amd import profile
    c = Q.BY_ID[cid]
    ops = Q.TUNED[cid]['ops']
    for code, v in ops:
        fields = VARIANT_FIELDS[v[0]].split()
        assert len(v) == len(fields), (cid, v)
        nt = {'q_conv_k': profile.QConvV, 'q_pws_k': profile.QPwsV, 'q_dw_k': profile.QDwV, 'q_dwm_k': profile.QDwV, 'q_dwpw_k': profile.QDwpwV,
              'q_conv0_k': profile.QConv0V, 'q_add_k': profile.QOtherV, 'q_ssd_decode_k': profile.QOtherV}[v[0]]
        assert list(nt._fields) == fields
        assert code not in (19, 20)
    v = dict(zip(VARIANT_FIELDS[ops[op_index(c)][1][0]].split(), ops[op_index(c)][1]))
    for k, want in c['want'].items():
        assert v.get(k) == want, (cid, k, v)
    if c['kind'] == 'dwpw' and c['want'].get('kernel') == 'q_dwm_k':
        assert len(ops) == 4 and ops[3][1][0] in ('q_conv_k', 'q_pws_k'), ops          # the two-op form: depthwise, then pointwise


def test_variant_words_round_trip():
    """profile.q_variant decodes the packing of include/deepdish_hip.h (packed here by hand from the header's table)."""
    from deepdish_amd import profile
    w = 1 | 3 << 4 | 1 << 7 | 2 << 8 | 1 << 11 | 3 << 12 | 1 << 14 | 0 << 15 | 1 << 16 | 1 << 17 | 1 << 18
    assert profile.q_variant(w) == ('q_conv_k', 3, True, 2, True, 3, True, False, True, True, 1)
    assert profile.q_variant(2 | 1 << 4 | 3 << 6 | 1 << 9 | 1 << 11 | 0 << 12 | 1 << 14) == ('q_pws_k', 512, 3, 'rows', True, 0, True)
    assert profile.q_variant(2 | 2 << 4 | 2 << 6 | 0 << 9 | 0 << 11 | 2 << 12) == ('q_pws_k', 1024, 2, 'q16', False, 2, False)
    assert profile.q_variant(3 | 1 << 8) == ('q_dw_k', 0, False, 1)
    assert profile.q_variant(4 | 1 << 4 | 1 << 5 | 2 << 8) == ('q_dwm_k', 1, True, 2)
    assert profile.q_variant(5 | 16 << 4 | 8 << 9 | 1 << 13 | 1 << 15 | 1 << 17 | 2 << 19 | 1 << 21) == ('q_dwpw_k', 512, 512, 1, 64, 'rowsum', 2, 1)
    assert profile.q_variant(5 | 1 << 4 | 1 << 9 | 1 << 13 | 2 << 15 | 3 << 17 | 0 << 19 | 1 << 21) == ('q_dwpw_k', 32, 64, 1, 128, 'dup', 0, 1)
    assert profile.q_variant(6 | 1 << 4 | 2 << 5 | 1 << 8) == ('q_conv0_k', True, 2, 1)
    assert profile.q_variant(7 | 1 << 8) == ('q_add_k', 1) and profile.q_variant(8) == ('q_ssd_decode_k', 1) and profile.q_variant(0) is None


# ------------------------------------------------------------------------------------------- liveliness
@pytest.mark.parametrize('cid', IDS)
def test_case_is_lively(cid):
    c = Q.BY_ID[cid]
    ref = ref_of(cid)
    layers = Q.layers_of(c)
    out = Q.tested_output(c, ref)
    name = 'conv0' if c['kind'] == 'conv0' else 'pw' if c['kind'] == 'dwpw' else 'cls' if c['kind'] in ('heads', 'decode') else 'op'
    if c['kind'] == 'conv_add':
        a = Q.add_params(c, layers)
        lo, hi, linear = a['lo'], a['hi'], False
    else:
        lo, hi = Q.TUNED[cid][name]['fixed'][2:]
        linear = layers[name]['act'] == 'none'
    if c['kind'] in ('rows', 'heads', 'decode') and c['op']['n_cols'] != 4:
        # (the phantom columns are one constant each: judged on the real ones, of the anchors the op writes)
        rc = (c['op']['n_cols'] + 15) // 16 * 16
        out = out.reshape(c['frames'], -1, rc)[:, :, :c['op']['n_cols']]
    if c['kind'] in ('rows', 'heads'):
        # the slack the op must leave alone is there: before the first row, behind the last, and in `pitch` cases inside every pixel's pitch
        for m in ([ref['rows_mask']] if c['kind'] == 'rows' else [ref['cls_mask'], ref['box_mask']]):
            assert not m[:, 0].any() and not m[:, -1].any() and m.any() and (~m).sum() >= 20
            if c['op'].get('pitch'):
                first, last = np.flatnonzero(m[0])[[0, -1]]
                assert not m[0, first:last + 1].all()
    if c['kind'] in ('heads', 'decode'):
        # the box rows of the same op: linear, so neither end need occur; not clamped, not constant
        b = ref['box'][ref['box_mask']]
        print('%s, box rows: %.1f %% at 0, %.1f %% at 255, %d distinct values' % (cid, 100 * (b == 0).mean(), 100 * (b == 255).mean(), len(np.unique(b))))
        assert (b == 0).mean() <= 0.35 and (b == 255).mean() <= 0.35 and len(np.unique(b)) >= 32
    at_lo, at_hi = float((out == lo).mean()), float((out == hi).mean())
    print('%s: %.1f %% at lo = %d, %.1f %% at hi = %d, %d distinct values' % (cid, 100 * at_lo, lo, 100 * at_hi, hi, len(np.unique(out))))
    assert at_lo <= 0.35 and at_hi <= 0.35
    if not linear:
        assert at_lo > 0 and at_hi > 0
    assert len(np.unique(out)) >= 32
    if 'feed' in ref:
        assert len(np.unique(ref['feed'])) >= 64
    assert out.min() >= lo and out.max() <= hi


# ------------------------------------------------------------------------------------------- mutants
def small(c):
    return c['frames'] <= 4 and c['hw'][0] * c['hw'][1] <= 64


def conv_cases(pred):
    return [c['id'] for c in Q.CASES if small(c) and pred(c)]


def _slow_op(c, layers, x, mut):
    """The op under test of a conv / dw / dwpw / conv0 case by the explicit statement, with faults."""
    k = c['kind']
    if k == 'conv0':
        return R.conv_slow(x, layers['conv0'], mut)
    if k == 'dwpw':
        return R.conv_slow(R.dw(x, layers['dw']), layers['pw'], mut) if 'pw_only' in mut else R.conv_slow(R.conv_slow(x, layers['dw'], mut), layers['pw'])
    return R.conv_slow(x, layers['op'], mut)


def _input_of(c, ref):
    return ref['frames'] if c['kind'] == 'conv0' else ref['feed']


def _plain(c, ref):
    return ref['conv0'] if c['kind'] == 'conv0' else ref['out'][..., :Q.layers_of(c)['op' if c['kind'] != 'dwpw' else 'pw']['w'].shape[-1]]


SLOW_KINDS = ('conv0', 'conv', 'dw', 'dwpw')
MUTANTS = {
    # name: (applies to, where the changed byte must lie: None = anywhere)
    'pad_side': lambda c: c['kind'] in SLOW_KINDS and _odd_pad(c),
    'shift_tap': lambda c: c['kind'] == 'conv0' or (min(c['hw']) >= 2 and (c['kind'] in ('dw', 'dwpw') or (c['kind'] == 'conv' and c['op']['k'] == 3))),      # (tap (0, 0) inside somewhere)
    'drop_plane': lambda c: c['kind'] == 'conv',
    'drop_rowsum': lambda c: (c['kind'] == 'conv' and c['op'].get('w_zp', 97) != 128) or (c['kind'] == 'conv0' and c['c0'].get('w_zp', 97) != 128),
    'next_bias': lambda c: c['kind'] in SLOW_KINDS,
    'floor_round': lambda c: c['kind'] == 'conv' and c['op'].get('act') == 'none',
    'byte_clamp': lambda c: c['kind'] in SLOW_KINDS and (c['op'].get('out_zp') == 6 or c['c0'].get('out_zp') == 6),
}


def _odd_pad(c):
    if c['kind'] == 'conv0':
        return any((-(-s // 2) - 1) * 2 + 3 - s == 1 for s in c['in_hw'])
    k = 3 if c['kind'] in ('dw', 'dwpw') else c['op']['k']
    s = c['op'].get('stride', 1)
    return any(max((-(-d // s) - 1) * s + k - d, 0) % 2 == 1 for d in c['hw'])


@pytest.mark.parametrize('mut', sorted(MUTANTS))
def test_mutant_changes_every_case_it_applies_to(mut):
    ids = [c['id'] for c in Q.CASES if small(c) and MUTANTS[mut](c)]
    assert len(ids) >= 2, mut
    for cid in ids:
        c, ref = Q.BY_ID[cid], ref_of(cid)
        layers = Q.layers_of(c)
        x = _input_of(c, ref)
        good = _slow_op(c, layers, x, ())
        np.testing.assert_array_equal(good, _plain(c, ref), err_msg=cid)          # the explicit statement is the reference
        m = (mut, 'pw_only') if c['kind'] == 'dwpw' and mut in ('next_bias', 'byte_clamp', 'drop_rowsum') else (mut,)
        bad = _slow_op(c, layers, x, m)
        changed = bad != good
        print('%s / %s: %.1f %% of the bytes change' % (mut, cid, 100 * changed.mean()))
        assert changed.any(), (mut, cid)
        if mut == 'pad_side':                               # the edge it is aimed at: the first or last row / column
            edge = np.zeros(changed.shape, bool)
            edge[:, 0], edge[:, -1], edge[:, :, 0], edge[:, :, -1] = True, True, True, True
            assert (changed & edge).any(), (mut, cid)
        if mut == 'drop_plane':                             # ... where the last plane's channels carry weight at all: everywhere
            assert changed.mean() > 0.2, (mut, cid)


def test_mutant_phantom_fragment_stored():
    """A natural-order launch whose last group holds phantom fragments (80 channels: 3 + 2, 112: 3 + 3 + 1) must not store them: plane
    c16 of a row is plane 0 of the next row -- or, behind the last row, the border.  The fault changes bytes there."""
    n = 0
    for cid in ('q16n_80_relu6', 'q16n_80_none', 'q16n_112_relu6', 'q16n_112_none', 'q16n_own_clamp', 'q16n_3x3_s2_112'):
        c, ref = Q.BY_ID[cid], ref_of(cid)
        zp = Q.layers_of(c)['op']['out_zp']
        raw = R.to_raw(ref['out'], zp)
        bad = raw.copy()
        nn, hp, c16, wp, _ = raw.shape
        flat = bad.reshape(nn, hp * c16, wp, 16)             # rows of planes: the plane behind the last one of row y is the first of row y + 1
        phantom_bytes = np.uint8(Q.R.conv(ref['feed'][:1, :1, :1], dict(Q.layers_of(c)['op'], w=np.full_like(Q.layers_of(c)['op']['w'], 128)))[0, 0, 0, 0]) ^ 0x80
        for y in range(1, hp - 1):
            flat[:, y * c16 + c16, 1:-1, :] = phantom_bytes
        changed = bad != raw
        assert changed.any(), cid
        assert changed[:, -1].any(), cid                     # the bottom border row
        print('phantom_fragment / %s: %.1f %% of the raw bytes change, %d of them in the border' % (cid, 100 * changed.mean(), int(changed[:, -1].sum())))
        n += 1
    assert n == 6


def test_mutant_rows_at_base_zero():
    """The second map of a rows tensor written at base_off = 0: its bytes land in the slack before the first map and on the first map's
    rows, and its own range keeps the fill."""
    c, ref = Q.BY_ID['rows_two_maps'], ref_of('rows_two_maps')
    layers = Q.layers_of(c)
    a, n_cols = c['op']['a'], c['op']['n_cols']
    L2, row_cols = R.rows_layer(layers['op2'], a, n_cols)
    npix2 = ref['down'].shape[1] * ref['down'].shape[2]
    lay = Q.rows_layout(c, row_cols, [c['hw'][0] * c['hw'][1], npix2])
    g1, g2 = lay['maps']
    bad = ref['rows'].copy()
    bad[:, g2['base_off']:g2['base_off'] + npix2 * g2['row_bytes']] = Q.FILL
    R.rows_write(bad, R.conv(ref['down'], L2, (a * row_cols + 15) // 16 * 16), 0, g2['row_bytes'], g2['cout_store'])
    changed = bad != ref['rows']
    print('rows_base_zero: %.1f %% of the bytes change' % (100 * changed.mean()))
    assert g1['base_off'] > 0 and changed[:, :g1['base_off']].any()          # the slack before the first map: the edge the fault is aimed at
    assert changed[:, g1['base_off']:g2['base_off']].any() and changed[:, g2['base_off']:].any()


def test_mutant_add_operands_swapped():
    ids = [c['id'] for c in Q.CASES if c['kind'] == 'conv_add' and Q.ADDS[c['op']['add']]['r1'] != Q.ADDS[c['op']['add']]['r2']]      # (equal scales: the sum commutes)
    assert len(ids) >= 6
    for cid in ids:
        c, ref = Q.BY_ID[cid], ref_of(cid)
        layers = Q.layers_of(c)
        a = Q.add_params(c, layers)
        bad = R.add_u8(ref['feed'], ref['proj'], a)
        changed = bad != ref['out']
        print('add_swapped / %s: %.1f %% of the bytes change' % (cid, 100 * changed.mean()))
        assert changed.any(), cid


# ------------------------------------------------------------------------------------------- the fused block's gate
def test_blocks_outside_the_launchers_rule_compile_to_two_ops():
    """netsq.dwpw_fits is the launcher's own rule (dd_netq_dwpw_fits, host code): a block on a map the fused kernel does not take compiles to
    a depthwise and a pointwise op -- 512 -> 512 on 20 x 20 (block 12 of a 320 x 320 model) used to compile to an OP_QDWPW that
    dd_net_forward refused."""
    from deepdish_amd import netsq
    assert netsq.dwpw_fits(512, 512, 1, 19, 19) and not netsq.dwpw_fits(512, 512, 1, 20, 20)
    for cin, cout, s in netsq.FUSED_SHAPES:                   # every block of the 300 x 300 model still runs fused
        size = {32: 150, 64: 150, 128: 75, 256: 38, 512: 19}[cin]
        assert netsq.dwpw_fits(cin, cout, s, size, size, 64 <= cin <= 128), (cin, cout, s)
    assert not netsq.dwpw_fits(48, 64, 1, 19, 19)            # no kernel for the shape
    for c in Q.CASES:
        if c['kind'] != 'dwpw':
            continue
        P, t = Q.build_program(c)
        kinds = [int(o[0]) for o in P.ops]
        if c['want']['kernel'] == 'q_dwpw_k':
            assert kinds == [netsq.OP_QCONV0, netsq.OP_QCONV, netsq.OP_QDWPW], c['id']
        else:
            assert kinds == [netsq.OP_QCONV0, netsq.OP_QCONV, netsq.OP_QDW, netsq.OP_QCONV], c['id']
