"""GPU: every fused launch of the f16 engine on its own -- mars_ws128_k, mars_pair64_k, res_unit_rows_k, res_pair_rows_k, conv3x3_pool_rows_k (plain
and <STEM>), stem_conv_pool_wide_k, conv3x3_s2_rows_k, conv3x3_c64_rows_k, ssd_front_k, dwpw_rows_k, conv_ws_dw_k -- against the float64 compositions
of tests/net_op_ref.py, at the crop counts where a workgroup's rings wrap, and against the layer-by-layer kernels of the same engine bit for bit.

For every case (tests/fused_op_cases.py) and crop count: the launch codes of its ops are asserted; every tensor the launch writes is compared,
element by element and pad channels included, with the reference within the bound derived from the arithmetic (net_op_ref's docstring; up to
2 CU + 1 crops every crop, above that the stated pick); and, where the process has another path, the same inputs run through the same engine in
chunks below the dispatch thresholds must give the same bits for every crop, and the tensors the fused launch keeps on the chip are refused.
That run writes the tensors between the layers; fed with them, the reference holds every layer of the launch to its own one-op bound
(net_op_ref.EXACT_MID), which is far tighter than the composition's.  A failure names the launch, the tensor, and the crop / pixel / channel.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import net_op_ref as R  # noqa: E402
import fused_op_cases as F  # noqa: E402
from net_op_rig import Rig  # noqa: E402

pytestmark = pytest.mark.gpu


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _codes(rig, b, case):
    got = tuple(rig.launches()[b.first_op:b.first_op + len(case.codes)])
    from deepdish_amd.profile import OPK_NAMES
    print('%s: ops %d.. ran as %s (%s)' % (case.name, b.first_op, got, ', '.join(OPK_NAMES.get(c, str(c)) for c in got)))
    return got


@pytest.mark.parametrize('case,n', F.PARAMS, ids=F.IDS)
def test_fused_launch(case, n, monkeypatch):
    if _cus() != F.CU:
        pytest.skip('the crop counts and the launchers\' literal grids are those of a %d-CU device; this one has %d' % (F.CU, _cus()))
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    img = F.images(case, n)
    rig = Rig(case.H, case.W, n, program_input=case.program_input, img=img)
    b = F.build(case, rig)
    rig.run(b.outs['out'])

    # 1. the launch
    assert _codes(rig, b, case) == case.codes, '%s at %d crops' % (case.name, n)

    # 2. every tensor it writes, against float64
    sel = F.pick(case, n)
    fused = {k: rig.raw(t).copy() for k, t in b.outs.items()}
    inp = {k: rig.raw(t)[sel].astype(np.float64) for k, t in b.inputs.items()}
    ref = F.reference(case, inp, img[sel])
    assert set(ref) >= set(fused)
    for k, got in fused.items():
        want, bnd = ref[k]
        assert got.shape[-1] == want.shape[-1]                     # all channels up to cs
        try:
            R.assert_within('%s %s, %d crops (%d compared)' % (case.name, k, n, len(sel)), got[sel].astype(np.float64), want, bnd)
        except AssertionError as e:
            raise AssertionError('%s -- crop index is into the compared crops %s...' % (e, sel[:8].tolist())) from None
    for t in b.hidden:                                           # a tensor the launch kept on the chip is not handed out
        with pytest.raises(Exception):
            rig.raw(t)

    # 3. the same engine, layer by layer: the same bits for every crop
    if case.chunk is None:
        return
    mids = [[] for _ in b.mids]
    for lo in range(0, n, case.chunk):
        rig.forward(img[lo:lo + case.chunk])
        got = rig.launches()[b.first_op:b.first_op + len(case.codes)]
        assert not set(got) & (F.FUSED_CODES | {F.OPK_FOLDED, F.OPK_FOLDED_PREV}), '%s: a chunk of %d crops ran as %s' % (case.name, case.chunk, got)
        for k, t in b.outs.items():
            one = rig.raw(t)
            np.testing.assert_array_equal(fused[k][lo:lo + len(one)].view(np.uint16), one.view(np.uint16),
                                          err_msg='%s %s at %d crops: crops %d.. differ from the layer-by-layer run' % (case.name, k, n, lo))
        for m, t in zip(mids, b.mids):
            m.append(rig.raw(t).copy())

    # 4. ... whose tensors between the layers are in memory: with those known, each layer of the launch is held to its own one-op bound
    if b.mids:
        known = [np.concatenate(m)[sel].astype(np.float64) for m in mids]

        def put(stage, v, ctx):
            if stage != 'mid.h16':
                return v
            t = known.pop(0)
            assert t.shape == v.shape, (t.shape, v.shape)
            return t
        R.HOOK, R.EXACT_MID = put, True
        try:
            tight = F.reference(case, inp, img[sel])
        finally:
            R.HOOK, R.EXACT_MID = None, False
        assert not known
        for k, got in fused.items():
            R.assert_within('%s %s, %d crops, intermediates known' % (case.name, k, n), got[sel].astype(np.float64), tight[k][0], tight[k][1])
