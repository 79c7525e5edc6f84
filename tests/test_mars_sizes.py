"""CPU: the three crop sizes of the re-ID encoders the reference ships (encoders/mars-64x32x3, mars-128x64x3, mars-256x128x3) as synthetic
weights, as model names and as op programs."""
import numpy as np
import pytest

from deepdish_amd import nets
from deepdish_amd.tools.weights_io import load_mars_weights

SIZES = [(64, 32), (128, 64), (256, 128)]


def test_default_size_weights_are_unchanged():
    """synthetic_mars_weights(seed) and synthetic_mars_weights(seed, (64, 32)) are the same arrays, name for name and bit for bit, and carry no
    '__in_hw__' entry (what every existing fixture and golden file was made from)."""
    a, b = nets.synthetic_mars_weights(1234), nets.synthetic_mars_weights(1234, (64, 32))
    assert list(a) == list(b) and '__in_hw__' not in a
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a['fc1/weights'].shape == (4096, 128)


@pytest.mark.parametrize('hw,rows', [((128, 64), 16384), ((256, 128), 65536)])
def test_larger_sizes_draw_the_same_layers_and_a_larger_fc1(hw, rows):
    """Every array in front of fc1 is drawn in the same order, so it equals the 64 x 32 draw; fc1 has (h/8)(w/8)128 rows and gain sqrt(2/K)."""
    a, b = nets.synthetic_mars_weights(1234), nets.synthetic_mars_weights(1234, hw)
    assert b['__in_hw__'] == hw
    assert b['fc1/weights'].shape == (rows, 128) and b['fc1/weights'].dtype == np.float32
    keys = list(a)
    for k in keys[:keys.index('fc1/weights')]:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert abs(float(b['fc1/weights'].std()) / np.sqrt(2.0 / rows) - 1.0) < 0.02


def test_synthetic_names_state_the_size():
    assert load_mars_weights('synthetic-mars-128x64x3')['__in_hw__'] == (128, 64)
    assert load_mars_weights('synthetic-mars-256x128x3')['__in_hw__'] == (256, 128)
    assert load_mars_weights('synthetic:77-mars-128x64x3.pb')['fc1/weights'].shape == (16384, 128)
    for name in ('synthetic-mars-64x32x3', 'synthetic'):
        wd = load_mars_weights(name)
        assert '__in_hw__' not in wd and wd['fc1/weights'].shape == (4096, 128)
    np.testing.assert_array_equal(load_mars_weights('synthetic-mars-128x64x3')['conv1_1/weights'],
                                  nets.synthetic_mars_weights(1234)['conv1_1/weights'])


@pytest.mark.parametrize('hw', SIZES)
def test_compile_mars_at_each_size(hw):
    """128 output values at every size; the first layer carries the fold marker (word 30) at all three widths; at widths 64 and 128 the 3x3
    layer and the pool stay two ops (the engine runs all three as one launch, or as three)."""
    wd = nets.synthetic_mars_weights(1234, hw)
    P = nets.compile_mars(wd, *hw)
    assert (P.in_h, P.in_w) == hw
    out = P.T(P.out_tensor)
    assert (out['h'], out['w'], out['c']) == (1, 1, 128) and P.meta['out_dim'] == 128
    assert P.ops[0][0] == nets.OP_STEM and P.ops[0][30] == 1
    pool = P.T(P.meta['tensors']['pool1'])
    assert (pool['h'], pool['w'], pool['c']) == (hw[0] // 2 - 1, hw[1] // 2 - 1, 32)
    if hw[1] == 32:
        assert P.ops[1][0] == nets.OP_CONV and P.ops[1][29] == 1
    else:
        assert P.ops[1][0] == nets.OP_CONV and P.ops[1][29] == 0 and P.ops[1][30] == 0
        assert P.ops[2][0] == nets.OP_MAXPOOL and P.ops[2][1] == P.ops[1][2]
    words, blob = P.serialize()
    assert words.dtype == np.int32 and len(blob) > 0


def test_other_sizes_still_compile_unfused():
    """A width the wide kernel does not take (96 x 48) keeps the three plain ops and no marker."""
    wd = nets.synthetic_mars_weights(5, (96, 48))
    P = nets.compile_mars(wd, 96, 48)
    assert P.ops[0][30] == 0 and P.ops[2][0] == nets.OP_MAXPOOL
