"""CPU: the uint8 compilers emit, byte for byte, the programs they emitted before their op builders were lifted out of them into
netsq.QBuilder.  The literals are sha256(words + blob) of Program.serialize(), taken at the commit before the change from the
nested-closure compilers, with this same loop; a switch is turned off by setting the module attribute the environment variable sets."""
import hashlib

import pytest

DIGESTS = {
    ('v1', False, None): '8790526783a2e5a00857ed38b87f864229a568fe44c5c775e24784129e66d951',
    ('v1', True, None): '18ec019c7ee668746bb1873066693d812ac3a8b2a6ca1905d0c36326bd475a50',
    ('v2', False, None): 'c7783d68e297b447ee06b2f3bd5c5859e133eed24ca54ae26e2c108c991a466f',
    ('v2', True, None): '499fce34c6f53e896971ed45e607b80cdb7fa97338529b53e8d0fa4d7ef2ede9',
    ('v1', False, 'FUSE_BLOCKS'): '9b8e8d8b34074feff5d7dab87cca75d254d5506f9b410d8d469d681d49502a7d',
    ('v1', False, 'SPLIT_PW'): '70b31ca7a3ace4ce120b8250975ca974e6affb3f3340a3719190a9583875f0e7',
    ('v1', False, 'DUP32'): '51ae323914ff6727eb8c0c76d5b802b6034b749c2ec93932ec8712bc392d51e7',
    ('v1', False, 'MERGE_HEADS'): 'edeca84d36d0edcb6fdd4169e051508bf559db87e3aa96d54614674f920dba40',
    ('v2', False, 'ADD_FUSE'): 'f06419e24367f59c951899f48eb313d5dda290b327e6e46ee1487ebb2e572aec',
}

_models = {}


def _model(kind, sym):
    from deepdish_amd import quantize
    if (kind, sym) not in _models:
        make = quantize.synthetic_ssd_quant_model if kind == 'v1' else quantize.synthetic_ssd_v2_quant_model
        _models[(kind, sym)] = make(1234, symmetric_weights=sym)
    return _models[(kind, sym)]


@pytest.mark.parametrize('kind,sym,off', sorted(DIGESTS, key=str))
def test_program_is_byte_identical(kind, sym, off, monkeypatch):
    from deepdish_amd import netsq
    for flag in ('FUSE_BLOCKS', 'SPLIT_PW', 'DUP32', 'MERGE_HEADS', 'ADD_FUSE'):
        monkeypatch.setattr(netsq, flag, flag != off)
    monkeypatch.setattr(netsq, 'SPLIT_PW_MAX_CIN', 128)
    monkeypatch.setattr(netsq, 'SPLIT_PW_MIN_CIN', 64)
    words, blob = netsq.compile_ssd_mobilenet_quant(_model(kind, sym)).serialize()
    assert hashlib.sha256(words.tobytes() + blob).hexdigest() == DIGESTS[(kind, sym, off)]


def _layer(cin=64, cout=64, bias=0, in_scale=0.02, w_scale=0.01, out_scale=0.0235, out_zp=0):
    import numpy as np
    return dict(kind='conv', w=np.full((1, 1, cin, cout), 130, np.uint8), w_zp=128, w_scale=np.float32(w_scale), bias=np.full(cout, bias, np.int32), stride=1,
                act='relu6', in_scale=np.float32(in_scale), in_zp=0, out_scale=np.float32(out_scale), out_zp=out_zp)


def test_model_properties_are_refused_by_name_not_by_assert():
    """A bias that leaves 32 bits once the zero-point terms are folded in, a requantisation addend that leaves 62 bits and a first layer of
    another shape are properties of the model file: UnsupportedModel (python -O strips asserts, and such a file would run wrong)."""
    import numpy as np
    from deepdish_amd import netsq, quantize
    from deepdish_amd.nets import Program
    from deepdish_amd.tools.tflite_reader import UnsupportedModel

    def one_layer(L):
        P = Program(33, 33)
        B = netsq.QBuilder(P)
        x = P.qtensor(17, 17, L['w'].shape[2], L['in_zp'])
        return B.conv(x, L, 'layer')

    one_layer(_layer())                                                   # the same layer with an ordinary bias compiles
    # folded bias = bias - (za - 128) sum (w - 128) + ...: za = 0, 64 weights of +2 -> bias + 16 384 leaves int32
    with pytest.raises(UnsupportedModel, match='32 bits'):
        one_layer(_layer(bias=2 ** 31 - 1000))
    # ReLU6 with a multiplier of 2^-31 (e = 30) and zero point 255: zo << (31 + e) = 255 * 2^61
    tiny = _layer(in_scale=2.0 ** -20, w_scale=2.0 ** -11, out_scale=1.0, out_zp=255)
    m, shift = quantize.conv_multiplier(tiny)
    assert -shift + 31 >= 55
    with pytest.raises(UnsupportedModel, match='62 bits'):
        one_layer(tiny)
    with pytest.raises(UnsupportedModel, match='first layer'):
        netsq.pack_conv0(dict(_layer(), w=np.zeros((3, 3, 3, 16), np.uint8)))
