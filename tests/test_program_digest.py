"""CPU: the f16 compilers emit, byte for byte, the programs they emitted before the op words got names (deepdish_amd/nets.py OP_FIELDS, HINT_*).
The literals are sha256(words + blob) of Program.serialize(), taken at the commit before that change with this same loop: every model from its
synthetic_* weights with seed 1234, once with every fusion switch on and once per switch turned off for the model the switch affects (a switch is
turned off by setting the attribute its environment variable sets)."""
import hashlib

import pytest

MARS_SWITCHES = ('STEM_POOL_FUSE', 'RES_UNIT_FUSE', 'RES_PAIR_FUSE', 'PAIR64_FUSE', 'PROJ_FUSE')          # attributes of nets.Program
SSD_SWITCHES = ('SSD_FRONT_FUSE', 'PW_DW_FUSE')
YOLO_SWITCHES = ('FOCUS32', 'FOCUS_FUSE', 'YOLO_SPP_FUSE', 'YOLO_C3_MERGE')                                # attributes of the module

DIGESTS = {
    ('mars64x32', None): 'c7cbefe3d7d513d52d0bf1c0f3f7b4c4ed38450c4de23cb9c7d896b01a42a41e',
    ('mars64x32', 'STEM_POOL_FUSE'): 'c1928f0bfb06ac37c877828fda33d5f6eb3ec2419674731bc824f2faae8b6571',
    ('mars64x32', 'RES_UNIT_FUSE'): 'c358ad29d12b679eb4946e2d88564f595004d268080b121a10d4788ea0d7f383',
    ('mars64x32', 'RES_PAIR_FUSE'): 'f7658b0d7828fcb46501807973876dc18e224d5ebb748ecd1f675009d11b64fd',
    ('mars64x32', 'PAIR64_FUSE'): 'e08f2fc7eb0f4f8135cedd17ef0b7b8a444918bcbcd1a51c5c38b43b3e80e2f2',
    ('mars64x32', 'PROJ_FUSE'): 'f95b01312e2e72d6de2b9ea6d79f73bc1803a348e20c4058a75074c45af00ecc',
    ('mars128x64', None): 'aff9bd62e151b08f6e6fb128c699b7497c507579721dc7376430ca048c051e0d',
    ('mars128x64', 'STEM_POOL_FUSE'): 'a024d45628028b957bf95938bbf4c556a0546aa1b23d9fe85ecd059e01391d95',
    ('mars128x64', 'RES_UNIT_FUSE'): 'a5ee7d260a3035573719a7def91e6ca086769ff57fb5033e6c3221922c43ad02',
    ('mars128x64', 'RES_PAIR_FUSE'): '24db780d36ef5d50a4d08af6f5b9a509862b3a2c669b62e3de4bc00295edca29',
    ('mars128x64', 'PAIR64_FUSE'): '8bb14d6e7da5af216ffb61d7ee60d796a959ab903dc0648d733e53a2e484852e',
    ('mars128x64', 'PROJ_FUSE'): '5f39e095080285c6ee4fd779e3d56b270bfb421688e91ea3f056535314a655f0',
    ('mars256x128', None): '8f31e984431be95a2d9cc7f1054e1035e4da2e36c170056f93d95548b554407d',
    ('mars256x128', 'STEM_POOL_FUSE'): '90c86546e793ad79a39e6b2ca3356536cb8c2fbd4cd3a6325a77a734acd94b7f',
    ('mars256x128', 'RES_UNIT_FUSE'): 'd5fd3e0505137085c6b5e54d91111beb048fcf664c0fe9ef5620d2fd5ca39ea2',
    ('mars256x128', 'RES_PAIR_FUSE'): '29bd1a2f9899bdefdfb5c0637f30be73303ebba11db91b0ed10801843a1dedce',
    ('mars256x128', 'PAIR64_FUSE'): '1301f8ea9da099a0299b08d7d798d94101a1e6f01594713150431571d97640b4',
    ('mars256x128', 'PROJ_FUSE'): '06ef2ebce7506eb4f4d49d2f838db06f7a4e2e24d921a79945d0962fd7d997ff',
    ('ssd', None): 'd914ba61c75c7e820a8b0b262e80f0e72600c20ded7e3cf6f059602be675911d',
    ('ssd', 'SSD_FRONT_FUSE'): '5f4da3becb587451002271125fbca47fb961271003d2da06deb28c614ddb6944',
    ('ssd', 'PW_DW_FUSE'): '4c4203cddd78ae844216f0566a9d374472f56389ddb96f5a45512a4a9d96fa08',
    ('yolov5s', None): 'a8184dead480169d8ad35453bba84f62dc4b6f93efe9649dcbabfd60839eaf6b',
    ('yolov5s', 'FOCUS32'): '9ae8963433fe03c2449c4795fd70b7b55f822d112ff5de89fb60e5be0726b3cd',
    ('yolov5s', 'FOCUS_FUSE'): '4a8ef0e6cf73f2e192ee43da87e547a31a908c3d810b5fec1f96670d338f9caa',
    ('yolov5s', 'YOLO_SPP_FUSE'): '9bcdf55e4beb2cf66a25f5e7ec3d9f42107adbb20c369581f9be75b756c25cd1',
    ('yolov5s', 'YOLO_C3_MERGE'): 'a521ffb42b618428a76f3393f3c358be4b6e01c9bf43c459c843a24b32d2a3af',
}

_weights = {}


def _compile(model):
    from deepdish_amd import nets
    if model.startswith('mars'):
        hw = tuple(int(v) for v in model[4:].split('x'))
        assert hw in nets.MARS_SIZES
        if model not in _weights:
            _weights[model] = nets.synthetic_mars_weights(1234, hw)
        return nets.compile_mars(_weights[model], *hw)
    if model not in _weights:
        _weights[model] = nets.synthetic_ssd_weights(1234) if model == 'ssd' else nets.synthetic_yolov5s_weights(1234)
    return nets.compile_ssd_mobilenet(_weights[model]) if model == 'ssd' else nets.compile_yolov5s(_weights[model])


def digest(model, off, setattr_):
    from deepdish_amd import nets
    for flag in MARS_SWITCHES + SSD_SWITCHES:
        setattr_(nets.Program, flag, flag != off)
    for flag in YOLO_SWITCHES:
        setattr_(nets, flag, flag != off)
    words, blob = _compile(model).serialize()
    return hashlib.sha256(words.tobytes() + blob).hexdigest()


def keys():
    out = []
    for model in ('mars64x32', 'mars128x64', 'mars256x128'):
        out += [(model, None)] + [(model, s) for s in MARS_SWITCHES]
    out += [('ssd', None)] + [('ssd', s) for s in SSD_SWITCHES]
    out += [('yolov5s', None)] + [('yolov5s', s) for s in YOLO_SWITCHES]
    return out


def test_every_case_has_a_literal():
    assert sorted(DIGESTS, key=str) == sorted(keys(), key=str)


@pytest.mark.parametrize('model,off', keys())
def test_program_is_byte_identical(model, off, monkeypatch):
    assert digest(model, off, monkeypatch.setattr) == DIGESTS[(model, off)]


if __name__ == '__main__':           # prints the table (run at the commit the literals are to be taken from)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for k in keys():
        print('    %r: %r,' % (k, digest(k[0], k[1], setattr)))
