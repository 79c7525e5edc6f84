"""GPU: mask_stream_count_k (csrc/gate.hip, dd_mask_stream_count, background.mask_stream_count) against np.count_nonzero per plane.
Every comparison is equality.  The shapes: one byte; 15-byte planes, so that every plane after the first starts off a 16-byte boundary;
planes shorter than, equal to and longer than one block's 16 KiB; 640 x 480, which takes 19 blocks per plane."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 3, 5), (2, 7, 19), (4, 48, 64), (2, 480, 640)]


def _contents(S, H, W):
    """name -> u8 [S, H, W]: the mask contents the kernel is held to."""
    hw = H * W
    out = {'zero': np.zeros((S, H, W), np.uint8), 'full': np.full((S, H, W), 255, np.uint8)}
    a = np.zeros(S * hw, np.uint8); a[0] = 127
    out['shadow_first'] = a.reshape(S, H, W)
    a = np.zeros(S * hw, np.uint8); a[-1] = 255
    out['last_byte'] = a.reshape(S, H, W)
    rng = np.random.default_rng(S * 1000 + hw)
    out['random'] = rng.choice(np.array([0, 1, 127, 255], np.uint8), size=(S, H, W))
    out['sparse'] = np.where(rng.random((S, H, W)) < 0.01, 1, 0).astype(np.uint8)
    return out


@pytest.fixture(scope='module')
def count():
    from deepdish_amd.background import mask_stream_count
    return mask_stream_count


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_counts_equal_count_nonzero_per_plane(count, shape):
    S, H, W = shape
    for name, m in _contents(S, H, W).items():
        want = [int(np.count_nonzero(m[z])) for z in range(S)]
        got = count(torch.from_numpy(m).cuda())
        assert got.dtype == np.int32 and got.tolist() == want, (shape, name)
        assert count(torch.from_numpy(m).cuda()).tolist() == got.tolist(), (shape, name, 'second call')
    assert count(torch.from_numpy(_contents(S, H, W)['full']).cuda()).tolist() == [H * W] * S


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_a_single_one_on_either_side_of_every_16_byte_boundary(count, shape):
    """One byte of value 1 in the last byte before a 16-byte ADDRESS boundary and in the first after it -- the seams between a plane's
    byte-wise head, its 16-byte body and its byte-wise tail -- for the first boundaries of every plane and the last of the buffer."""
    S, H, W = shape
    hw = H * W
    dev = torch.zeros((S, H, W), dtype=torch.uint8, device='cuda')
    base = dev.data_ptr()
    flat = dev.view(-1)
    bounds = [o for o in range(1, S * hw) if (base + o) % 16 == 0]
    picked = sorted(set(bounds[:3] + bounds[-2:] + [b for z in range(S) for b in bounds if z * hw < b <= z * hw + 16]))
    for b in picked:
        for o in (b - 1, b):
            flat.zero_()
            flat[o] = 1
            want = [0] * S
            want[o // hw] = 1
            assert count(dev).tolist() == want, (shape, o)


def test_a_stream_list_reads_and_writes_only_what_it_names(count):
    """A subset in ascending order: n outputs in list order; a guard of sentinel ints behind the host output stays untouched; the planes
    that are not listed may hold anything."""
    from deepdish_amd._lib import lib, check, P
    from deepdish_amd.runtime import default_context, ptr
    S, H, W = 5, 7, 19
    rng = np.random.default_rng(7)
    m = rng.choice(np.array([0, 1, 127, 255], np.uint8), size=(S, H, W))
    dev = torch.from_numpy(m).cuda()
    for streams in ([1, 3], [0], [4], [0, 2, 4], [0, 1, 2, 3, 4]):
        assert count(dev, streams).tolist() == [int(np.count_nonzero(m[z])) for z in streams]
    assert count(dev, []).size == 0
    streams = np.array([1, 3], np.int32)
    out = np.full(2 + 6, -77, np.int32)
    check(lib().dd_mask_stream_count(default_context().handle, ptr(dev), S, H, W, streams.ctypes.data_as(P), 2, out.ctypes.data_as(P)))
    assert out[:2].tolist() == [int(np.count_nonzero(m[1])), int(np.count_nonzero(m[3]))] and (out[2:] == -77).all()
    # the unlisted planes are not read: poisoning them changes nothing
    m2 = m.copy(); m2[[0, 2, 4]] = 255
    assert count(torch.from_numpy(m2).cuda(), [1, 3]).tolist() == out[:2].tolist()


def test_bad_arguments_are_dd_e_arg(count):
    from deepdish_amd._lib import lib, P
    from deepdish_amd.runtime import default_context, ptr
    DD_E_ARG = -1
    ctx = default_context().handle
    dev = torch.zeros((2, 4, 4), dtype=torch.uint8, device='cuda')
    out = np.zeros(4, np.int32)
    o = out.ctypes.data_as(P)

    def call(ctx_, mask, S, H, W, streams, n, o_):
        a = None if streams is None else np.asarray(streams, np.int32)
        return lib().dd_mask_stream_count(ctx_, mask, S, H, W, None if a is None else a.ctypes.data_as(P), n, o_)
    assert call(ctx, ptr(dev), 2, 4, 4, None, 2, o) == 0
    assert call(None, ptr(dev), 2, 4, 4, None, 2, o) == DD_E_ARG
    assert call(ctx, None, 2, 4, 4, None, 2, o) == DD_E_ARG
    assert call(ctx, ptr(dev), 0, 4, 4, None, 0, o) == DD_E_ARG
    assert call(ctx, ptr(dev), 2, 0, 4, None, 2, o) == DD_E_ARG
    assert call(ctx, ptr(dev), 2, 4, -1, None, 2, o) == DD_E_ARG
    assert call(ctx, ptr(dev), 2, 4, 4, None, -1, o) == DD_E_ARG
    assert call(ctx, ptr(dev), 2, 4, 4, None, 1, o) == DD_E_ARG          # no list = all streams
    assert call(ctx, ptr(dev), 2, 4, 4, [0, 2], 2, o) == DD_E_ARG        # a stream that does not exist
    assert call(ctx, ptr(dev), 2, 4, 4, [-1], 1, o) == DD_E_ARG
    assert call(ctx, ptr(dev), 2, 4, 4, [0], 1, None) == DD_E_ARG
    assert b'dd_mask_stream_count' in lib().dd_last_error()
    assert call(ctx, ptr(dev), 2, 4, 4, [1], 0, None) == 0               # n = 0 does nothing
    with pytest.raises(ValueError, match='streams'):
        count(dev, [2])
    with pytest.raises(ValueError, match='mask_dev'):
        count(torch.zeros((2, 4, 4), dtype=torch.float32, device='cuda'))
