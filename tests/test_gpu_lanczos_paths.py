"""GPU: every path of ddk::resize_lanczos (csrc/image.hip) against Pillow at the smallest geometry that takes it -- equality only.
Each case first asks dd_resize_lanczos_plan which kernels the geometry runs and holds the answer to the branch its row names, then runs
the real calls: a batch of three frames (noise, all 255, a checkerboard that overshoots both ways) through dd_resize_lanczos_batch into
a sentinel-guarded buffer, and frame 0 alone through dd_resize_lanczos.

The switches (DD_LANCZOS_NO_WIDE, DD_LANCZOS_FUSED, DD_LANCZOS_DEBUG) are read once per process.  Run as a script
(`python tests/test_gpu_lanczos_paths.py out.npz CASE...`) this file is the child that runs the named cases under whatever the
environment sets and saves their plans and bytes."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

pytestmark = pytest.mark.gpu

H_STEPS = ('none', 'copy', 'swap_copy', 'h_row', 'h_scalar', 'band_wide', 'band_narrow', 'fused')      # DD_LANCZOS_H_* of deepdish_hip.h
V_STEPS = ('none', 'memcpy', 'v4', 'v_scalar', 'band_wide', 'band_narrow', 'fused')                    # DD_LANCZOS_V_*
BATCH = 3
LEAD, TAIL = 64, 256                                               # guard bytes around the output (LEAD keeps its 64-byte alignment)
ALL_FORMS = ((3, 0), (3, 1), (4, 0), (4, 1))                       # (src_c, swap_rb): RGB, BGR, RGBA, BGRA


def fused(kh):
    return ('fused', 'fused', kh, 1)


def band(kh, kv):
    return ('band_wide', 'band_wide', kh, kv)


def scalar(hs, vs):
    return (hs, vs, 0, 0)


# (branch, H, W, h, w, {(src_c, swap_rb): (h_step, v_step, h_ksteps, v_ksteps)}).  The window steps of a horizontal band table depend on
# the channel form (4-byte pixels widen the window, the swap moves its first and last byte), so every form states its own.
ROWS = [
    ('fused<1,1> upscale', 96, 128, 300, 300, {f: fused(1) for f in ALL_FORMS}),
    ('fused<1,1> upscale, QVGA', 240, 320, 300, 300, {(3, 1): fused(1)}),
    ('fused<2,1>, one row tile', 64, 96, 32, 48, {f: fused(2) for f in ALL_FORMS}),
    ('fused, partial second row tile', 80, 96, 40, 48, {(3, 1): fused(2)}),
    ('fused at h = 320', 96, 128, 320, 100, {(3, 1): fused(1)}),
    ('band at h = 324', 96, 128, 324, 100, {(3, 1): band(1, 1)}),
    ('band wide, horizontal KS 1 / 2', 528, 128, 300, 100, {(3, 0): band(1, 1), (3, 1): band(1, 1), (4, 0): band(2, 1), (4, 1): band(2, 1)}),
    ('band wide, horizontal KS 1, 640x480', 480, 640, 416, 416, {(3, 0): band(1, 1), (3, 1): band(2, 1)}),
    ('band wide, horizontal KS 3', 128, 1024, 64, 300, {(3, 1): band(3, 1), (4, 0): band(3, 1)}),
    ('band wide, horizontal KS 4 / table refused (5 steps)', 128, 2048, 64, 300,
     {(3, 0): band(4, 1), (3, 1): band(4, 1), (4, 0): scalar('h_scalar', 'v4'), (4, 1): scalar('h_scalar', 'v4')}),
    ('band wide, vertical KS 2', 256, 256, 100, 200, {(3, 1): band(1, 2)}),
    ('band wide, vertical KS 3', 576, 256, 100, 200, {(3, 1): band(1, 3)}),
    ('band wide, vertical KS 4', 1024, 256, 100, 200, {(3, 1): band(1, 4)}),
    ('vertical table refused (H < 64)', 48, 64, 24, 32, {f: scalar('h_row', 'v4') for f in ALL_FORMS}),
    ('h_scalar, ksize > HTAPS, tiny', 16, 96, 8, 20, {f: scalar('h_scalar', 'v4') for f in ALL_FORMS}),
    ('h_scalar ksize 41, H = 1080', 1080, 1920, 300, 300, {(3, 1): scalar('h_scalar', 'v4'), (4, 0): scalar('h_scalar', 'v4')}),
    ('h_row / h_scalar (row > 6144 bytes), H = 1080', 1080, 1920, 640, 640, {(3, 1): scalar('h_row', 'v4'), (4, 0): scalar('h_scalar', 'v4')}),
    ('h_row + v_scalar', 32, 96, 20, 41, {f: scalar('h_row', 'v_scalar') for f in ALL_FORMS}),
    ('h_scalar + v_scalar, tiny', 16, 96, 8, 21, {f: scalar('h_scalar', 'v_scalar') for f in ALL_FORMS}),
    ('h_scalar + v_scalar, 640x480', 480, 640, 150, 150, {(3, 1): scalar('h_scalar', 'v_scalar')}),
    ('horizontal only', 480, 640, 480, 300, {(3, 1): scalar('h_row', 'none'), (4, 0): scalar('h_row', 'none')}),
    ('vertical only', 480, 640, 300, 640,
     {(3, 0): scalar('none', 'v4'), (3, 1): scalar('swap_copy', 'v4'), (4, 0): scalar('copy', 'v4'), (4, 1): scalar('copy', 'v4')}),
    ('same size: memcpy / copies', 32, 36, 32, 36,
     {(3, 0): scalar('none', 'memcpy'), (3, 1): scalar('swap_copy', 'none'), (4, 0): scalar('copy', 'none'), (4, 1): scalar('copy', 'none')}),
]
CASES = [(H, W, h, w, c, s) + want for (_, H, W, h, w, forms) in ROWS for (c, s), want in sorted(forms.items())]
CASE_IDS = ['%dx%d-%dx%d-c%d-swap%d' % c[:6] for c in CASES]


# ------------------------------------------------------------------ inputs, expectation, the calls
@functools.lru_cache(maxsize=None)
def _rgb(H, W):
    """The RGB view of a geometry's three frames: noise, all 255, a checkerboard of 0 / 255 in cells of 3 rows x 5 pixels."""
    f = np.random.default_rng(H * 10007 + W).integers(0, 256, (BATCH, H, W, 3), dtype=np.uint8)
    f[1] = 255
    yy, xx = np.mgrid[0:H, 0:W]
    f[2] = (((yy // 3 + xx // 5) & 1) * 255).astype(np.uint8)[..., None]
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _want(H, W, h, w):
    """Pillow's resize of every frame: computed once per geometry, shared by its channel forms and by the switch tests."""
    from PIL import Image
    out = np.stack([np.asarray(Image.fromarray(fr).convert('RGB').resize((w, h), Image.LANCZOS)) for fr in _rgb(H, W)])
    out.setflags(write=False)
    return out


def _source(H, W, src_c, swap_rb):
    """The frames as the call is given them: red and blue swapped for swap_rb, a fourth (noise: it must be ignored) channel for src_c 4."""
    rgb = _rgb(H, W)
    px = rgb[..., ::-1] if swap_rb else rgb
    if src_c == 4:
        alpha = np.random.default_rng(H + W).integers(0, 256, (BATCH, H, W, 1), dtype=np.uint8)
        px = np.concatenate([px, alpha], axis=-1)
    return np.ascontiguousarray(px)


def _plan(ctx, H, W, src_c, swap_rb, h, w, batch, src_addr, dst_addr):
    from deepdish_amd._lib import lib, check
    hs, vs, kh, kv = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    check(lib().dd_resize_lanczos_plan(ctx.handle, H, W, src_c, swap_rb, h, w, batch, ctypes.c_void_p(src_addr), ctypes.c_void_p(dst_addr),
                                       None, ctypes.byref(hs), ctypes.byref(vs), ctypes.byref(kh), ctypes.byref(kv)), 'dd_resize_lanczos_plan')
    return (H_STEPS[hs.value], V_STEPS[vs.value], kh.value, kv.value)


def _run(case):
    """-> (plan of the batch call, its three frames, plan of the one-frame call, its frame); the guards around both outputs are checked."""
    import torch
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import default_context
    H, W, h, w, src_c, swap_rb = case[:6]
    ctx = default_context()
    src = ctx.to_device(_source(H, W, src_c, swap_rb))
    res = []
    for n in (BATCH, 1):
        nb = n * h * w * 3
        buf = torch.full((LEAD + nb + TAIL,), 0xA5, dtype=torch.uint8, device='cuda')
        torch.cuda.synchronize()                                  # the fill ran on torch's stream, the resize runs on the context's
        dst = buf.data_ptr() + LEAD
        plan = _plan(ctx, H, W, src_c, swap_rb, h, w, n, src.data_ptr(), dst)
        if n == 1:
            check(lib().dd_resize_lanczos(ctx.handle, ctypes.c_void_p(src.data_ptr()), H, W, src_c, swap_rb, ctypes.c_void_p(dst), h, w, None))
        else:
            check(lib().dd_resize_lanczos_batch(ctx.handle, ctypes.c_void_p(src.data_ptr()), n, H, W, src_c, swap_rb, ctypes.c_void_p(dst), h, w, None))
        host = ctx.to_host(buf)
        assert (host[:LEAD] == 0xA5).all() and (host[LEAD + nb:] == 0xA5).all(), 'bytes outside the output were written (batch %d)' % n
        res += [plan, host[LEAD:LEAD + nb].reshape(n, h, w, 3)]
    return tuple(res)


# ------------------------------------------------------------------ every path against Pillow
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_path_vs_pillow(case):
    H, W, h, w = case[:4]
    plan_n, got_n, plan_1, got_1 = _run(case)
    assert plan_n == case[6:], 'the geometry no longer takes the path this row is here for'
    assert plan_1 == plan_n
    want = _want(H, W, h, w)
    for i in range(BATCH):
        np.testing.assert_array_equal(got_n[i], want[i], err_msg='frame %d' % i)
    np.testing.assert_array_equal(got_1[0], got_n[0])


def test_the_table_reaches_every_path():
    """Every step dd_resize_lanczos_plan can name is the plan of some row (band-narrow only runs under DD_LANCZOS_NO_WIDE: below), and
    both band passes run with 1, 2, 3 and 4 window steps."""
    import torch
    from deepdish_amd.runtime import default_context
    ctx = default_context()
    mem = torch.empty(4096, dtype=torch.uint8, device='cuda')      # addresses with the alignment _run's buffers have; nothing is launched
    plans = []
    for case in CASES:
        H, W, h, w, src_c, swap_rb = case[:6]
        plans.append(_plan(ctx, H, W, src_c, swap_rb, h, w, BATCH, mem.data_ptr(), mem.data_ptr() + LEAD))
        assert plans[-1] == case[6:], case
    assert {p[0] for p in plans} == set(H_STEPS) - {'band_narrow'}
    assert {p[1] for p in plans} == set(V_STEPS) - {'band_narrow'}
    assert {p[2] for p in plans if p[0] == 'band_wide'} == {1, 2, 3, 4}
    assert {p[3] for p in plans if p[1] == 'band_wide'} == {1, 2, 3, 4}
    assert {p[2] for p in plans if p[0] == 'fused'} == {1, 2}


# ------------------------------------------------------------------ the switches, one fresh process each
BAND_CASES = [i for i, c in enumerate(CASES) if c[6] == 'band_wide']
_pick = lambda *key: CASES.index(next(c for c in CASES if c[:6] == key))
FUSED_CASE, BAND_CASE, ROW_CASE = _pick(96, 128, 300, 300, 3, 1), _pick(528, 128, 300, 100, 4, 0), _pick(48, 64, 24, 32, 3, 1)
FUSED_CASES = [i for i, c in enumerate(CASES) if c[6] == 'fused']


def _narrow(p):
    return ('band_narrow', 'band_narrow') + p[2:]


def _unfused(p):
    return ('band_wide', 'band_wide') + p[2:]


# environment -> (cases the child runs, what each default plan turns into)
SWITCHES = {
    'DD_LANCZOS_NO_WIDE=1': (BAND_CASES, _narrow),
    'DD_LANCZOS_FUSED=0': (FUSED_CASES, _unfused),
    'DD_LANCZOS_DEBUG=4': ([FUSED_CASE, BAND_CASE, ROW_CASE], lambda p: scalar('h_row', 'v4')),      # all three rows are short and narrow enough for h_row
    'DD_LANCZOS_DEBUG=1': ([FUSED_CASE, BAND_CASE, ROW_CASE], lambda p: scalar('h_scalar', 'v4') if p[0] == 'h_row' else p),
    'DD_LANCZOS_DEBUG=2': ([FUSED_CASE, BAND_CASE, ROW_CASE], lambda p: scalar('h_row', 'v_scalar') if p[1] == 'v4' else p),
}


@pytest.mark.parametrize('setting', sorted(SWITCHES))
def test_switch_in_a_child_process(setting, tmp_path):
    """The forced forms give Pillow's bytes too (the default path's: test_path_vs_pillow), and the plan says which form ran:
    band_resample_k<1..4> under DD_LANCZOS_NO_WIDE, the two banded launches under DD_LANCZOS_FUSED=0, the scalar kernels under
    DD_LANCZOS_DEBUG bit 4, lanczos_h_k for lanczos_h_row_k under bit 1, lanczos_v_k for lanczos_v4_k under bit 2."""
    which, becomes = SWITCHES[setting]
    name, value = setting.split('=')
    path = str(tmp_path / 'child.npz')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path] + [str(i) for i in which], env=dict(os.environ, **{name: value}),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(path) as z:
        for i in which:
            case = CASES[i]
            H, W, h, w = case[:4]
            assert tuple(z['plan%d' % i]) == tuple(str(v) for v in becomes(case[6:])), (setting, CASE_IDS[i])
            assert tuple(z['plan1_%d' % i]) == tuple(z['plan%d' % i])
            np.testing.assert_array_equal(z['out%d' % i], _want(H, W, h, w), err_msg=CASE_IDS[i])
            np.testing.assert_array_equal(z['out1_%d' % i][0], z['out%d' % i][0], err_msg=CASE_IDS[i])
    if setting == 'DD_LANCZOS_NO_WIDE=1':                          # band_resample_k in all four instantiations, in both passes
        assert {CASES[i][8] for i in which} == {1, 2, 3, 4} and {CASES[i][9] for i in which} == {1, 2, 3, 4}


if __name__ == '__main__':
    saved = {}
    for i in (int(a) for a in sys.argv[2:]):
        plan_n, got_n, plan_1, got_1 = _run(CASES[i])
        saved.update({'plan%d' % i: np.array([str(v) for v in plan_n]), 'out%d' % i: got_n,
                      'plan1_%d' % i: np.array([str(v) for v in plan_1]), 'out1_%d' % i: got_1})
    np.savez(sys.argv[1], **saved)
