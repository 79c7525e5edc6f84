"""GPU: the launch shapes bench.py runs, tied to the oracle.  The headline runs 3 072 streams in two worker groups: 1 536 frames per
detector / Lanczos launch (3 072 with --groups 1), ~30 720 crops per encoder launch in an engine sized for 32 x 1 536 = 49 152 crops
(deepdish_amd/multipipe.py; 98 304 with --groups 1).  The kernels change form exactly in that range -- 32-bit offsets behind explicit
size guards, fallbacks above them -- so the tests here run those sizes and pick items on both sides of every offset limit they cross.

The reference has no such notion -- it runs one stream, one frame at a time (deepdish.py:1324-1340 upstream) -- so this is
the build's own batching and its own obligation: the kernels that only run from some batch size on (conv3x3_pool_rows_k<STEM>,
res_unit_rows_k, conv3x3_c64_rows_k, conv3x3_s2_rows_k, ssd_front_k, dwpw_rows_k, conv_ws_k, conv_ws_dw_k) must give, for
every image of a bench-sized launch, the bits of that image's own single-image forward, and those single-image forwards are
what tests/test_gpu_nets.py holds against oracle/nets_torch.py -- repeated here on images taken out of the big launch."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(got, want, atol, rtol):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    return float((err / (atol + rtol * np.abs(want.astype(np.float64)))).max())


def test_ssd_launch_of_384_frames_is_frame_independent_and_matches_the_oracle():
    """One 384-frame launch (bench: 384 streams per worker group): frames 0, 1, 2, n/2, n-1 bit-identical to their single-frame
    forwards; two of them against the f32 restatement at test_gpu_nets.py's per-element tolerance."""
    _ssd_launch(384)


def test_ssd_launch_of_1536_frames_is_frame_independent_and_matches_the_oracle():
    """--detector-dtype f16 at the headline's shape: one worker group = 1 536 frames per launch.  The first layers' activations hold at
    least 150 x 150 x 32 f16 values a frame (1.44 MB), so their byte offsets pass 2^31 no later than frame 1 491 (1 491 x 1 440 000 =
    2 147 040 000, 1 492 x 1 440 000 > 2^31): frames n/2 = 768 and n-1 = 1 535 lie on both sides of that point.  Same checks as at 384."""
    _ssd_launch(1536)


def _ssd_launch(n):
    from deepdish_amd import nets
    from deepdish_amd.engine import Net
    from deepdish_amd.profile import net_op_launches, OPK_NAMES
    from oracle import nets_torch
    wd = nets.synthetic_ssd_weights(1234)
    net = Net(nets.compile_ssd_mobilenet(wd), max_batch=n)
    rng = np.random.default_rng(384)
    x = rng.integers(0, 256, (n, 300, 300, 3), dtype=np.uint8)
    x[1] = 0; x[2] = 255
    net.forward(x)
    ran = {OPK_NAMES.get(int(c)) for c in net_op_launches(net)}
    assert {'ssd_front_k', 'dwpw_rows_k', 'conv_ws_k', 'conv_ws_dw_k'} <= ran, ran       # the bench's kernels did run
    full = net.read()[:, :, 0, :].copy()
    assert np.isfinite(full).all()
    picks = (0, 1, 2, n // 2, n - 1)
    for i in picks:
        net.forward(x[i:i + 1])
        np.testing.assert_array_equal(net.read()[0, :, 0, :], full[i], err_msg='frame %d' % i)
    two = [0, n - 1]
    want = nets_torch.ssd_forward(wd, x[two], w16=True)
    assert _close(full[two], want, 8e-3, 1e-2) <= 1.0


@pytest.mark.parametrize('n', [7680, 15360, 30720, 49152, 98304])
def test_mars_launch_of_7680_crops_is_crop_independent_and_matches_the_oracle(n):
    """One 7 680-crop launch (384 streams x 20 detections: conv3x3_pool_rows_k<STEM> with one unit per crop, the residual-unit
    and conv3_x row kernels on every CU): crops 0, 1, 2, n/2, n-1 bit-identical to single-crop forwards; eight crops
    against the f32 restatement within test_gpu_nets.py's tolerance (5e-3 absolute, 5e-4 cosine).

    30 720 = the headline's launch (1 536 streams x 20), 49 152 = its engine (32 x 1 536), 98 304 = the engine of --groups 1.  The
    largest tensor the fused stem writes is 32 KB a crop (f16 64 x 16 x 16): byte offsets pass 2^31 at crop 65 536.  The unfused stem's
    conv1_1 (f16 64 x 32 x 32, 128 KB a crop) passes 2^31 bytes at crop 16 384 and 2^31 elements at crop 32 768 (test_gpu_switches.py
    runs that form at 49 152).  Picked crops lie on both sides of each point: 16 383 / 16 384, 32 767 / 32 768, 65 535 / 65 536.
    From 30 720 crops the single-crop forwards reuse the big engine after its output is copied out (one engine of that size at a time)."""
    from deepdish_amd import nets
    from deepdish_amd.engine import Net
    from deepdish_amd.profile import net_op_launches, OPK_NAMES
    from oracle import nets_torch
    wd = nets.synthetic_mars_weights(1234)                         # 15 360 = 768 streams x 20 detections: the default bench's launch since round 5
    net = Net(nets.compile_mars(wd), max_batch=n)
    rng = np.random.default_rng(7680)
    x = rng.integers(0, 256, (n, 64, 32, 3), dtype=np.uint8)
    x[1] = 0; x[2] = 255
    net.forward(x)
    ran = {OPK_NAMES.get(int(c)) for c in net_op_launches(net)}
    assert {'conv3x3_pool_rows_k<STEM>', 'res_pair_rows_k', 'mars_pair64_k', 'mars_ws128_k'} <= ran, ran
    full = net.read()[:, 0, 0, :].copy()
    np.testing.assert_allclose(np.linalg.norm(full.astype(np.float64), axis=1), 1.0, atol=1e-4)
    if n <= 15360:
        one = Net(nets.compile_mars(wd), max_batch=n)              # same engine size: same split-K decisions
        picks = (0, 1, 2, n // 2, n - 1)
        eight = [0, 1, 2, 3, n // 2, n // 2 + 1, n - 2, n - 1]
    else:
        one = net
        picks = sorted({i for i in (0, 1, 2, 16383, 16384, 32767, 32768, 65535, 65536) if i < n} | {n // 2, n - 1})
        eight = [i for i in (0, 32768, n // 2, n - 1) if i < n]
        for i in (16384, 65536, 1, n - 2, 16383, 2, 3):
            if len(eight) < 8 and i < n and i not in eight:
                eight.append(i)
        assert len(set(eight)) == 8 and n - 1 in eight and (n <= 32768 or 32768 in eight)
    for i in picks:
        one.forward(x[i:i + 1])
        np.testing.assert_array_equal(one.read()[0, 0, 0, :], full[i], err_msg='crop %d' % i)
    del one, net
    want = nets_torch.mars_forward(wd, x[eight], w16=True)
    got = full[eight]
    assert np.abs(got - want).max() < 5e-3
    assert (1.0 - np.sum(got * want, axis=1)).max() < 5e-4


@pytest.mark.parametrize('batch', [192, 256, 300, 384])
def test_pointwise_plus_depthwise_launch_at_the_bench_batch_sizes(batch):
    """conv_ws_dw_k takes whole frames per worker: 256 frames = 2 per worker, 384 = 3 (the bench's case: another ring phase),
    192 and 300 = uneven (only the layer whose frames balance over its workers fuses, the others run as two launches).
    Whatever runs, the forward has the bits of the unfused path (DD_WS_DW_OFF=1; the switch is read once per process: two
    child processes)."""
    sums, fused = [], []
    for off in ('0', '1'):
        env = dict(os.environ, DD_WS_DW_OFF=off)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'time_forward.py'), 'ssd', str(batch), 'kernels'],
                           capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        sums.append(re.search(r'sha (\S+)', r.stdout).group(1))
        fused.append('conv_ws_dw_k' in r.stdout)
    assert sums[0] == sums[1], sums
    assert fused[1] is False and (fused[0] or batch not in (256, 384)), (batch, fused)


def test_yolo_launch_of_256_frames_is_frame_independent_and_matches_the_oracle():
    """Config 3's launch shape (256 frames per detector launch: conv_ws_k on the 256/512-channel pointwise layers, the Focus
    slicing inside conv3x3_rw_k, the Detect heads reducing their rows): frames 0, 1, n/2, n-1 give the boxes / confidences /
    classes of their single-frame forwards bit for bit, and one of them those that tools/yolov5.py:121-128 computes from the
    f32 restatement's rows (boxes and confidence within test_gpu_nets.py's per-element tolerance; the class wherever the
    restatement's best two products are further apart than that tolerance)."""
    import torch
    from deepdish_amd import nets
    from deepdish_amd.engine import Net
    from deepdish_amd.profile import net_op_launches, OPK_NAMES
    from oracle import nets_torch
    n = 256
    wd = nets.synthetic_yolov5s_weights(1234)
    net = Net(nets.compile_yolov5s(wd), max_batch=n)
    net.yolo_decode(True)
    rng = np.random.default_rng(256)
    x = rng.integers(0, 256, (n, 640, 640, 3), dtype=np.uint8)
    x[1] = 0
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    net.forward(xd)
    ran = {OPK_NAMES.get(int(c)) for c in net_op_launches(net)}
    assert {'conv_ws_k', 'conv_glds_k<yolo_head_decode>'} <= ran, ran
    boxes, conf, cls = net.yolo_decoded()
    assert np.isfinite(boxes).all() and np.isfinite(conf).all()
    for i in (0, 1, n // 2, n - 1):
        net.forward(xd[i:i + 1])
        b1, c1, k1 = net.yolo_decoded()
        np.testing.assert_array_equal(b1[0], boxes[i], err_msg='frame %d boxes' % i)
        np.testing.assert_array_equal(c1[0], conf[i], err_msg='frame %d confidence' % i)
        np.testing.assert_array_equal(k1[0], cls[i], err_msg='frame %d class' % i)
    want = nets_torch.yolov5s_forward(wd, x[n - 1:n], w16=True)[0]
    assert _close(boxes[n - 1], want[:, :4], 2e-4, 1e-2) <= 1.0
    prod = want[:, 5:] * want[:, 4:5]
    order = np.sort(prod, axis=-1)
    assert _close(conf[n - 1], order[:, -1], 2e-4, 2e-2) <= 1.0
    # the class: on every row whose two best products are further apart than twice the stated tolerance of a product
    # (2e-4 + 2e-2 * value each), and those rows must be >= 90 % of the rows that pass the detector's 0.25 threshold (or of the 200 best)
    clear = (order[:, -1] - order[:, -2]) > 2 * (2e-4 + 2e-2 * order[:, -1])
    np.testing.assert_array_equal(cls[n - 1][clear], np.argmax(prod, axis=-1)[clear])
    # ... and on EVERY row, clear or not, the class picked must be one whose oracle product is within that margin of the oracle's best
    # (seeded random weights make near-ties common: 28 % of the 200 most confident rows here -- an exact-class demand on those rows
    # would test the tie, not the kernel)
    picked = prod[np.arange(len(prod)), cls[n - 1]]
    assert (picked >= order[:, -1] - 2 * (2e-4 + 2e-2 * order[:, -1])).all()
    top = np.argsort(-order[:, -1])[:200]
    print('rows with a clear best class: %.0f %% of all, %.0f %% of the 200 most confident' % (100 * clear.mean(), 100 * clear[top].mean()))


@pytest.mark.parametrize('n', [384, 768, 1536, 3072, 1533])
def test_lanczos_launch_of_384_frames_matches_pillow(n):
    """The detector pre-resize of a whole worker group (384 / 768 frames of 640x480 -> 300x300 in one launch of lanczos_fused_k: 15
    blocks per frame): four frames across the launch equal Pillow's bytes.

    1 536 / 3 072 frames: the headline's group and --groups 1.  The source is 921 600 bytes a frame, so its byte offsets pass 2^31 inside
    frame 2 330 (it starts at 2 330 x 921 600 = 2 147 328 000 and ends at 2 148 249 600; 2^31 = 2 147 483 648): at 3 072 frames
    2 329 (all below), 2 330 (across) and 2 331 (all above) are checked too.
    1 533 frames: 15 x 1 533 blocks is not a multiple of the eight XCDs, the branch of dd_xcd_remap (csrc/common.h) for an uneven
    grid, which 15 x 384 and 15 x 768 never take."""
    import torch
    from PIL import Image
    from deepdish_amd._lib import lib, check
    from deepdish_amd.runtime import default_context, ptr
    ctx = default_context()
    H, W, h, w = 480, 640, 300, 300
    g = torch.Generator(device='cuda'); g.manual_seed(384)
    src = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device='cuda', generator=g)
    dst = torch.empty((n, h, w, 3), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    check(lib().dd_resize_lanczos_batch(ctx.handle, ptr(src), n, H, W, 3, 1, ptr(dst), h, w, None))
    ctx.sync()
    picks = [0, 1, n // 2 - 1, n - 1] + [i for i in (2329, 2330, 2331) if i < n - 1]
    for i in picks:
        bgr = src[i].cpu().numpy()
        rgba = np.dstack([bgr[..., ::-1], np.full((H, W, 1), 255, np.uint8)])
        want = np.asarray(Image.fromarray(rgba, 'RGBA').convert('RGB').resize((w, h), Image.LANCZOS))
        np.testing.assert_array_equal(dst[i].cpu().numpy(), want, err_msg='frame %d' % i)
