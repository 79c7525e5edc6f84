"""GPU: the 128 x 64 and 256 x 128 MARS encoders (encoders/mars-128x64x3.pb, mars-256x128x3.pb upstream) -- the engine's one-launch front
(stem_conv_pool_wide_k: first layer + conv1_2 + max pool) against the three launches and the f32 restatement, and the batched pipeline at
all three crop sizes against the oracle chain and the single-stream plugin."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = 'stem_conv_pool_wide_k'
NEW_SIZES = [(128, 64), (256, 128)]


def _launches(net):
    from deepdish_amd.profile import net_op_launches, OPK_NAMES
    return {OPK_NAMES.get(int(c)) for c in net_op_launches(net)}


def _check_against_restatement(wd, x, got):
    from oracle import nets_torch
    want = nets_torch.mars_forward(wd, x, w16=True)
    err, cos = float(np.abs(got - want).max()), float((1.0 - np.sum(got * want, axis=1)).max())
    print('restatement: max abs %.3g, max cosine distance %.3g' % (err, cos))
    assert err < 5e-3                                            # the encoder's tolerance (tests/test_gpu_bench_size.py)
    assert cos < 5e-4


@pytest.mark.parametrize('hw,n', [((128, 64), 768), ((256, 128), 384)])
def test_wide_front_is_crop_independent_and_matches_the_restatement(hw, n, monkeypatch):
    """A batch above the fusion threshold (with DD_STEM_WIDE=1 the engine takes the one-launch front from 64 crops; by default it keeps the three
    launches, same bits): stem_conv_pool_wide_k ran, the pooled
    tensor and the features of crops 0, 1 (all zero), 2 (all 255), n/2 and n-1 are bit-identical to single-crop forwards (which run the three
    launches: stem_conv3_k, conv3x3_rw_k, maxpool_k), and eight crops agree with the f32 restatement within the encoder's tolerance."""
    from deepdish_amd import nets
    from deepdish_amd.engine import Net
    wd = nets.synthetic_mars_weights(1234, hw)
    prog = nets.compile_mars(wd, *hw)
    net = Net(prog, max_batch=n)
    rng = np.random.default_rng(n)
    x = rng.integers(0, 256, (n,) + hw + (3,), dtype=np.uint8)
    x[1] = 0; x[2] = 255
    monkeypatch.delenv('DD_STEM_WIDE', raising=False)
    net.forward(x)
    assert WIDE not in _launches(net), 'the default dispatch keeps the three launches until the kernel has been timed'
    by_default = net.read()[:, 0, 0, :].copy()
    monkeypatch.setenv('DD_STEM_WIDE', '1')                      # read on every forward
    net.forward(x)
    assert WIDE in _launches(net), _launches(net)
    np.testing.assert_array_equal(net.read()[:, 0, 0, :], by_default)
    full = net.read()[:, 0, 0, :].copy()
    pool_t = prog.meta['tensors']['pool1']
    pooled = net.read(tensor=pool_t).copy()
    with pytest.raises(Exception):                               # a tensor no launch wrote is not handed out
        net.read(tensor=prog.meta['tensors']['conv1_1'])
    np.testing.assert_allclose(np.linalg.norm(full.astype(np.float64), axis=1), 1.0, atol=1e-4)
    one = Net(nets.compile_mars(wd, *hw), max_batch=n)           # same engine size: same split-K decisions
    for i in (0, 1, 2, n // 2, n - 1):
        one.forward(x[i:i + 1])
        assert WIDE not in _launches(one)
        np.testing.assert_array_equal(one.read(tensor=pool_t)[0], pooled[i], err_msg='pooled tensor, crop %d' % i)
        np.testing.assert_array_equal(one.read()[0, 0, 0, :], full[i], err_msg='crop %d' % i)
    # an odd crop count (a workgroup of the 64-wide form holds two crops) and a count that splits each crop's rows over four workgroups
    for m in (65, 257):
        net.forward(x[:m])
        assert WIDE in _launches(net)
        np.testing.assert_array_equal(net.read(tensor=pool_t), pooled[:m], err_msg='%d crops' % m)
    del one, net
    eight = [0, 1, 2, 3, n // 2, n // 2 + 1, n - 2, n - 1]
    _check_against_restatement(wd, x[eight], full[eight])


def _child(size, n, env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'time_mars_sizes.py'), size, str(n), '--reps', '1', '--runs', '1',
                        '--warmup', '1'], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.splitlines()[0])


@pytest.mark.parametrize('size,n', [('128x64', 640), ('256x128', 320)])
def test_wide_front_switch_gives_the_same_bits(size, n):
    """DD_STEM_WIDE=1 / 0 in two child processes: the one-launch front / the three launches; the pooled tensor and the features have the
    same digest."""
    on, off = _child(size, n, {'DD_STEM_WIDE': '1'}), _child(size, n, {'DD_STEM_WIDE': '0'})
    assert WIDE in on['launches'] and WIDE not in off['launches'], (on['launches'], off['launches'])
    assert on['sha_pool'] == off['sha_pool']
    assert on['sha'] == off['sha']


@pytest.mark.parametrize('hw,n,gb', [((128, 64), 20480, 24.0), ((256, 128), 6144, 28.0)])
def test_one_large_launch_past_2_31_bytes_of_the_pooled_tensor(hw, n, gb, monkeypatch):
    """20 480 crops at 128 x 64 / 6 144 at 256 x 128 in one launch.  The pooled tensor is 63 x 31 x 32 f16 = 124 992 B a crop (2^31 bytes
    fall inside crop 17 180) / 127 x 63 x 32 f16 = 512 064 B a crop (inside crop 4 193): crops on both sides of the crossing, computed here
    from the tensor size, give the bits of their single-crop forwards on the same engine (three launches), and eight crops agree with the
    restatement.  The engine is built as the pipeline builds it (buffers overlaid by lifetime): its activation memory is printed and must
    stay under `gb` -- it takes 21.5 GB / 25.8 GB (the two full-resolution tensors of the three-launch path, 1 MiB / 4 MiB a crop, are the
    largest live pair: nets.MARS_ARENA_BYTES_PER_CROP)."""
    from deepdish_amd import nets
    from deepdish_amd.engine import Net
    wd = nets.synthetic_mars_weights(1234, hw)
    monkeypatch.setenv('DD_STEM_WIDE', '1')
    net = Net(nets.compile_mars(wd, *hw), max_batch=n, shared=True)
    act_gb = net.activation_bytes() / 1e9
    print('%d x %d, %d crops: engine activations %.1f GB' % (hw + (n, act_gb)))
    assert act_gb < gb
    per_crop = (hw[0] // 2 - 1) * (hw[1] // 2 - 1) * 32 * 2
    cross = (1 << 31) // per_crop                                # the crop that holds byte 2^31 of the pooled tensor
    assert 2 < cross < n - 2 and cross == {(128, 64): 17180, (256, 128): 4193}[hw]
    rng = np.random.default_rng(n)
    x = rng.integers(0, 256, (n,) + hw + (3,), dtype=np.uint8)
    x[1] = 0; x[2] = 255
    net.forward(x)
    assert WIDE in _launches(net), _launches(net)
    full = net.read()[:, 0, 0, :].copy()
    np.testing.assert_allclose(np.linalg.norm(full.astype(np.float64), axis=1), 1.0, atol=1e-4)
    for i in sorted({0, 1, 2, cross - 1, cross, cross + 1, n // 2, n - 1}):
        net.forward(x[i:i + 1])
        assert WIDE not in _launches(net)
        np.testing.assert_array_equal(net.read()[0, 0, 0, :], full[i], err_msg='crop %d' % i)
    del net
    eight = [0, 1, 2, cross - 1, cross, cross + 1, n // 2, n - 1]
    _check_against_restatement(wd, x[eight], full[eight])


@pytest.mark.parametrize('size', ['64x32x3', '128x64x3', '256x128x3'])
def test_multistream_pipeline_matches_oracle_per_stream_at_each_size(size):
    """tests/test_gpu_pipeline.py::test_multistream_pipeline_matches_oracle_per_stream with encoder_model='synthetic-mars-<size>': 3 streams
    batched in C++ == 3 independent oracle runs (NMS, crops of that size, f32 encoder, deep_sort, count line) -- track tables identical every
    frame, means within that test's tolerance, counts equal and non-zero.  Scenes and seeds are that test's: the oracle tracker's tables
    were checked on the CPU to be stable at all three sizes under feature noise of 1.6 x the encoder's tolerance."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    from oracle import deepsort_np as ds, countline_np as cl, image_np, nets_torch
    hw = tuple(int(v) for v in size.split('x')[:2])
    S, F = 3, 45
    scenes = [Scene(seed=21 + z, n_obj=10 + 3 * z, n_frames=F) for z in range(S)]
    mp = MultiStreamPipeline(S, run_detector=True, encoder_model='synthetic-mars-' + size)
    assert mp.enc_hw == hw
    otrk = [ds.Tracker(ds.Metric(0.2), max_iou_distance=0.7, max_age=60) for _ in range(S)]
    ocnt = [cl.CountLine(sc.countline()) for sc in scenes]
    for f in range(F):
        frames = np.stack([sc.frame(f) for sc in scenes])
        per = []
        for z, sc in enumerate(scenes):
            boxes, scores, _, _ = sc.detections(f)
            per.append(([tuple(int(v) for v in b) for b in boxes], ['person'] * len(boxes), [float(s) for s in scores]))
            keep = ds.non_max_suppression(boxes, 0.6, scores)
            patches = np.stack([image_np.extract_image_patch(frames[z], boxes[i], hw) for i in keep])
            feats = nets_torch.mars_forward(mp.enc_weights, patches)
            otrk[z].predict()
            otrk[z].update([ds.Det(boxes[i], 'person', scores[i], feats[j]) for j, i in enumerate(keep)])
            ocnt[z].step(otrk[z])
        mp.step(torch.from_numpy(frames).cuda(), mp.pack_injected(per))
        for z in range(S):
            ints, means = mp.tracker(z).table()
            want = np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in otrk[z].tracks],
                            dtype=np.int64).reshape(-1, 5)
            np.testing.assert_array_equal(ints[:, :5], want, err_msg=f'frame {f} stream {z}')
            if len(want):
                np.testing.assert_allclose(means, np.array([t.mean for t in otrk[z].tracks]), rtol=1e-6, atol=1e-6)
    got = mp.counts()
    for z in range(S):
        np.testing.assert_array_equal(got[z], ocnt[z].vector())
    assert got.sum() > 0
    assert mp.stage_ms()['steps'] == F


def test_multistream_pipeline_matches_plugin_on_a_128x64_frozen_graph(tmp_path):
    """MultiStreamPipeline given a mars-128x64x3.pb (written by graphdef.write_mars) takes 128 x 64 crops as ImageEncoder does
    (generate_detections.py:118-148): per stream the track tables of a HotPath on the same file, frame by frame, detector output and all."""
    from deepdish_amd import nets
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import HotPath, DEFAULT_LABELS
    from deepdish_amd.synth import Scene
    from deepdish_amd.tools import graphdef
    path = str(tmp_path / 'mars-128x64x3.pb')
    graphdef.write_mars(nets.synthetic_mars_weights(4321, (128, 64)), path, in_hw=(128, 64))
    wanted = sorted({l.strip() for l in open(DEFAULT_LABELS)} - {'???'})
    scenes = [Scene(seed=3, n_obj=8, n_frames=6), Scene(seed=5, n_obj=5, n_frames=6)]
    mp = MultiStreamPipeline(2, wanted_labels=wanted, encoder_model=path)
    assert mp.enc_hw == (128, 64)
    hps = [HotPath(wanted_labels=wanted, encoder_model=path) for _ in scenes]
    assert hps[0].encoder.image_encoder.image_shape == (128, 64, 3)
    seen = 0
    for f in range(6):
        fr = torch.from_numpy(np.stack([sc.frame(f) for sc in scenes])).cuda()
        mp.step(fr)
        for z, hp in enumerate(hps):
            hp.step(fr[z])
            ints, means = mp.tracker(z).table()
            want = np.array([[t.track_id, t.state, t.time_since_update, t.hits, t.age] for t in hp.tracker.tracks],
                            dtype=np.int64).reshape(-1, 5)
            np.testing.assert_array_equal(ints[:, :5], want, err_msg=f'frame {f} stream {z}')
            if len(want):
                np.testing.assert_allclose(means, np.array([t.mean for t in hp.tracker.tracks]), rtol=1e-9, atol=1e-9)
            seen = max(seen, len(want))
    assert seen > 0


def test_multistream_pipeline_takes_the_256x128_encoder_and_refuses_other_sizes(tmp_path):
    """The 256 x 128 encoder constructs and steps (from a synthetic name and from a frozen graph); the default crops-per-forward shrinks with
    the crop area; a size that is none of the reference's three is refused with a message that names them."""
    from deepdish_amd import nets
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.pipeline import HotPath
    from deepdish_amd.synth import Scene
    from deepdish_amd.tools import graphdef
    from deepdish_amd.pipeline import DEFAULT_LABELS
    # every label wanted, six frames: the seeded detector's classes are arbitrary (as in test_multistream_detector_output_matches_plugin)
    wanted = sorted({l.strip() for l in open(DEFAULT_LABELS)} - {'???'})
    sc = Scene(seed=3, n_obj=8, n_frames=6)
    path = str(tmp_path / 'mars-256x128x3.pb')
    graphdef.write_mars(nets.synthetic_mars_weights(4321, (256, 128)), path, in_hw=(256, 128))
    for name in ('synthetic-mars-256x128x3', path):
        mp = MultiStreamPipeline(2, wanted_labels=wanted, encoder_model=name)
        assert mp.enc_hw == (256, 128) and mp.enc.max_batch == 16
        for f in range(6):
            fr = torch.from_numpy(sc.frame(f)).cuda()
            mp.step(torch.stack([fr, fr]))
        a, b = mp.tracker(0).table(), mp.tracker(1).table()
        assert len(a[0]) > 0
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    hp = HotPath(encoder_model='synthetic-mars-256x128x3')
    assert hp.encoder.image_encoder.image_shape == (256, 128, 3)
    hp.step(torch.from_numpy(sc.frame(0)).cuda())
    mp = MultiStreamPipeline(64, encoder_model='synthetic-mars-128x64x3', run_detector=False)      # 2 048 crops at 64 x 32: 451 MB of activations
    assert mp.enc.max_batch == 430 and mp.enc.activation_bytes() <= 2048 * nets.MARS_ARENA_BYTES_PER_CROP[(64, 32)] + 65536
    assert abs(mp.enc.activation_bytes() / 430 / nets.MARS_ARENA_BYTES_PER_CROP[(128, 64)] - 1.0) < 0.01
    odd = str(tmp_path / 'mars-96x48x3.pb')
    graphdef.write_mars(nets.synthetic_mars_weights(4321, (96, 48)), odd, in_hw=(96, 48))
    with pytest.raises(ValueError, match=r'64 x 32, 128 x 64 and 256 x 128'):
        MultiStreamPipeline(1, encoder_model=odd)


@pytest.mark.parametrize('hw', [(64, 32), (128, 64), (256, 128)])
def test_arena_bytes_per_crop_table_matches_the_engine(hw):
    """nets.MARS_ARENA_BYTES_PER_CROP sizes the pipeline's default crops per forward: each entry is what an engine with overlaid buffers
    (dd_net_create_shared) takes per crop (the buffers' 256-byte paddings aside)."""
    from deepdish_amd import nets
    from deepdish_amd.engine import Net
    n = 256
    net = Net(nets.compile_mars(nets.synthetic_mars_weights(1234, hw), *hw), max_batch=n, shared=True)
    per_crop = net.activation_bytes() / n
    print('%d x %d: %.0f B per crop' % (hw + (per_crop,)))
    assert 0 <= per_crop - nets.MARS_ARENA_BYTES_PER_CROP[hw] < 64


def test_multistream_pipeline_runs_the_wide_front_from_64_crops_per_forward(monkeypatch):
    """Six streams of 20 objects at 128 x 64 with 256 crops per encoder forward: the step's kept boxes (more than 64) go through the encoder in
    one forward, which takes the one-launch front under DD_STEM_WIDE=1 and the three launches under DD_STEM_WIDE=0 (the switch is read on
    every forward).  Two pipelines of the same engine size, one stepped under each: track tables and means are equal bit for bit at every frame."""
    from deepdish_amd.multipipe import MultiStreamPipeline
    from deepdish_amd.synth import Scene
    S, F = 6, 8
    scenes = [Scene(seed=31 + z, n_obj=20, n_frames=F, churn=False) for z in range(S)]      # 120 objects in every frame
    wide, three = (MultiStreamPipeline(S, run_detector=False, encoder_model='synthetic-mars-128x64x3', encoder_max_batch=256) for _ in range(2))
    for f in range(F):
        frames = torch.from_numpy(np.stack([sc.frame(f) for sc in scenes])).cuda()
        per = []
        for sc in scenes:
            boxes, scores, _, _ = sc.detections(f)
            per.append(([tuple(int(v) for v in b) for b in boxes], ['person'] * len(boxes), [float(v) for v in scores]))
        monkeypatch.setenv('DD_STEM_WIDE', '1')
        wide.step(frames, wide.pack_injected(per))
        assert WIDE in _launches(wide.enc), (f, _launches(wide.enc))
        monkeypatch.setenv('DD_STEM_WIDE', '0')
        three.step(frames, three.pack_injected(per))
        assert WIDE not in _launches(three.enc)
        for z in range(S):
            a, b = wide.tracker(z).table(), three.tracker(z).table()
            np.testing.assert_array_equal(a[0], b[0], err_msg=f'frame {f} stream {z}')
            np.testing.assert_array_equal(a[1], b[1], err_msg=f'frame {f} stream {z}')
    assert sum(len(wide.tracker(z).table()[0]) for z in range(S)) > 0
