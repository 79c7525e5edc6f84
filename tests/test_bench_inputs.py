"""CPU: bench.py paints its frames on the device from each scene's seeded draws (_scene_spec + render_frames) instead of shipping
rendered frames from its generator processes; the frames and the injected detections must be exactly what synth.Scene gives
(the same computation run on torch's CPU backend here), streams split over worker groups in uneven chunks included."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402
from deepdish_amd.synth import Scene  # noqa: E402


def _scene(seed, n_frames, W, H):
    sc = Scene(seed=seed, n_obj=bench.N_OBJ, width=W, height=H, n_frames=n_frames)
    per = []
    for f in range(n_frames):
        boxes, scores, _, _ = sc.detections(f)
        per.append(([tuple(int(v) for v in b) for b in boxes], ['person'] * len(boxes), [float(x) for x in scores]))
    return np.stack([sc.frame(f) for f in range(n_frames)]), per


@pytest.mark.parametrize('W,H,n_frames,seeds', [(640, 480, 25, (0, 1000, 3071)), (640, 640, 6, (5,)), (1280, 720, 3, (0,))])
def test_rendered_frames_are_scene_frames(W, H, n_frames, seeds):
    out = [bench._scene_spec((s, n_frames, W, H)) for s in seeds]
    frames = bench.render_frames([o[0] for o in out], W, H, 'cpu').numpy()
    for c, s in enumerate(seeds):
        want, per = _scene(s, n_frames, W, H)
        assert out[c][1] == per
        np.testing.assert_array_equal(frames[:, c], want)


def test_streams_land_in_their_groups_slots(monkeypatch):
    monkeypatch.setattr(bench, 'RENDER_CHUNK', 3)
    S, F, W, H, bounds = 11, 3, 640, 480, [0, 5, 11]
    dev = [torch.zeros((F, bounds[g + 1] - bounds[g], H, W, 3), dtype=torch.uint8) for g in range(2)]
    dets = bench.make_inputs_rendered(None, 0, S, F, W, H, dev, bounds, 'cpu')
    for s in range(S):
        g = 0 if s < bounds[1] else 1
        want, per = _scene(s, F, W, H)
        assert dets[s] == per
        np.testing.assert_array_equal(dev[g][:, s - bounds[g]].numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize('W,H,n_frames,seeds', [(640, 480, 6, (0, 1000, 3071)), (640, 640, 4, (5,)), (1280, 720, 3, (0, 2))])
def test_rendered_frames_on_the_device_are_scene_frames(W, H, n_frames, seeds):
    """bench.py paints on 'cuda' (render_frames' float64 background stretch and the pasted rectangles on the GPU): the same
    bytes as synth.Scene.frame, as the CPU-backend test above holds for torch's CPU kernels."""
    out = [bench._scene_spec((s, n_frames, W, H)) for s in seeds]
    frames = bench.render_frames([o[0] for o in out], W, H, 'cuda').cpu().numpy()
    for c, s in enumerate(seeds):
        want, per = _scene(s, n_frames, W, H)
        assert out[c][1] == per
        np.testing.assert_array_equal(frames[:, c], want, err_msg='%dx%d seed %d' % (W, H, s))
