"""CPU, through ctypes: dd_ground_camera and the host path of dd_ground_from_image (csrc/ground.hip, csrc/ground_dev.h) against
tests/topdown_ref.py -- bit for bit: the ref performs the header's IEEE operations in the header's order, and the header is compiled
with floating-point contraction off."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import topdown_ref  # noqa: E402

CAMERAS = [dict(f_mm=3.6, sensor_mm=(6.17, 4.55), image=(640, 480), elevation_m=4.0, tilt_deg=60.0, roll_deg=0.0),
           dict(f_mm=3.6, sensor_mm=(6.17, 4.55), image=(640, 480), elevation_m=2.5, tilt_deg=30.0, roll_deg=10.0),
           dict(f_mm=2.8, sensor_mm=(5.37, 4.04), image=(1280, 720), elevation_m=7.25, tilt_deg=85.0, roll_deg=-10.0),
           dict(f_mm=8.0, sensor_mm=(7.2, 5.4), image=(640, 480), elevation_m=12.0, tilt_deg=0.0, roll_deg=3.5),
           dict(f_mm=4.2, sensor_mm=(6.17, 4.55), image=(642, 482), elevation_m=3.0, tilt_deg=45.0, roll_deg=-1.0)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _camera(**k):
    from deepdish_amd._lib import lib
    out = np.full(9, -77.0)
    rc = lib().dd_ground_camera(k['f_mm'], k['sensor_mm'][0], k['sensor_mm'][1], k['image'][0], k['image'][1], k['elevation_m'], k['tilt_deg'],
                                k.get('roll_deg', 0.0), out.ctypes.data)
    return rc, out


def _from_image(cams, points, idx=None, n=None, out=None):
    from deepdish_amd._lib import lib
    cams = np.ascontiguousarray(cams, dtype=np.float64).reshape(-1, 9)
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    out = np.full_like(points, -77.0) if out is None else out
    idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    rc = lib().dd_ground_from_image(None, cams.ctypes.data, len(cams), None if idx is None else idx.ctypes.data, points.ctypes.data,
                                    len(points) if n is None else n, out.ctypes.data, 0, None)
    return rc, out


def test_camera_equals_the_ref():
    """The five exact fields are equal; the four trigonometric ones come from the same C library (math.cos is libm's cos), so they are
    compared exactly too -- and to 1 ulp should a platform's Python not call the library the host code links."""
    for k in CAMERAS:
        rc, got = _camera(**k)
        assert rc == 0
        want = topdown_ref.camera(**k)
        np.testing.assert_array_equal(got[:5], want[:5])
        np.testing.assert_allclose(got[5:], want[5:], rtol=0, atol=2.0 ** -52)
    assert _camera(**CAMERAS[0])[1][0] == 3.6 / 6.17 * 640 and _camera(**CAMERAS[0])[1][3] == 240.0


@pytest.mark.parametrize('field,value', [('f_mm', 0.0), ('f_mm', -1.0), ('f_mm', float('nan')), ('sensor_mm', (0.0, 4.55)), ('sensor_mm', (6.17, -4.55)),
                                         ('sensor_mm', (float('inf'), 4.55)), ('image', (0, 480)), ('image', (640, -1)), ('elevation_m', 0.0),
                                         ('elevation_m', -3.0), ('elevation_m', float('nan')), ('tilt_deg', float('inf')), ('roll_deg', float('nan'))])
def test_camera_refusals(field, value):
    from deepdish_amd._lib import lib
    k = dict(CAMERAS[0])
    k[field] = value
    rc, out = _camera(**k)
    assert rc < 0 and b'dd_ground_camera' in lib().dd_last_error()
    assert (out == -77.0).all()                                     # nothing written


def test_python_class_refuses_too():
    from deepdish_amd._lib import DeepDishHipError
    from deepdish_amd.ground import GroundPlane
    with pytest.raises(DeepDishHipError, match='dd_ground_camera'):
        GroundPlane(3.6, sensor_mm=(6.17, 4.55), image=(640, 480), elevation_m=-1.0, tilt_deg=60.0)
    with pytest.raises(ValueError, match='image sizes'):
        GroundPlane.stack([GroundPlane(3.6, (6.17, 4.55), (640, 480), 4.0, 60.0), GroundPlane(3.6, (6.17, 4.55), (1280, 720), 4.0, 60.0)])


def _points(rng, n):
    """Pixels over and around a 1280 x 720 image: most on it, some far off, fractional."""
    p = rng.uniform(-200.0, 1500.0, (n, 2))
    p[::7] = np.round(p[::7])
    return p


def test_host_path_equals_the_ref_bit_for_bit():
    rng = np.random.default_rng(20260117)
    cams = np.stack([topdown_ref.camera(**k) for k in CAMERAS])
    pts = _points(rng, 4096)
    idx = rng.integers(0, len(cams), 4096).astype(np.int32)
    rc, got = _from_image(cams, pts, idx)
    assert rc == 0
    want = topdown_ref.space_from_image(cams, pts, idx)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    nan = np.isnan(want[:, 0])
    assert 0.05 < nan.mean() < 0.95 and (np.isnan(want[:, 1]) == nan).all()      # both sides of the horizon are in the set
    # camera 0 without an index array; the Python class over the library's own cameras
    rc, got0 = _from_image(cams, pts)
    np.testing.assert_array_equal(_bits(got0), _bits(topdown_ref.space_from_image(cams, pts)))
    from deepdish_amd.ground import GroundPlane
    table = GroundPlane.stack([GroundPlane(k['f_mm'], k['sensor_mm'], k['image'], k['elevation_m'], k['tilt_deg'], k['roll_deg'])
                               for k in CAMERAS if k['image'] == (640, 480)])
    sub = [i for i, k in enumerate(CAMERAS) if k['image'] == (640, 480)]
    assert len(table) == 3
    idx3 = rng.integers(0, 3, 4096)
    got3 = table.space_from_image(pts, idx3)
    assert isinstance(got3, np.ndarray)
    np.testing.assert_array_equal(_bits(got3), _bits(topdown_ref.space_from_image(table.table, pts, idx3)))
    np.testing.assert_allclose(table.table, cams[sub], rtol=0, atol=2.0 ** -52)


def test_nan_at_and_above_the_horizon_and_for_non_finite_input():
    cam = topdown_ref.camera(3.6, (6.17, 4.55), (640, 480), 4.0, 60.0)
    fy, cy = cam[1], cam[3]
    horizon = cy - fy * np.tan(np.radians(30.0))
    pts = np.array([[320.0, horizon + 40.0], [320.0, horizon - 1.0], [5.0, 0.0], [320.0, np.nan], [np.inf, 400.0], [-np.inf, np.nan], [100.0, 479.0]])
    rc, got = _from_image(cam, pts)
    assert rc == 0
    assert np.isfinite(got[0]).all() and np.isfinite(got[6]).all()
    assert np.isnan(got[1:6]).all()
    assert (_bits(got[1:6]) == 0x7ff8000000000000).all()            # one fixed quiet NaN, whatever produced it
    np.testing.assert_array_equal(_bits(got), _bits(topdown_ref.space_from_image(cam, pts)))
    # den == 0 exactly: tilt 0 never gets there, a camera made by hand does (cos t = 0, sin t = 1, b' = 0)
    flat = cam.copy()
    flat[5], flat[6] = 0.0, 1.0
    rc, got = _from_image(flat, [[320.0, 240.0], [320.0, 300.0]])
    assert np.isnan(got[0]).all() and np.isfinite(got[1]).all()


def test_bad_camera_index_is_refused_and_nothing_is_written():
    from deepdish_amd._lib import lib
    cams = np.stack([topdown_ref.camera(**k) for k in CAMERAS])
    pts = _points(np.random.default_rng(3), 16)
    for bad in (5, -1, 2 ** 31 - 1):
        idx = np.zeros(16, dtype=np.int32)
        idx[11] = bad
        rc, out = _from_image(cams, pts, idx)
        assert rc < 0 and b'dd_ground_from_image' in lib().dd_last_error()
        assert (out == -77.0).all()
    from deepdish_amd._lib import DeepDishHipError
    from deepdish_amd.ground import GroundPlane
    with pytest.raises(DeepDishHipError, match='camera 1 of 1'):
        GroundPlane(3.6, (6.17, 4.55), (640, 480), 4.0, 60.0).space_from_image(pts, np.ones(16, np.int32))


def test_no_points_is_a_no_op():
    from deepdish_amd._lib import lib
    cam = topdown_ref.camera(**CAMERAS[0])
    out = np.full((4, 2), -77.0)
    rc, out = _from_image(cam, np.zeros((4, 2)), n=0, out=out)
    assert rc == 0 and (out == -77.0).all()
    assert lib().dd_ground_from_image(None, None, 1, None, None, 0, None, 0, None) == 0
    from deepdish_amd.ground import GroundPlane
    assert GroundPlane(3.6, (6.17, 4.55), (640, 480), 4.0, 60.0).space_from_image(np.zeros((0, 2))).shape == (0, 2)
    # the output may not be the input, and device arrays need a context
    p = np.zeros((4, 2))
    assert lib().dd_ground_from_image(None, cam.ctypes.data, 1, None, p.ctypes.data, 4, p.ctypes.data, 0, None) < 0
    assert lib().dd_ground_from_image(None, cam.ctypes.data, 1, None, p.ctypes.data, 4, out.ctypes.data, 1, None) < 0
