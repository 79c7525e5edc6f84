"""Ground-plane unprojection (csrc/ground.hip, csrc/ground_dev.h): the camera of the reference's --3d mode (deepdish.py:592-611) and its
cam.spaceFromImage (:1088-1097), image pixels -> metres on the ground.

    cam = GroundPlane(3.6, sensor_mm=(6.17, 4.55), image=(640, 480), elevation_m=4.0, tilt_deg=60.0)
    xy = cam.space_from_image([[320, 400], [100, 300]])            # f64 [2, 2]; NaN where the pixel lies at or above the horizon
    table = GroundPlane.stack([cam_a, cam_b, cam_c])                # one camera per stream
    xy = table.space_from_image(points_dev, cam_index_dev)          # device tensors in, a device tensor out: one launch

The reference takes this geometry from the `cameratransform` package; here it is restated from the package's published definition
(rectilinear projection, heading 0, camera at (0, 0, elevation), tilt 0 = straight down) and held to tests/topdown_ref.py.  Parity with
the package itself is not pinned."""
import numpy as np

from ._lib import lib, check, P

CAMERA_DOUBLES = 9         # fx, fy, cx, cy, elevation, cos tilt, sin tilt, cos roll, sin roll


class GroundPlane:
    def __init__(self, focallength_mm, sensor_mm, image, elevation_m, tilt_deg, roll_deg=0.0, context=None):
        sw, sh = sensor_mm
        W, H = image
        if int(W) != W or int(H) != H:
            raise ValueError('image size %r: whole pixels' % (image,))
        self.image = (int(W), int(H))
        self.table = np.zeros((1, CAMERA_DOUBLES), dtype=np.float64)
        check(lib().dd_ground_camera(float(focallength_mm), float(sw), float(sh), int(W), int(H), float(elevation_m), float(tilt_deg),
                                     float(roll_deg), P(self.table.ctypes.data)), 'dd_ground_camera')
        self.ctx = context
        self._table_dev = None

    @classmethod
    def stack(cls, cameras, context=None):
        """The camera table of several streams: camera i is cameras[i].  All must share one image size."""
        cameras = list(cameras)
        if not cameras:
            raise ValueError('no camera to stack')
        images = {c.image for c in cameras}
        if len(images) != 1:
            raise ValueError('cameras of different image sizes in one table: %s' % sorted(images))
        out = cls.__new__(cls)
        out.image = cameras[0].image
        out.table = np.ascontiguousarray(np.concatenate([c.table for c in cameras], axis=0))
        out.ctx = context or cameras[0].ctx
        out._table_dev = None
        return out

    def __len__(self):
        return len(self.table)

    def _context(self):
        if self.ctx is None:
            from .runtime import default_context
            self.ctx = default_context()
        return self.ctx

    def space_from_image(self, points, cam_index=None):
        """points [n, 2] (u, v) in pixels, cam_index int32 [n] into the table (default: camera 0) -> [n, 2] (X, Y) in metres, of the kind
        given: a numpy array is computed on the host, a device tensor by one launch queued on the context's stream (the tensors must
        be complete by then: ctx.to_device waits).  Host and device agree bit for bit.  On the host an index outside the table raises;
        on the device such a point yields NaN."""
        if hasattr(points, 'data_ptr'):
            import torch
            assert points.dtype == torch.float64 and points.dim() == 2 and points.shape[1] == 2 and points.is_contiguous() and points.is_cuda
            n = int(points.shape[0])
            if cam_index is not None:
                assert cam_index.dtype == torch.int32 and tuple(cam_index.shape) == (n,) and cam_index.is_contiguous() and cam_index.is_cuda
            ctx = self._context()
            if self._table_dev is None:
                self._table_dev = ctx.to_device(self.table)
            out = torch.empty_like(points)
            check(lib().dd_ground_from_image(ctx.handle, P(self._table_dev.data_ptr()), len(self.table), P(cam_index.data_ptr()) if cam_index is not None else P(None),
                                             P(points.data_ptr()), n, P(out.data_ptr()), 1, None), 'dd_ground_from_image')
            return out
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
        idx = None if cam_index is None else np.ascontiguousarray(cam_index, dtype=np.int32).reshape(-1)
        if idx is not None and len(idx) != len(pts):
            raise ValueError('%d camera indices for %d points' % (len(idx), len(pts)))
        out = np.empty_like(pts)
        check(lib().dd_ground_from_image(None, P(self.table.ctypes.data), len(self.table), P(idx.ctypes.data) if idx is not None else P(None),
                                         P(pts.ctypes.data), len(pts), P(out.ctypes.data), 0, None), 'dd_ground_from_image')
        return out


def for_pipeline(ground, topdownview_size_m, input_size, n_streams):
    """What the pipelines' constructors make of `ground` and `topdownview_size_m` -> (camera table or None, scale f64 [2] or None).
    ground: None, a GroundPlane (one camera for every stream, or a table with one per stream) or a list with one per stream.
    deepdish.py:601-609: the panel is (W / 4, H / 4) pixels; --topdownview-size-m X,Y (through int(), as upstream) makes it X x Y metres."""
    if ground is None:
        if topdownview_size_m is not None:
            raise ValueError('topdownview_size_m without ground: the top-down view needs a camera')
        return None, None
    if isinstance(ground, (list, tuple)):
        if len(ground) != n_streams:
            raise ValueError('%d cameras for %d streams' % (len(ground), n_streams))
        ground = GroundPlane.stack(ground)
    if len(ground) not in (1, n_streams):
        raise ValueError('%d cameras for %d streams' % (len(ground), n_streams))
    W, H = (int(v) for v in input_size)
    if ground.image != (W, H):
        raise ValueError('the camera is calibrated for %d x %d images, the pipeline runs on %d x %d' % (ground.image + (W, H)))
    scale = np.array([1.0, 1.0])
    if topdownview_size_m is not None:
        X, Y = (int(v) for v in topdownview_size_m)
        if X <= 0 or Y <= 0:
            raise ValueError('topdownview_size_m %r: whole positive metres' % (topdownview_size_m,))
        scale = np.array([W / 4, H / 4], dtype=np.float64) / np.array([X, Y], dtype=np.float64)
    return ground, scale
