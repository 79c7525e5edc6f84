"""Baseline JPEG files from BGR frames in HBM (csrc/jpeg.hip): the exit of the render path.

The reference hands its annotated output frame to cv2.imencode(".jpg", frame) for the MJPEG web stream (deepdish.py:155-181), to
frame_%06d.jpg under --output-cvat-dir (:764-766) and to the file --stream-path names.  Here the frame is encoded where it was painted:

    enc = JpegEncoder(480, 640)                          # quality 95 (cv2's default), one restart interval per MCU row
    files = enc.encode_to_host(frames_dev)               # u8 [n, 480, 640, 3] BGR on the device -> list of n bytes objects
    part = wire.mjpeg_part(files[0])                     # what deepdish.py:178-179 yields

The bytes are libjpeg's for 8-bit YCbCr 4:2:0 with the ITU-T T.81 Annex K tables: Pillow's
Image.save(f, 'JPEG', quality=q, subsampling='4:2:0', restart_marker_rows=r) byte for byte, header included (tests/test_jpeg_ref.py,
tests/test_gpu_jpeg.py).  The one deviation from cv2.imencode is the DRI segment and the RSTn markers, which cv2 does not write and every
decoder honours: a restart interval is the unit of parallel work.  Parity with OpenCV's own bytes is not pinned."""
import ctypes

import numpy as np

from ._lib import lib, check, P, DeepDishHipError

PATH_LDS, PATH_STREAM = 0, 1
E_CAPACITY = -4


def plan(H, W, restart_rows=1):
    """Which kernel path a geometry takes (PATH_LDS: the interval stays in LDS; PATH_STREAM: too large for that).  Needs no device."""
    path = ctypes.c_int(-1)
    check(lib().dd_jpeg_plan(int(H), int(W), int(restart_rows), ctypes.byref(path)), 'dd_jpeg_plan')
    return path.value


def _header(handle):
    n = ctypes.c_int()
    check(lib().dd_jpeg_header(handle, None, 0, ctypes.byref(n)), 'dd_jpeg_header')
    buf = (ctypes.c_uint8 * n.value)()
    check(lib().dd_jpeg_header(handle, buf, n.value, ctypes.byref(n)), 'dd_jpeg_header')
    return bytes(buf)


def header(H, W, quality=95, restart_rows=1):
    """SOI .. the SOS segment of every file such an encoder writes.  Needs no device."""
    h = P()
    check(lib().dd_jpeg_create(None, int(H), int(W), int(quality), int(restart_rows), ctypes.byref(h)), 'dd_jpeg_create')
    try:
        return _header(h)
    finally:
        lib().dd_jpeg_destroy(h)


class JpegEncoder:
    """One frame size, quality and restart interval."""

    def __init__(self, H, W, quality=95, restart_rows=1, context=None):
        from .runtime import default_context
        self.ctx = context or default_context()
        self.H, self.W, self.quality, self.restart_rows = int(H), int(W), int(quality), int(restart_rows)
        h = P()
        check(lib().dd_jpeg_create(self.ctx.handle, self.H, self.W, self.quality, self.restart_rows, ctypes.byref(h)), 'dd_jpeg_create')
        self._h = h
        self.path = plan(self.H, self.W, self.restart_rows)
        self.header = _header(h)
        self.default_capacity = self.H * self.W * 3 + 1024

    def __del__(self):
        try:
            if self._h:
                lib().dd_jpeg_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _encode(self, frames_dev, out, capacity):
        import torch
        if frames_dev.dim() == 3:
            frames_dev = frames_dev[None]
        assert tuple(frames_dev.shape[1:]) == (self.H, self.W, 3) and frames_dev.dtype == torch.uint8 and frames_dev.is_contiguous()
        n = int(frames_dev.shape[0])
        if out is None:
            out = torch.empty((n, int(capacity if capacity is not None else self.default_capacity)), dtype=torch.uint8, device=frames_dev.device)
        assert out.dim() == 2 and out.shape[0] == n and out.dtype == torch.uint8 and out.is_contiguous()
        lengths = torch.empty(n, dtype=torch.int32, device=frames_dev.device)
        torch.cuda.current_stream(frames_dev.device).synchronize()          # frames made by torch ops; the launches go to the context's stream
        rc = lib().dd_jpeg_encode(self._h, P(frames_dev.data_ptr()), n, P(out.data_ptr()), int(out.shape[1]), P(lengths.data_ptr()), None)
        return rc, out, lengths

    def encode(self, frames_dev, out=None, capacity=None):
        """frames_dev: u8 [n, H, W, 3] (or [H, W, 3]) BGR torch tensor in HBM -> (bytes u8 [n, capacity], lengths int32 [n]), both on the
        device: file i is bytes[i, :lengths[i]].  capacity defaults to H * W * 3 + 1024 (out: a tensor to write instead of a new one).
        Queued on the context's stream and complete on return.  A file longer than the capacity raises (its length is in the message)."""
        rc, out, lengths = self._encode(frames_dev, out, capacity)
        check(rc, 'dd_jpeg_encode')
        return out, lengths

    def encode_to_host(self, frames_dev):
        """-> list of n bytes objects: one device-to-host copy of the lengths and one of the bytes in use.  Frames that overflow the
        default capacity are encoded once more with the length the first call reported."""
        import torch
        if frames_dev.dim() == 3:
            frames_dev = frames_dev[None]
        rc, out, lengths = self._encode(frames_dev, None, None)
        if rc not in (0, E_CAPACITY):
            check(rc, 'dd_jpeg_encode')
        lens = lengths.cpu().numpy().astype(np.int64)
        cap = int(out.shape[1])
        over = [i for i in range(len(lens)) if lens[i] > cap]
        pieces = [out[i, :int(lens[i])] if lens[i] <= cap else None for i in range(len(lens))]
        if over:
            retry, _ = self.encode(frames_dev[over].contiguous(), capacity=int(lens[over].max()))
            for k, i in enumerate(over):
                pieces[i] = retry[k, :int(lens[i])]
        flat = torch.cat(pieces).cpu().numpy().tobytes()
        ends = np.cumsum(lens)
        return [flat[int(e - l):int(e)] for e, l in zip(ends, lens)]
