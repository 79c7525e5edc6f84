"""Frame ingest ring (csrc/ingest.hip): the GPU side of Pipeline.capture (deepdish.py:837-878 upstream).

A decoder thread writes raw BGR frames of S streams into a pinned slot (`host(slot)` is a numpy view of
it), `submit(slot)` queues upload + cv2.flip(frame, 0) + cv2.resize(frame, input_size) on a private copy
stream, and `acquire(slot)` hands the device frames to the hot path once its stream has been told to wait
for them -- the host never blocks on a copy.

With `pixel_format='nv12'` or `'i420'` a slot holds what a decoder produces itself (4:2:0 YUV, 1.5 bytes per pixel): half the bytes
cross the host link, and the conversion to BGR (csrc/yuv.hip, OpenCV's BT.601 fixed-point arithmetic restated) runs on the copy
stream in front of the flip + resize.  `yuv420_to_bgr` is the same conversion for frames that are already in device memory.

With `pixel_format='yuy2'` or `'uyvy'` a slot holds packed 4:2:2, what a UVC / V4L2 camera (YUY2: Y0 U Y1 V) or an SDI / HDMI capture card
(UYVY: U Y0 V Y1) delivers raw: 2 bytes per pixel, two thirds of BGR, converted with the same arithmetic (cv2.cvtColor COLOR_YUV2BGR_YUY2 /
_UYVY restated; tests/yuv422_ref.py is the definition, parity with OpenCV itself is unpinned).  `yuv422_to_bgr` is that conversion for
frames already in device memory.

With `pixel_format='bayer_rggb'`, `'bayer_grbg'`, `'bayer_gbrg'` or `'bayer_bggr'` a slot holds the 8-bit Bayer mosaic a machine-vision (GigE / USB3
Vision BayerRG8 and its siblings) or CSI camera delivers before any colour processing, named by the sensor's top-left 2 x 2 block read row
by row; with `'gray'` 8-bit monochrome (GREY / Y800, infrared cameras).  One byte per pixel, a third of BGR.  The mosaic is demosaiced on the
copy stream by OpenCV's published bilinear rule restated (csrc/bayer.hip; cv2.cvtColor COLOR_BayerBG2BGR for RGGB, _BayerGB2BGR for GRBG,
_BayerGR2BGR for GBRG, _BayerRG2BGR for BGGR -- OpenCV names the block at (1, 1); tests/bayer_ref.py is the definition, parity with OpenCV
itself is unpinned), in one launch with the flip + resize.  `raw8_to_bgr` is that conversion for frames already in device memory.  Not
built: 10 / 12 / 16-bit and packed RAW10 mosaics; white balance, gamma or colour matrices (a camera that sends 8-bit Bayer has applied its
own before the mosaic leaves it); edge-aware / VNG demosaicing.

With `pixel_format='jpeg'` a slot holds baseline JPEG files, what an IP camera's MJPEG stream or the reference's frame_%06d.jpg sequence
(--input-cvat-dir) delivers -- a tenth or less of the raw bytes: `put(slot, stream, file)` copies a file into the slot's pinned arena and
parses its header on the calling thread, `submit(slot)` uploads the bytes in use and decodes on the copy stream (csrc/jpeg_dec.hip,
libjpeg's arithmetic restated), and `status(slot)` tells per stream whether its frame is good (deepdish_amd.jpeg.ST_*).  `jpeg_scale=2`, 4, 8
or 'auto' decodes at that fraction (libjpeg's scale_denom, deepdish_amd.jpeg.JpegDecoder(scale=...)) in front of the resize: megapixel
cameras feeding a 640 x 480 pipeline never have their full-size frames written.  `jpeg_any_size=True` makes src_size the largest file
accepted, not the only one: cameras of every mode share one ring, each file stretched to dst_size as the reference's
cv2.resize(frame, self.input_size) does (deepdish.py:867), and `source_sizes(slot)` says what each stream sent."""
import ctypes
import numpy as np

from ._lib import lib, check, P
from .runtime import default_context, ptr

PIXEL_FORMATS = {'bgr': 0, 'nv12': 1, 'i420': 2, 'jpeg': 3, 'yuy2': 4, 'uyvy': 5, 'bayer_rggb': 6, 'bayer_grbg': 7, 'bayer_gbrg': 8, 'bayer_bggr': 9,
                 'gray': 10}
PACKED_422 = ('yuy2', 'uyvy')
BAYER = ('bayer_rggb', 'bayer_grbg', 'bayer_gbrg', 'bayer_bggr')
RAW8 = BAYER + ('gray',)


class FrameIngest:
    def __init__(self, n_streams, src_size, dst_size=None, slots=2, flip=False, context=None, pixel_format='bgr', jpeg_slot_bytes=None, jpeg_scale=1, jpeg_progressive=False,
                 jpeg_split=False, jpeg_any_size=False, jpeg_std_tables=False):
        """src_size / dst_size: (width, height) like the reference's `input_size`; dst defaults to src.
        pixel_format: what a slot holds, 'bgr' | 'nv12' | 'i420' (4:2:0 needs an even width and height) | 'yuy2' | 'uyvy' (packed 4:2:2,
        named by FOURCC: an even width, any height) | 'bayer_rggb' | 'bayer_grbg' | 'bayer_gbrg' | 'bayer_bggr' (an 8-bit mosaic named by its top-left
        2 x 2 block: both sides at least 3, either may be odd) | 'gray' (8-bit monochrome, any size) | 'jpeg'; the consumer always gets BGR.  jpeg_slot_bytes: the size of a JPEG slot's arena, by default n_streams * width * height * 3 // 8.
        jpeg_scale ('jpeg' only; anything but 1 with another format is a ValueError): 1, 2, 4, 8 or 'auto' = deepdish_amd.jpeg.draft_scale(src_size,
        dst_size), Pillow's draft rule.  src_size stays what every file must state; the ring decodes ceil(height / scale) x ceil(width / scale)
        frames and resizes from there -- or decodes straight into the slot when that is dst_size and no flip is asked.
        jpeg_progressive ('jpeg' only): take progressive (SOF2) files as well as baseline ones, at any jpeg_scale
        (deepdish_amd.jpeg.JpegDecoder(progressive=True)); without it such a file is ST_HEADER, as ever.
        jpeg_split ('jpeg' only): files without restart markers are decoded by a workgroup each, not by one lane
        (deepdish_amd.jpeg.JpegDecoder(split=True)); the frames are the same.
        jpeg_any_size ('jpeg' only, a ValueError otherwise): src_size is the largest file accepted.  A file with 1 <= height <= src height and
        1 <= width <= src width is ST_OK and is stretched to dst_size (a file of exactly twice dst_size takes the 2 x INTER_AREA shortcut); one
        with either side larger is ST_SIZE and absent.  A camera may change its size from one frame to the next.  jpeg_scale='auto' then means
        the draft rule per file, draft_scale((file_w, file_h), dst_size), worked out in put(); an integer is that denominator for every file.
        Every submit decodes into a staging buffer of uniform slots, n_streams * ceil(height / scale) * ceil(width / scale) * 3 bytes -- with
        'auto' or 1 that is n_streams * height * width * 3: 9.6 GB for 1 536 streams accepting up to 1920 x 1080.  It is the price of uniform
        slots and the caller's to size.
        jpeg_std_tables ('jpeg' only): baseline files that leave a Huffman table slot 0 / 1 undefined (MJPG cameras send no DHT segment) decode
        with the Annex K.3 tables (deepdish_amd.jpeg.JpegDecoder(std_tables=True)); without it such a file is ST_HEADER, as ever."""
        self._h = None
        if pixel_format not in PIXEL_FORMATS:
            raise ValueError("pixel_format %r is none of 'bgr', 'nv12', 'i420', 'yuy2', 'uyvy', 'jpeg', 'bayer_rggb', 'bayer_grbg', 'bayer_gbrg', 'bayer_bggr', 'gray'%s"
                             % (pixel_format, " (packed Y0 U Y1 V is spelt 'yuy2', its FOURCC)" if pixel_format == 'yuyv'
                                else " (8-bit monochrome is spelt 'gray')" if pixel_format == 'grey' else ''))
        self.pixel_format = pixel_format
        self.sw, self.sh = src_size
        self.dw, self.dh = dst_size or src_size
        if pixel_format in ('nv12', 'i420') and (self.sw % 2 or self.sh % 2):
            raise ValueError('%s frames need an even width and height, got %dx%d' % (pixel_format, self.sw, self.sh))
        if pixel_format in PACKED_422 and self.sw % 2:
            raise ValueError('%s frames need an even width, got %dx%d' % (pixel_format, self.sw, self.sh))
        if pixel_format in BAYER and (self.sw < 3 or self.sh < 3):
            raise ValueError('%s frames need a width and height of at least 3, got %dx%d' % (pixel_format, self.sw, self.sh))
        if pixel_format != 'jpeg' and jpeg_scale != 1:
            raise ValueError("jpeg_scale %r: only a 'jpeg' ring decodes, a %r ring has nothing to scale" % (jpeg_scale, pixel_format))
        if pixel_format != 'jpeg' and jpeg_any_size:
            raise ValueError("jpeg_any_size: only a 'jpeg' ring decodes, a %r ring has no files to take" % (pixel_format,))
        if pixel_format != 'jpeg' and jpeg_std_tables:
            raise ValueError("jpeg_std_tables: only a 'jpeg' ring decodes, a %r ring has no files to take" % (pixel_format,))
        self.jpeg_any_size, self.jpeg_std_tables = bool(jpeg_any_size), bool(jpeg_std_tables)
        self.jpeg_scale_auto = self.jpeg_any_size and jpeg_scale == 'auto'          # per file, in put(); the slots are sized for scale 1
        if self.jpeg_scale_auto:
            jpeg_scale = 1
        if jpeg_scale == 'auto':
            from .jpeg import draft_scale
            jpeg_scale = draft_scale((self.sw, self.sh), (self.dw, self.dh))
        if isinstance(jpeg_scale, bool) or jpeg_scale not in (1, 2, 4, 8):
            raise ValueError("jpeg_scale %r is none of 1, 2, 4, 8, 'auto'" % (jpeg_scale,))
        self.jpeg_scale = int(jpeg_scale)
        if pixel_format != 'jpeg' and jpeg_progressive:
            raise ValueError("jpeg_progressive: only a 'jpeg' ring decodes, a %r ring has no files to take" % (pixel_format,))
        self.jpeg_progressive = bool(jpeg_progressive)
        if pixel_format != 'jpeg' and jpeg_split:
            raise ValueError("jpeg_split: only a 'jpeg' ring decodes, a %r ring has no files to split" % (pixel_format,))
        self.jpeg_split = bool(jpeg_split)
        self.ctx = context or default_context()
        self.S, self.slots = int(n_streams), int(slots)
        h = P()
        if pixel_format == 'bgr':
            check(lib().dd_ingest_create(self.ctx.handle, self.slots, self.S, self.sh, self.sw, self.dh, self.dw, int(bool(flip)),
                                         ctypes.byref(h)), 'dd_ingest_create')
        elif pixel_format == 'jpeg':
            self.jpeg_slot_bytes = int(jpeg_slot_bytes) if jpeg_slot_bytes else self.S * self.sw * self.sh * 3 // 8
            if self.jpeg_progressive or self.jpeg_split or self.jpeg_any_size or self.jpeg_std_tables:
                flags = (1 if self.jpeg_progressive else 0) | (2 if self.jpeg_split else 0) | (4 if self.jpeg_any_size else 0) | (8 if self.jpeg_std_tables else 0)
                check(lib().dd_ingest_create_jpeg_ex(self.ctx.handle, self.slots, self.S, self.sh, self.sw, self.dh, self.dw, int(bool(flip)),
                                                     0 if self.jpeg_scale_auto else self.jpeg_scale, flags, self.jpeg_slot_bytes, ctypes.byref(h)), 'dd_ingest_create_jpeg_ex')
            elif self.jpeg_scale == 1:
                check(lib().dd_ingest_create_jpeg(self.ctx.handle, self.slots, self.S, self.sh, self.sw, self.dh, self.dw, int(bool(flip)),
                                                  self.jpeg_slot_bytes, ctypes.byref(h)), 'dd_ingest_create_jpeg')
            else:
                check(lib().dd_ingest_create_jpeg_scaled(self.ctx.handle, self.slots, self.S, self.sh, self.sw, self.dh, self.dw, int(bool(flip)),
                                                         self.jpeg_scale, self.jpeg_slot_bytes, ctypes.byref(h)), 'dd_ingest_create_jpeg_scaled')
        elif pixel_format in RAW8:
            check(lib().dd_ingest_create_raw8(self.ctx.handle, self.slots, self.S, self.sh, self.sw, self.dh, self.dw, int(bool(flip)),
                                              PIXEL_FORMATS[pixel_format], ctypes.byref(h)), 'dd_ingest_create_raw8')
        else:
            check(lib().dd_ingest_create_format(self.ctx.handle, self.slots, self.S, self.sh, self.sw, self.dh, self.dw, int(bool(flip)),
                                                PIXEL_FORMATS[pixel_format], ctypes.byref(h)), 'dd_ingest_create_format')
        self._h = h
        self._host = []
        for i in range(self.slots if pixel_format != 'jpeg' else 0):
            p, n = ctypes.c_void_p(), ctypes.c_int64()
            check(lib().dd_ingest_host_slot(self._h, i, ctypes.byref(p), ctypes.byref(n)), 'dd_ingest_host_slot')
            buf = (ctypes.c_uint8 * n.value).from_address(p.value)
            if pixel_format == 'bgr':
                shape = (self.S, self.sh, self.sw, 3)
            elif pixel_format in PACKED_422:
                shape = (self.S, self.sh, self.sw, 2)
            elif pixel_format in RAW8:
                shape = (self.S, self.sh, self.sw)
            else:
                shape = (self.S, self.sh * 3 // 2, self.sw)
            self._host.append(np.frombuffer(buf, dtype=np.uint8).reshape(shape))

    def __del__(self):
        try:
            if self._h:
                self._host = []
                lib().dd_ingest_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def host(self, slot):
        """Pinned numpy view of a slot, [S, src_h, src_w, 3] for BGR, [S, src_h * 3 // 2, src_w] for NV12 / I420, [S, src_h, src_w, 2]
        for YUY2 / UYVY and [S, src_h, src_w] for a Bayer mosaic or gray (the shapes cv2 gives such frames): fill it, then submit(slot).  Blocks until the slot's previous upload has left the host buffer."""
        if self.pixel_format == 'jpeg':
            raise ValueError("a 'jpeg' ring has no raw slot to fill: hand each stream's file to put(slot, stream, data)")
        check(lib().dd_ingest_wait_uploaded(self._h, slot), 'dd_ingest_wait_uploaded')
        return self._host[slot]

    def put(self, slot, stream, data):
        """'jpeg' rings: stream `stream`'s next frame as a baseline JPEG file (bytes).  Blocks until the slot's previous upload has left
        it, copies the file into the slot's arena and parses its header here, on the calling thread (several threads may put into one
        slot at once).  A full arena raises (DD_E_CAPACITY, -4).  A file that is refused or of another size is accepted here and shows
        in status(slot)."""
        data = bytes(data)
        check(lib().dd_ingest_jpeg_put(self._h, int(slot), int(stream), data, len(data)), 'dd_ingest_jpeg_put')

    def status(self, slot):
        """'jpeg' rings: int32 [S], deepdish_amd.jpeg.ST_* per stream of the slot's last submit (waits for it).  A stream with a
        non-zero status has unspecified pixels in its own frame and costs the others nothing."""
        out = np.empty(self.S, np.int32)
        check(lib().dd_ingest_status(self._h, int(slot), out.ctypes.data_as(P)), 'dd_ingest_status')
        return out

    def source_sizes(self, slot):
        """jpeg_any_size rings: int32 [S, 3] = (width, height, scale) of the file each stream put into the slot, zeros where nothing was put
        or the header was refused (a file too large keeps the size it stated).  What put() learnt on the host: it does not wait."""
        out = np.zeros((self.S, 3), np.int32)
        check(lib().dd_ingest_source_sizes(self._h, int(slot), out.ctypes.data_as(P)), 'dd_ingest_source_sizes')
        return out

    def present(self, slot):
        """uint8 [S]: the mask MultiStreamPipeline.step(..., present=) takes for this slot's frames -- status(slot) == 0 on a 'jpeg' ring
        (a stream whose file was refused, of another size, damaged or missing is absent from the step, as a failed cap.read() is
        dropped), all ones on the raw rings.  Like status() it waits for the slot's decode on a 'jpeg' ring."""
        if self.pixel_format != 'jpeg':
            return np.ones(self.S, np.uint8)
        return (self.status(slot) == 0).astype(np.uint8)

    def submit(self, slot):
        check(lib().dd_ingest_submit(self._h, slot), 'dd_ingest_submit')

    def acquire(self, slot, stream=None):
        """-> device address of u8 [S, dst_h, dst_w, 3]; the consumer stream waits for the slot's upload."""
        p = ctypes.c_void_p()
        check(lib().dd_ingest_acquire(self._h, slot, stream, ctypes.byref(p)), 'dd_ingest_acquire')
        return p.value

    def release(self, slot, stream=None):
        check(lib().dd_ingest_release(self._h, slot, stream), 'dd_ingest_release')

    def frames(self, slot, stream=None):
        """acquire() wrapped as an object with .shape / .data_ptr() (what MultiStreamPipeline.step takes)."""
        return _DevView(self.acquire(slot, stream), (self.S, self.dh, self.dw, 3))


class _DevView:
    """Minimal stand-in for a device tensor: what runtime.ptr() and MultiStreamPipeline.step need."""

    def __init__(self, addr, shape):
        self._addr, self.shape = addr, shape

    def data_ptr(self):
        return self._addr


def yuv420_to_bgr(src, height, width, layout, pitch=0, chroma_offset=0, frame_stride=0, out=None, context=None, stream=None):
    """NV12 / I420 frames in device memory -> u8 [batch, height, width, 3] BGR device tensor (cv2.cvtColor COLOR_YUV2BGR_NV12 / _I420
    restated).  src: u8 device tensor, [batch, height * 3 // 2, width] when dense; a decoder's padded surfaces are described by
    pitch (bytes per luma row), chroma_offset (frame start -> chroma) and frame_stride, 0 meaning dense -- the batch is then what
    fits.  out: a tensor to write into (the batch is then its first dimension).  The launch is queued on the context's stream (or
    `stream`): `context.sync()` before torch reads the result on another stream."""
    import torch
    if layout not in ('nv12', 'i420'):
        raise ValueError("layout %r is neither 'nv12' nor 'i420'" % (layout,))
    ctx = context or default_context()
    p = pitch or width
    co = chroma_offset or p * height
    if layout == 'nv12':
        extent, dense = co + p * (height // 2 - 1) + width, co + p * (height // 2)
    else:
        extent, dense = co + (p // 2) * (height - 1) + width // 2, co + (p // 2) * height
    stride = frame_stride or dense
    if out is not None:
        batch = out.shape[0]
    else:
        batch = max(0, (src.numel() - extent) // stride + 1)
        out = torch.empty((batch, height, width, 3), dtype=torch.uint8, device=src.device)
    if tuple(out.shape[1:]) != (height, width, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError('out must be a contiguous u8 [batch, %d, %d, 3] tensor' % (height, width))
    if src.dtype != torch.uint8 or not src.is_contiguous():
        raise ValueError('src must be a contiguous u8 tensor')
    if batch > 0 and src.numel() < (batch - 1) * stride + extent:
        raise ValueError('src holds %d bytes, %d frames need %d' % (src.numel(), batch, (batch - 1) * stride + extent))
    check(lib().dd_yuv420_to_bgr(ctx.handle, ptr(src), batch, height, width, PIXEL_FORMATS[layout], pitch, chroma_offset, frame_stride,
                                 ptr(out), stream), 'dd_yuv420_to_bgr')
    return out


def yuv422_to_bgr(src, height, width, order, pitch=0, frame_stride=0, out=None, context=None, stream=None):
    """Packed 4:2:2 frames in device memory -> u8 [batch, height, width, 3] BGR device tensor (cv2.cvtColor COLOR_YUV2BGR_YUY2 / _UYVY
    restated).  order: 'yuy2' (Y0 U Y1 V) or 'uyvy' (U Y0 V Y1).  src: u8 device tensor, [batch, height, width, 2] when dense; padded
    surfaces are described by pitch (bytes per row, 0 = 2 * width) and frame_stride (0 = pitch * height) -- the batch is then what
    fits.  out: a tensor to write into (the batch is then its first dimension).  The launch is queued on the context's stream (or
    `stream`): `context.sync()` before torch reads the result on another stream."""
    import torch
    if order not in PACKED_422:
        raise ValueError("order %r is neither 'yuy2' nor 'uyvy'" % (order,))
    ctx = context or default_context()
    p = pitch or 2 * width
    extent = p * (height - 1) + 2 * width
    stride = frame_stride or p * height
    if out is not None:
        batch = out.shape[0]
    else:
        batch = max(0, (src.numel() - extent) // stride + 1)
        out = torch.empty((batch, height, width, 3), dtype=torch.uint8, device=src.device)
    if tuple(out.shape[1:]) != (height, width, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError('out must be a contiguous u8 [batch, %d, %d, 3] tensor' % (height, width))
    if src.dtype != torch.uint8 or not src.is_contiguous():
        raise ValueError('src must be a contiguous u8 tensor')
    if batch > 0 and src.numel() < (batch - 1) * stride + extent:
        raise ValueError('src holds %d bytes, %d frames need %d' % (src.numel(), batch, (batch - 1) * stride + extent))
    check(lib().dd_yuv422_to_bgr(ctx.handle, ptr(src), batch, height, width, PIXEL_FORMATS[order], pitch, frame_stride, ptr(out), stream),
          'dd_yuv422_to_bgr')
    return out


def raw8_to_bgr(src, height, width, layout, pitch=0, frame_stride=0, out=None, context=None, stream=None):
    """8-bit raw sensor frames in device memory -> u8 [batch, height, width, 3] BGR device tensor.  layout: 'bayer_rggb', 'bayer_grbg',
    'bayer_gbrg' or 'bayer_bggr' (cv2.cvtColor COLOR_BayerBG2BGR / _BayerGB2BGR / _BayerGR2BGR / _BayerRG2BGR restated: bilinear, the outer
    ring of pixels repeats its inner neighbour; width and height at least 3) or 'gray' (COLOR_GRAY2BGR).  src: u8 device tensor,
    [batch, height, width] when dense; padded surfaces are described by pitch (bytes per row, 0 = width) and frame_stride (0 = pitch *
    height) -- the batch is then what fits.  out: a tensor to write into (the batch is then its first dimension).  The launch is queued on
    the context's stream (or `stream`): `context.sync()` before torch reads the result on another stream."""
    import torch
    if layout not in RAW8:
        raise ValueError("layout %r is none of 'bayer_rggb', 'bayer_grbg', 'bayer_gbrg', 'bayer_bggr', 'gray'" % (layout,))
    if layout in BAYER and (width < 3 or height < 3):
        raise ValueError('%s frames need a width and height of at least 3, got %dx%d' % (layout, width, height))
    ctx = context or default_context()
    p = pitch or width
    extent = p * (height - 1) + width
    stride = frame_stride or p * height
    if out is not None:
        batch = out.shape[0]
    else:
        batch = max(0, (src.numel() - extent) // stride + 1)
        out = torch.empty((batch, height, width, 3), dtype=torch.uint8, device=src.device)
    if tuple(out.shape[1:]) != (height, width, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError('out must be a contiguous u8 [batch, %d, %d, 3] tensor' % (height, width))
    if src.dtype != torch.uint8 or not src.is_contiguous():
        raise ValueError('src must be a contiguous u8 tensor')
    if batch > 0 and src.numel() < (batch - 1) * stride + extent:
        raise ValueError('src holds %d bytes, %d frames need %d' % (src.numel(), batch, (batch - 1) * stride + extent))
    check(lib().dd_raw8_to_bgr(ctx.handle, ptr(src), batch, height, width, PIXEL_FORMATS[layout], pitch, frame_stride, ptr(out), stream),
          'dd_raw8_to_bgr')
    return out
