"""Baseline JPEG files from BGR frames in HBM (csrc/jpeg.hip): the exit of the render path.

The reference hands its annotated output frame to cv2.imencode(".jpg", frame) for the MJPEG web stream (deepdish.py:155-181), to
frame_%06d.jpg under --output-cvat-dir (:764-766) and to the file --stream-path names.  Here the frame is encoded where it was painted:

    enc = JpegEncoder(480, 640)                          # quality 95 (cv2's default), one restart interval per MCU row
    files = enc.encode_to_host(frames_dev)               # u8 [n, 480, 640, 3] BGR on the device -> list of n bytes objects
    part = wire.mjpeg_part(files[0])                     # what deepdish.py:178-179 yields

The bytes are libjpeg's for 8-bit YCbCr 4:2:0 with the ITU-T T.81 Annex K tables: Pillow's
Image.save(f, 'JPEG', quality=q, subsampling='4:2:0', restart_marker_rows=r) byte for byte, header included (tests/test_jpeg_ref.py,
tests/test_gpu_jpeg.py).  The one deviation from cv2.imencode is the DRI segment and the RSTn markers, which cv2 does not write and every
decoder honours: a restart interval is the unit of parallel work.  Parity with OpenCV's own bytes is not pinned.

The way in is the mirror (csrc/jpeg_parse.h, csrc/jpeg_dec.hip): `parse(file)` reads a baseline file's header on the host, and
`JpegDecoder(H, W).decode(files)` turns files in host memory into BGR frames in HBM, byte for byte libjpeg's pixels (tests/jpeg_dec_ref.py,
tests/test_gpu_jpeg_decode.py); the ingest ring's `pixel_format='jpeg'` slots (deepdish_amd/ingest.py) are built on it.  With `scale=2`, 4
or 8 the decoder transforms every 8 x 8 block straight to 4 x 4, 2 x 2 or 1 x 1 samples, libjpeg's scale_denom and Pillow's Image.draft
(tests/jpeg_scaled_ref.py), and `draft_scale(src, want)` picks the scale as Pillow does.

Progressive (SOF2) files -- what cv2.imread reads without being asked, and what a CVAT directory re-saved by a tool usually holds -- are an
option: `parse(file, progressive=True)`, `JpegDecoder(H, W, progressive=True)` and `FrameIngest(..., jpeg_progressive=True)`
(tests/jpeg_prog_ref.py is the definition; jpeg_prog_entropy_k runs once per level of the scan script).  Without the option such a file is
refused as before (reason 'progressive', ST_HEADER).

Files without restart markers -- what an MJPEG camera, cv2.imencode and Pillow write by default -- are one entropy-coded segment, which the
decoder gives to a single lane.  `JpegDecoder(H, W, split=True)` and `FrameIngest(..., jpeg_split=True)` cut such a scan into subsequences
of DD_JPEGDEC_SPLIT_BYTES (by default 64, doubled per file until a workgroup's lanes have one each) that many lanes decode from guessed states until they agree (jpeg_split_entropy_k); the frames
are the same bytes.  `split_stats()` says what the last decode took.

A camera fleet delivers VGA, 720p, 1080p and 4K side by side, and the reference stretches whatever arrives to its input size (deepdish.py:867).
`JpegDecoder(H, W, any_size=True)` and `FrameIngest(..., jpeg_any_size=True)` take every file of at most H x W, each at its own scale
(`decode(files, scales=[...])`; on the ring `jpeg_scale='auto'` is then Pillow's draft rule per file), into the top-left corner of uniform
slots.  UVC webcams in MJPG mode and MJPG AVI frames carry no DHT segment: `parse(file, std_tables=True)`, `JpegDecoder(..., std_tables=True)`
and `FrameIngest(..., jpeg_std_tables=True)` give every undefined table slot 0 / 1 of a baseline file its ITU-T T.81 Annex K.3 table, as
libjpeg-turbo does.  Both are off unless asked for."""
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


# ------------------------------------------------------------------------------------------------ decoder (csrc/jpeg_dec.hip)
DEC_PATH_LDS, DEC_PATH_PLANES = 0, 1
E_FORMAT = -5
ST_OK, ST_HEADER, ST_SIZE, ST_DATA, ST_NO_FRAME = 0, 1, 2, 3, 4
REASONS = {0: 'ok', 1: 'truncated', 2: 'progressive', 3: 'arithmetic', 4: 'lossless', 5: 'precision', 6: 'components', 7: 'sampling',
           8: 'scans', 9: 'huffman', 10: 'undefined', 11: 'size', 12: 'segment',
           13: 'ac_components', 14: 'ac_before_dc', 15: 'first_ah', 16: 'refinement', 17: 'incomplete', 18: 'capacity'}
MAX_SCANS, MAX_TABLES, MAX_LEVELS = 64, 32, 16
DEC_PROGRESSIVE, DEC_SPLIT, DEC_ANY_SIZE, DEC_STD_TABLES = 1, 2, 4, 8


class _Huff(ctypes.Structure):
    _fields_ = [('bits', ctypes.c_uint8 * 16), ('vals', ctypes.c_uint8 * 256), ('look', ctypes.c_uint16 * 256), ('maxcode', ctypes.c_int32 * 18),
                ('valoff', ctypes.c_int32 * 18), ('nvals', ctypes.c_int32), ('defined', ctypes.c_int32)]


class JpegInfo(ctypes.Structure):
    """dd_jpeg_info of include/deepdish_hip.h."""
    _fields_ = ([('reason', ctypes.c_int32), ('height', ctypes.c_int32), ('width', ctypes.c_int32), ('ncomp', ctypes.c_int32), ('sof', ctypes.c_int32)]
                + [(k, ctypes.c_int32 * 3) for k in ('hs', 'vs', 'tq', 'td', 'ta')]
                + [(k, ctypes.c_int32) for k in ('hmax', 'vmax', 'mcus_x', 'mcus_y', 'blocks_per_mcu', 'restart_interval', 'n_intervals', 'scan_offset',
                                                 'scan_length')]
                + [('quant_defined', ctypes.c_int32 * 4)]
                + [(k, ctypes.c_int32) for k in ('status', 'path', 'interval_base', 'reserved')]
                + [('file_offset', ctypes.c_int64), ('quant', (ctypes.c_uint16 * 64) * 4), ('huff', _Huff * 4)])


class JpegScan(ctypes.Structure):
    """dd_jpeg_scan of include/deepdish_hip.h."""
    _fields_ = ([('offset', ctypes.c_int32), ('length', ctypes.c_int32), ('ncomp', ctypes.c_int32), ('comp', ctypes.c_int32 * 3), ('dc', ctypes.c_int32 * 3)]
                + [(k, ctypes.c_int32) for k in ('ac', 'ss', 'se', 'ah', 'al', 'restart_interval', 'blocks_x', 'blocks_y', 'n_intervals', 'level', 'interval_base')])


class JpegScans(ctypes.Structure):
    """dd_jpeg_scans of include/deepdish_hip.h."""
    _fields_ = [('n_scans', ctypes.c_int32), ('n_tables', ctypes.c_int32), ('n_levels', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('level_base', ctypes.c_int32 * MAX_LEVELS), ('scan', JpegScan * MAX_SCANS), ('pool', _Huff * MAX_TABLES)]


def parse(file, progressive=False, std_tables=False):
    """The header of a baseline JPEG file, SOI .. the first SOS, as dd_jpeg_parse reads it -> dict.  Needs no device.  A file that is
    refused raises DeepDishHipError with .reason (a word of REASONS) and the reason spelt out in the message.

    progressive=True reads progressive (SOF2) files as well (dd_jpeg_parse_scans, which walks the whole file): the dict then holds the frame
    ('sof' 0xC2, no 'td' / 'ta' / 'huff', 'n_intervals' 0) and 'scans', one dict per SOS in file order -- 'comps', 'ss', 'se', 'ah', 'al',
    'restart_interval' (the DRI in force: MCUs for a scan of several components, the component's blocks for one), 'blocks_x', 'blocks_y',
    'n_intervals', 'level', 'offset', 'length' and 'dc' / 'ac', the (bits, vals) of the tables it reads -- with 'n_levels' and 'n_tables'.  A
    baseline file gives the same dict as without the option.

    std_tables=True (dd_jpeg_parse_flags): every DC / AC table slot 0 or 1 that a component of a baseline file references and the file does
    not define is the Annex K.3 table of that slot (0 luminance, 1 chrominance), in 'huff' like a table the file carries; without it such a
    file is refused with reason 'undefined'.  A table id above 1 and a progressive file with an undefined table stay refused."""
    data = bytes(file)
    info = JpegInfo()
    scans = JpegScans() if progressive else None
    who = 'dd_jpeg_parse_flags' if std_tables else 'dd_jpeg_parse_scans' if progressive else 'dd_jpeg_parse'
    if std_tables:
        rc = lib().dd_jpeg_parse_flags(data, len(data), DEC_STD_TABLES, ctypes.byref(info), ctypes.byref(scans) if progressive else None)
    elif progressive:
        rc = lib().dd_jpeg_parse_scans(data, len(data), ctypes.byref(info), ctypes.byref(scans))
    else:
        rc = lib().dd_jpeg_parse(data, len(data), ctypes.byref(info))
    if rc != 0:
        msg = lib().dd_last_error()
        err = DeepDishHipError('%s failed (%d): %s' % (who, rc, msg.decode() if msg else '?'))
        err.code, err.reason = rc, REASONS.get(info.reason, '?') if rc == E_FORMAT else None
        raise err
    nc = info.ncomp
    out = {k: getattr(info, k) for k in ('height', 'width', 'ncomp', 'sof', 'hmax', 'vmax', 'mcus_x', 'mcus_y', 'blocks_per_mcu', 'restart_interval',
                                          'n_intervals', 'scan_offset', 'scan_length')}
    out['comps'] = [(info.hs[c], info.vs[c], info.tq[c]) for c in range(nc)]
    out['td'], out['ta'] = list(info.td[:nc]), list(info.ta[:nc])
    out['quant'] = {t: np.array(info.quant[t][:], np.int64) for t in range(4) if info.quant_defined[t]}
    out['huff'] = {(t >> 1, t & 1): (list(info.huff[t].bits), list(info.huff[t].vals[:info.huff[t].nvals])) for t in range(4) if info.huff[t].defined}
    if progressive and scans.n_scans:
        def table(i):
            return (list(scans.pool[i].bits), list(scans.pool[i].vals[:scans.pool[i].nvals])) if i >= 0 else None
        out['scans'] = []
        for k in range(scans.n_scans):
            sc = scans.scan[k]
            d = {f: getattr(sc, f) for f in ('ss', 'se', 'ah', 'al', 'restart_interval', 'blocks_x', 'blocks_y', 'n_intervals', 'level', 'offset', 'length')}
            d['comps'] = list(sc.comp[:sc.ncomp])
            d['dc'], d['ac'] = [table(sc.dc[j]) for j in range(sc.ncomp)], table(sc.ac)
            out['scans'].append(d)
        out['n_levels'], out['n_tables'] = scans.n_levels, scans.n_tables
    return out


def decoder_plan(H, W, ncomp=3, hs=2, vs=2, scale=1):
    """-> (path, rows of a band, bands): DEC_PATH_LDS keeps a band's sample planes in LDS, DEC_PATH_PLANES takes them through HBM.
    H x W is the file's size; at scale 2, 4 or 8 the rows and bands are those of the scaled frame, and a band needs less LDS.
    Needs no device."""
    path, rows, bands = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    if scale == 1:
        check(lib().dd_jpegdec_plan(int(H), int(W), int(ncomp), int(hs), int(vs), ctypes.byref(path), ctypes.byref(rows), ctypes.byref(bands)), 'dd_jpegdec_plan')
    else:
        check(lib().dd_jpegdec_plan_scaled(int(H), int(W), int(ncomp), int(hs), int(vs), int(scale), ctypes.byref(path), ctypes.byref(rows), ctypes.byref(bands)),
              'dd_jpegdec_plan_scaled')
    return path.value, rows.value, bands.value


def draft_scale(src_size, want_size):
    """Pillow's Image.draft rule for files of src_size = (width, height) wanted at want_size = (width, height): the largest of 8, 4, 2, 1
    that is <= min(sw // dw, sh // dh), and 1 when that is 0 -- the cheapest decode that is still at least as large as what is wanted.
    Needs no device."""
    (sw, sh), (dw, dh) = src_size, want_size
    s = lib().dd_jpeg_draft_scale(int(sw), int(sh), int(dw), int(dh))
    if s < 1:
        check(s, 'dd_jpeg_draft_scale')
    return s


class JpegDecoder:
    """Baseline JPEG files of one frame size, H x W, in host memory -> BGR frames in HBM, byte for byte libjpeg's (Pillow's
    Image.open(f).convert('RGB') with the channels swapped; parity with OpenCV's decode is not pinned).  Files of one call may differ
    in sampling (4:2:0, 4:2:2, 4:4:4, greyscale), tables and restart interval.

        dec = JpegDecoder(480, 640, max_frames=64)
        frames, status = dec.decode(files)           # u8 [n, 480, 640, 3] and int32 [n] on the device

    status: ST_OK; ST_HEADER (refused: parse(file) says why) and ST_SIZE (not H x W) leave the frame untouched; ST_DATA (corrupt or
    truncated entropy data) leaves unspecified bytes in that frame alone; ST_NO_FRAME for an empty file.

    scale=2, 4 or 8 decodes at that fraction, as libjpeg's scale_denom does (Pillow's im.draft(mode, (W // scale, H // scale)), byte for
    byte; parity with cv2.IMREAD_REDUCED_COLOR_* is not pinned): H x W stays what a file must state, and the frames are
    [n, out_H, out_W, 3] with out_H = ceil(H / scale), out_W = ceil(W / scale).

    progressive=True makes the decoder take progressive (SOF2) files too, at any scale, beside baseline files in the same call: byte for
    byte libjpeg's pixels for a complete file (tests/jpeg_prog_ref.py).  parse(file, progressive=True) says what is refused: among it a
    script that leaves coefficients undelivered, which libjpeg would smooth or zero-fill.  A decoder without the option gives such files
    ST_HEADER and launches exactly what it always did.

    split=True, with any scale and with or without progressive: a baseline file that is a single restart interval and whose scan is longer
    than DD_JPEGDEC_SPLIT_BYTES (read here; a power of two, 16 .. 4096; 64 when not set) is decoded by a workgroup, not by one lane; every
    other file of the call goes the usual way.  Frames and statuses are the same; split_stats() counts what the last decode did.

    any_size=True, with any of the above: H x W is the largest file accepted, not the only one.  A file with 1 <= height <= H and
    1 <= width <= W is ST_OK, one with either side larger ST_SIZE.  The frames stay [n, out_H, out_W, 3]: frame i is the top-left
    ceil(h_i / s_i) x ceil(w_i / s_i) of its slot -- the pixels a decoder of that file's own size and scale gives -- and no other byte of the
    slot is written.  decode(files, scales=[...]) gives each file its own denominator; `scale` is then the smallest a call may use (it fixes
    out_H x out_W), and a smaller entry raises (DD_E_ARG).

    std_tables=True: a baseline file that leaves a Huffman table slot 0 / 1 undefined (MJPG cameras send no DHT segment) decodes with the
    Annex K.3 table there, as libjpeg-turbo does; see parse(file, std_tables=True).  Without it such a file is ST_HEADER."""

    def __init__(self, H, W, max_frames=16, max_bytes=None, context=None, scale=1, progressive=False, split=False, any_size=False, std_tables=False):
        from .runtime import default_context
        self.ctx = context or default_context()
        self.H, self.W, self.max_frames = int(H), int(W), int(max_frames)
        self.max_bytes = int(max_bytes) if max_bytes else self.max_frames * (self.H * self.W * 3 + 4096)
        self._h = None
        self.scale = scale
        self.progressive = bool(progressive)
        self.split = bool(split)
        self.any_size = bool(any_size)
        self.std_tables = bool(std_tables)
        h = P()
        if scale != 1 and (not isinstance(scale, int) or isinstance(scale, bool)):
            raise ValueError('scale %r is none of 1, 2, 4, 8' % (scale,))
        if self.progressive or self.split or self.any_size or self.std_tables:
            flags = ((DEC_PROGRESSIVE if self.progressive else 0) | (DEC_SPLIT if self.split else 0) | (DEC_ANY_SIZE if self.any_size else 0)
                     | (DEC_STD_TABLES if self.std_tables else 0))
            check(lib().dd_jpegdec_create_ex(self.ctx.handle, self.H, self.W, scale, flags, self.max_frames, self.max_bytes, ctypes.byref(h)),
                  'dd_jpegdec_create_ex')
        elif scale == 1:
            check(lib().dd_jpegdec_create(self.ctx.handle, self.H, self.W, self.max_frames, self.max_bytes, ctypes.byref(h)), 'dd_jpegdec_create')
        else:
            check(lib().dd_jpegdec_create_scaled(self.ctx.handle, self.H, self.W, scale, self.max_frames, self.max_bytes, ctypes.byref(h)),
                  'dd_jpegdec_create_scaled')
        self._h = h
        oh, ow = ctypes.c_int(), ctypes.c_int()
        check(lib().dd_jpegdec_output_size(self._h, ctypes.byref(oh), ctypes.byref(ow)), 'dd_jpegdec_output_size')
        self.out_H, self.out_W = oh.value, ow.value

    def __del__(self):
        try:
            if self._h:
                lib().dd_jpegdec_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def profile(self, on=True):
        """Record device events around the parts of every decode; read them with kernel_ms()."""
        check(lib().dd_jpegdec_profile(self._h, int(bool(on))), 'dd_jpegdec_profile')

    def kernel_ms(self):
        """-> {'upload', 'markers', 'entropy', 'pixels'}: milliseconds of the last profiled decode (waits for it)."""
        ms = (ctypes.c_float * 4)()
        check(lib().dd_jpegdec_profile_read(self._h, ms), 'dd_jpegdec_profile_read')
        return dict(zip(('upload', 'markers', 'entropy', 'pixels'), (float(v) for v in ms)))

    def level_ms(self):
        """progressive=True: milliseconds of jpeg_prog_entropy_k per level in the last profiled decode (waits for it); [] when the call held
        no progressive file.  kernel_ms()['entropy'] covers them and jpeg_entropy_k."""
        ms, n = (ctypes.c_float * MAX_LEVELS)(), ctypes.c_int()
        check(lib().dd_jpegdec_profile_levels(self._h, ms, ctypes.byref(n)), 'dd_jpegdec_profile_levels')
        return [float(v) for v in ms[:n.value]]

    def split_stats(self):
        """-> {'files', 'subsequences', 'max_rounds', 'lane_decodes'} of the last decode (waits for it): files that went to
        jpeg_split_entropy_k, the subsequences they were cut into, the most rounds one of them took (at most its subsequences + 1) and how
        often a subsequence was decoded in the rounds (the storing decode not counted).  All zeros on a decoder made without split=True."""
        out = (ctypes.c_int64 * 4)()
        check(lib().dd_jpegdec_split_stats(self._h, out), 'dd_jpegdec_split_stats')
        return dict(zip(('files', 'subsequences', 'max_rounds', 'lane_decodes'), (int(v) for v in out)))

    def decode(self, files, out=None, status=None, stream=None, scales=None):
        """files: a list of bytes objects -> (u8 [n, out_H, out_W, 3], int32 [n]).  out / status: tensors to write instead of new ones.  Queued on the context's stream (or
        `stream`): `context.sync()` before torch reads the result on another stream.  scales (any_size=True only): one of 1, 2, 4, 8 per
        file, none below the decoder's `scale`."""
        import torch
        n = len(files)
        lens = np.array([len(f) for f in files], np.int64)
        offs = np.zeros(n, np.int64)
        if n > 1:
            offs[1:] = np.cumsum((lens[:-1] + 63) & ~63)
        blob = bytearray(int(offs[-1] + lens[-1]) if n else 0)
        for f, o in zip(files, offs):
            blob[int(o):int(o) + len(f)] = f
        buf = (ctypes.c_uint8 * max(1, len(blob))).from_buffer(blob)
        dev = torch.device('cuda', self.ctx.device)
        if out is None:
            out = torch.empty((n, self.out_H, self.out_W, 3), dtype=torch.uint8, device=dev)
        if status is None:
            status = torch.empty(n, dtype=torch.int32, device=dev)
        assert tuple(out.shape) == (n, self.out_H, self.out_W, 3) and out.dtype == torch.uint8 and out.is_contiguous()
        assert tuple(status.shape) == (n,) and status.dtype == torch.int32
        torch.cuda.current_stream(out.device).synchronize()
        if scales is not None:
            sc = np.ascontiguousarray(scales, np.int32)
            if sc.shape != (n,):
                raise ValueError('scales: %d entries for %d files' % (sc.size, n))
            check(lib().dd_jpegdec_decode_scales(self._h, buf, offs.ctypes.data_as(P), lens.ctypes.data_as(P), sc.ctypes.data_as(P), n, P(out.data_ptr()),
                                                 P(status.data_ptr()), stream), 'dd_jpegdec_decode_scales')
            return out, status
        check(lib().dd_jpegdec_decode(self._h, buf, offs.ctypes.data_as(P), lens.ctypes.data_as(P), n, P(out.data_ptr()), P(status.data_ptr()), stream),
              'dd_jpegdec_decode')
        return out, status
