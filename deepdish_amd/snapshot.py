"""Stream snapshots of the batched pipeline (MultiStreamPipeline.snapshot / restore): a StreamSnapshot is host bytes only -- the blob of
csrc/snapshot_fmt.h -- so it can be written to a file, cross processes and go to a pipeline on another GPU."""
import ctypes
import struct

import numpy as np

from ._lib import lib, P

_MAGIC, _VERSION = 0x4E534444, 1
_INFO = ('frames_seen', 'n_tracks', 'next_id', 'gallery_rows', 'has_background', 'bytes')


class StreamSnapshot:
    """The state of some streams of a MultiStreamPipeline at one point between two steps, one self-contained entry per stream.
    len(), .info (one dict per entry: frames_seen, n_tracks, next_id, gallery_rows, has_background, bytes), .to_bytes(),
    StreamSnapshot.from_bytes(b), .select(entries)."""

    def __init__(self, blob):
        """blob: bytes-like; validated here (ValueError for one the validator refuses)."""
        own = isinstance(blob, np.ndarray) and blob.dtype == np.uint8 and blob.ndim == 1 and blob.flags.c_contiguous
        self._blob = blob if own else np.frombuffer(bytes(blob), dtype=np.uint8)
        n = ctypes.c_int()
        if lib().dd_snapshot_info(P(self._blob.ctypes.data), int(self._blob.size), ctypes.byref(n), None, 0) != 0:
            raise ValueError(lib().dd_last_error().decode())
        info = np.zeros((n.value, 8), dtype=np.int64)
        if lib().dd_snapshot_info(P(self._blob.ctypes.data), int(self._blob.size), ctypes.byref(n), P(info.ctypes.data), n.value) != 0:
            raise ValueError(lib().dd_last_error().decode())
        self._spans = [(int(r[6]), int(r[5])) for r in info]
        self.info = [dict(zip(_INFO, (int(r[0]), int(r[1]), int(r[2]), int(r[3]), bool(r[4]), int(r[5])))) for r in info]

    def __len__(self):
        return len(self._spans)

    def to_bytes(self):
        return self._blob.tobytes()

    @classmethod
    def from_bytes(cls, b):
        return cls(b)

    def select(self, entries):
        """A snapshot of the listed entries, in the listed order (an entry is self-contained: its bytes are copied)."""
        entries = [int(i) for i in entries]
        for i in entries:
            if not 0 <= i < len(self):
                raise ValueError('entries: indices 0 .. %d, got %r' % (len(self) - 1, entries))
        at = 16 + 16 * len(entries)
        head = [struct.pack('<IIII', _MAGIC, _VERSION, len(entries), 0)]
        for i in entries:
            head.append(struct.pack('<QQ', at, self._spans[i][1]))
            at += self._spans[i][1]
        raw = self._blob.tobytes()
        return StreamSnapshot(b''.join(head + [raw[self._spans[i][0]:self._spans[i][0] + self._spans[i][1]] for i in entries]))
