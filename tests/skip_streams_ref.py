"""Test-side restatement of the per-stream form of --object-detector-skip-frames (MultiStreamPipeline(object_detector_skip_frames=[...],
object_detector_skip_phase=[...]), dd_pipeline_detector_skip_streams): tests/skip_frames_ref.py's rule (deepdish.py:892-893,929-938,
1003-1014 upstream) applied to one stream's own present frames, plus `phase` -- this build's addition, which sets the counter after the
stream's FIRST detector step to phase instead of N and so only shortens the first cycle.  Test infrastructure only."""
import skip_frames_ref as ref


def schedule(n, phase, frames):
    """-> [True where the detector runs] over `frames` present frames of one stream with skip count n and phase (None: none)."""
    rem, has, out = 0, False, []
    for _ in range(frames):
        if rem > 0 and has:
            rem -= 1
            out.append(False)
        else:
            rem = phase if (not has and phase is not None) else (n or 0)
            has = True
            out.append(True)
    return out


class Stream(ref.Stream):
    """skip_frames_ref.Stream with a phase: after its first detector step the counter is phase, after every later one n."""

    def __init__(self, encode, line, n=None, phase=None, **kw):
        super().__init__(encode, line, n=n, **kw)
        self.phase = phase

    def step(self, frame, detections, fg_mask=None):
        first = self.prev_objd is None
        out = super().step(frame, detections, fg_mask)
        if first and self.phase is not None:          # the first step of a stream is always a detector step
            self.skip_rem = self.phase
        return out
