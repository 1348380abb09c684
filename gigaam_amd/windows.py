"""Longform without a speech detector: fixed overlapping windows whose kept frames tile the recording (host side, pure Python).

A recording is cut into windows of ``C`` encoder frames that start every ``step = C - 2 S`` frames; the ``S`` frames at each inner
window edge saw too little context and are dropped, the rest of every window is kept, and the kept ranges tile one stream of
``T_total`` frames with no gap and no overlap -- the ``chunk_length_s`` / ``stride_length_s`` convention of the Hugging Face ASR
pipeline.  ``plan_windows`` makes that table; ``gam_op_ctc_stitch`` (gigaam_amd/csrc/gam_stitch.h) executes it on the device.
``segment_words`` cuts the words of the decoded stream into segments.  Nothing here touches a GPU."""
from __future__ import annotations

import math
from bisect import bisect_right
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

MAX_CHUNK_S = 25.0    # ``transcribe``'s own limit (model.LONGFORM_THRESHOLD)


@dataclass(frozen=True)
class Window:
    """One window: samples ``[start, stop)`` of the file; its local encoder frames ``[lo, hi)`` are kept and land on rows
    ``[dst, dst + hi - lo)`` of the stitched stream; local frame j lies at ``start_s + j * shift`` seconds in the file."""
    start: int
    stop: int
    lo: int
    hi: int
    dst: int
    start_s: float
    shift: float


@dataclass(frozen=True)
class WindowPlan:
    windows: Tuple[Window, ...]
    t_total: int          # frames of the stitched stream
    chunk_frames: int     # C
    stride_frames: int    # S
    step_frames: int      # C - 2 S

    def locate(self, frames: Sequence[int]) -> Tuple[List[int], List[int], List[float]]:
        """Frames of the stitched stream -> per frame (window it was kept from, local frame inside that window -- ``lo`` included --,
        time in the file = the window's start + local frame x the window's frame shift)."""
        bounds = [w.dst for w in self.windows]
        wins, local, times = [], [], []
        for f in frames:
            f = int(f)
            if f < 0 or f >= self.t_total:
                raise ValueError(f"frame {f} outside the {self.t_total} stitched frames")
            k = bisect_right(bounds, f) - 1
            w = self.windows[k]
            j = w.lo + f - w.dst
            wins.append(k)
            local.append(j)
            times.append(w.start_s + j * w.shift)
        return wins, local, times

    def spans(self) -> List[Tuple[float, float]]:
        """(start, end) seconds of every window's kept frames: a window's span ends where the next one's begins (the last: one frame
        shift behind its last frame), so the spans tile the file."""
        starts = [w.start_s + w.lo * w.shift for w in self.windows]
        ends = starts[1:] + ([self.windows[-1].start_s + self.windows[-1].hi * self.windows[-1].shift] if self.windows else [])
        return list(zip(starts, ends))


def plan_windows(n_samples: int, frame_samples: int, enc_frames_of: Callable[[int], int], chunk_length_s: float = 20.0,
                 stride_length_s: Optional[float] = None, sample_rate: int = 16000) -> WindowPlan:
    """The window table of a recording of ``n_samples`` samples.  ``frame_samples``: samples per encoder frame (hop length x
    subsampling factor); ``enc_frames_of(n)``: encoder frames of an n-sample clip (the host length formula).  ``stride_length_s``
    defaults to ``chunk_length_s / 6`` -- the Hugging Face convention, not a measured optimum.  ``ValueError`` for a non-positive or
    non-finite chunk, a chunk beyond 25 s, a negative stride, or a stride that leaves no step (2 S >= C)."""
    if stride_length_s is None:
        stride_length_s = chunk_length_s / 6.0
    chunk_length_s, stride_length_s = float(chunk_length_s), float(stride_length_s)
    if not math.isfinite(chunk_length_s) or chunk_length_s <= 0:
        raise ValueError(f"chunk_length_s must be positive and finite, got {chunk_length_s}")
    if chunk_length_s > MAX_CHUNK_S:
        raise ValueError(f"chunk_length_s {chunk_length_s} beyond the {MAX_CHUNK_S:g} s a single clip may have")
    if not math.isfinite(stride_length_s) or stride_length_s < 0:
        raise ValueError(f"stride_length_s must be >= 0 and finite, got {stride_length_s}")
    if n_samples < 0 or frame_samples < 1:
        raise ValueError(f"bad geometry: n_samples={n_samples} frame_samples={frame_samples}")
    c = int(math.floor(chunk_length_s * sample_rate / frame_samples + 0.5))
    s = int(math.floor(stride_length_s * sample_rate / frame_samples + 1e-9))
    step = c - 2 * s
    if c < 1 or step < 1:
        raise ValueError(f"chunk of {c} frames with a stride of {s} frames on each side leaves no step (2 S >= C)")
    windows: List[Window] = []
    k = 0
    while True:
        start = k * step * frame_samples
        stop = min(start + c * frame_samples, n_samples)
        last = start + c * frame_samples >= n_samples
        n_k = max(stop - start, 0)
        tp = int(enc_frames_of(n_k)) if n_k > 0 else 0
        lo = 0 if k == 0 else s
        hi = tp if last else c - s
        if not last and hi > tp:
            raise ValueError(f"a full window of {n_k} samples has {tp} encoder frames, fewer than the {hi} the plan keeps")
        if hi > lo:
            shift = n_k / sample_rate / tp      # timestamps_utils.compute_frame_shift(n_k, tp)
            windows.append(Window(start=start, stop=stop, lo=lo, hi=hi, dst=k * step + lo, start_s=start / sample_rate, shift=shift))
        if last:      # (a last window with T' <= lo is dropped: stride 0 and a tail below one analysis window)
            break
        k += 1
    t_total = windows[-1].dst + windows[-1].hi - windows[-1].lo if windows else 0
    return WindowPlan(windows=tuple(windows), t_total=t_total, chunk_frames=c, stride_frames=s, step_frames=step)


def segment_words(words: Sequence, pause_s: float = 1.0, max_segment_s: float = 22.0) -> List[List]:
    """Runs of words (anything with ``start`` / ``end``): a new run starts where a word begins at least ``pause_s`` after the previous
    word's end, or where adding the word would stretch the run past ``max_segment_s``.  Both defaults are conventions."""
    runs: List[List] = []
    for w in words:
        if runs and w.start - runs[-1][-1].end < pause_s and w.end - runs[-1][0].start <= max_segment_s:
            runs[-1].append(w)
        else:
            runs.append([w])
    return runs
