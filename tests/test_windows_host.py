"""CPU: the window planner of the detector-free longform path (gigaam_amd/windows.py) and its word segmenter.  The planner's table is
what gam_op_ctc_stitch executes: its kept ranges must tile [0, T_total) exactly, never ask a window for more frames than it has, and
give strictly increasing frame times across the seams."""
import math
from collections import namedtuple

import pytest

from gigaam_amd.windows import plan_windows, segment_words

FRAME = 640          # hop 160 x subsampling 4
SR = 16000


def _half_up(n):
    return 0 if n <= 0 else (n + 1) // 2


def _enc_frames_of(center, win=400, hop=160):
    """The host length formula of the library (gam_feat_frames, gam_enc_frames) for one frontend geometry."""
    def f(n):
        feat = n // hop + 1 if center else (0 if n < win else (n - win) // hop + 1)
        return _half_up(_half_up(feat))
    return f


GEOMETRIES = {"center": _enc_frames_of(True), "nocenter_win320": _enc_frames_of(False, win=320)}
CHUNK_S = 4.0                                   # C = 100 frames: small enough to sweep, the arithmetic is the same at 20 s
C = 100
STRIDES = {"zero": 0.0, "one_frame": FRAME / SR, "sixth": None}


def _lengths(step):
    chunk = C * FRAME
    out = [1, 199, 319, chunk - 1, chunk, chunk + 1, 104729]            # below one analysis window ... a prime
    for m in (1, 2, 5):
        out += [m * step * FRAME - 1, m * step * FRAME, m * step * FRAME + 1]
        out += [m * step * FRAME + chunk - 1, m * step * FRAME + chunk, m * step * FRAME + chunk + 1]
    return sorted(set(n for n in out if n > 0))


@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
@pytest.mark.parametrize("stride", sorted(STRIDES))
def test_kept_ranges_tile_the_stream_and_times_increase(geom, stride):
    enc = GEOMETRIES[geom]
    s_frames = {"zero": 0, "one_frame": 1, "sixth": int(math.floor(CHUNK_S / 6 * SR / FRAME))}[stride]
    step = C - 2 * s_frames
    for n in _lengths(step):
        plan = plan_windows(n, FRAME, enc, CHUNK_S, STRIDES[stride], SR)
        assert (plan.chunk_frames, plan.stride_frames, plan.step_frames) == (C, s_frames, step)
        ws = plan.windows
        if not ws:
            assert plan.t_total == 0 and enc(n) == 0, n          # nothing to encode: below one analysis window without centring
            continue
        # the kept ranges tile [0, T_total) with no gap and no overlap, in order
        nxt = 0
        for k, w in enumerate(ws):
            assert w.dst == nxt and w.hi > w.lo >= 0, (n, k)
            assert w.start % (step * FRAME) == 0 and w.stop == min(w.start + C * FRAME, n), (n, k)
            assert w.dst == (w.start // FRAME) + w.lo, (n, k)                  # global index of local frame j: k step + j
            assert w.hi <= enc(w.stop - w.start), (n, k)                       # never more frames than the window has
            assert w.lo == (0 if w.start == 0 else s_frames), (n, k)
            if k + 1 < len(ws):
                assert w.hi == C - s_frames, (n, k)
            assert w.shift == (w.stop - w.start) / SR / enc(w.stop - w.start), (n, k)
            nxt += w.hi - w.lo
        assert plan.t_total == nxt, n
        # the last window is the first whose span reaches the end of the file (a dropped tail window aside)
        assert ws[-1].stop == n or (s_frames == 0 and enc(n - ws[-1].stop) == 0), n
        assert all(w.start + C * FRAME < n for w in ws[:-1]), n
        # frame times strictly increase over the whole stream, seams included
        wins, local, times = plan.locate(range(plan.t_total))
        assert all(b > a for a, b in zip(times, times[1:])), n
        assert wins == sorted(wins) and [local[0], wins[0]] == [0, 0]
        spans = plan.spans()
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and all(b > a for a, b in spans), n
        if n <= C * FRAME:
            # a file no longer than one chunk: one window, nothing dropped, transcribe's own frame shift
            assert len(ws) == 1 and (ws[0].lo, ws[0].hi, ws[0].dst, ws[0].start, ws[0].stop) == (0, enc(n), 0, 0, n), n
            assert ws[0].shift == n / SR / enc(n) and ws[0].start_s == 0.0, n


def test_default_chunk_and_stride_are_the_documented_convention():
    plan = plan_windows(3600 * SR, FRAME, GEOMETRIES["center"])
    assert (plan.chunk_frames, plan.stride_frames, plan.step_frames) == (500, 83, 334)     # 20 s, floor(20 / 6 s), C - 2 S
    assert plan.t_total == GEOMETRIES["center"](3600 * SR - plan.windows[-1].start) + plan.windows[-1].start // FRAME
    with pytest.raises(ValueError):
        plan.locate([plan.t_total])


@pytest.mark.parametrize("chunk, stride", [(20.0, 10.0), (20.0, 12.0), (0.0, None), (-1.0, None), (float("nan"), None),
                                           (float("inf"), None), (20.0, -0.1), (25.1, None), (0.01, 0.0)])
def test_bad_geometry_is_a_value_error(chunk, stride):
    with pytest.raises(ValueError):
        plan_windows(100 * SR, FRAME, GEOMETRIES["center"], chunk, stride)


def test_the_largest_chunk_is_accepted():
    assert plan_windows(100 * SR, FRAME, GEOMETRIES["center"], 25.0).chunk_frames == 625


W = namedtuple("W", "text start end")


def test_segmenter_cuts_at_pauses_and_at_the_length_limit():
    words = [W("a", 0.0, 0.5), W("b", 0.6, 1.0), W("c", 1.999, 2.5),      # 0.999 s pause: same run
             W("d", 3.5, 4.0),                                            # exactly 1.0 s pause: a new run
             W("e", 4.1, 25.5),                                           # 3.5 .. 25.5 = 22.0 s: still fits
             W("f", 25.6, 25.6),                                          # 22.1 s: a new run
             W("g", 25.7, 26.0)]
    runs = segment_words(words, pause_s=1.0, max_segment_s=22.0)
    assert [[w.text for w in r] for r in runs] == [["a", "b", "c"], ["d", "e"], ["f", "g"]]
    assert segment_words([]) == []
    assert [[w.text for w in r] for r in segment_words(words, pause_s=100.0, max_segment_s=1e9)] == [list("abcdefg")]
    assert [len(r) for r in segment_words(words, pause_s=0.0)] == [1] * 7
