"""CPU: the carrying reference of the resumable keyword search (tests/kws_stream_ref.py) against the one-shot reference for arbitrary
cuts, the host mapping from frames of the stitched stream to KeywordHits on hand-built window plans, the ``max_hits`` range and
``truncated`` of the windowed route, the refusals that need no GPU, and the ctypes declarations against the header."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from common import ROOT

import kws_inputs as I
import kws_ref as R
import kws_stream_ref as SR
from gigaam_amd import _lib, synth
from gigaam_amd.decoding import keyword_stream_hits, sort_keyword_hits
from gigaam_amd.types import KeywordHit
from gigaam_amd.windows import Window, WindowPlan

NEG = -np.inf


def _cuttings(rng, T):
    fixed = [c for c in (0, 1, 2, 5, 64, 65, 127, 128, 131) if c <= T]
    out = [[], fixed, sorted(fixed + fixed[2:4]), list(range(1, T))]              # one piece; the GPU tests' cuts; 0-frame pieces; 1-frame pieces
    out += [sorted(rng.integers(0, T + 1, int(rng.integers(1, 9))).tolist()) for _ in range(3)]
    return out


@pytest.mark.parametrize("kind", ["peaked", "flat", "dyadic"])
@pytest.mark.parametrize("V,T", [(8, 150), (34, 70), (4, 5)])
def test_carrying_reference_equals_the_one_shot_reference_for_any_cuts(kind, V, T):
    rng = np.random.default_rng(V * 1000 + T + len(kind))
    kws = [I.keyword(rng, U, V, r) for U, r in ((1, 0), (2, 1), (3, 0), (5, 2)) if 2 * U <= T + 1]
    top = I.background(rng, T, V)
    pos = 2
    for y in kws:
        r = I.plant(rng, top, V, y, pos, T)
        if r is not None:
            pos = r[2]
    lp = I.log_probs(rng, 1, T, V, kind, top[None] if kind == "peaked" else None)[0]
    for y in kws:
        E, S = R.dense(lp, y)
        for thr, mh in ((0.5, 64), (0.1, 2)):
            ms = len(y) * math.log(thr)
            hits, n = R.pick(E, S, ms, mh)
            for cuts in _cuttings(rng, T):
                E2, S2, hits2, n2 = SR.run(lp, y, ms, mh, cuts)
                assert np.array_equal(E2, E) and np.array_equal(S2, S), (y, cuts)
                assert hits2 == hits and n2 == n, (y, cuts)


def test_carrying_reference_counts_in_stream_frames():
    rng = np.random.default_rng(5)
    V, T, y = 6, 40, [1, 2]
    lp = I.log_probs(rng, 1, T, V, "dyadic")[0]
    E, S = R.dense(lp, y)
    hits, n = R.pick(E, S, -1.0, 8)
    E2, S2, hits2, n2 = SR.run(lp, y, -1.0, 8, [7, 7, 30], t_base=1000)
    assert np.array_equal(E2, E) and np.array_equal(S2, np.where(S >= 0, S + 1000, -1))
    assert hits2 == [(s + 1000, e + 1000, sc) for s, e, sc in hits] and n2 == n
    state = SR.begin(2)
    state, _, _ = SR.push(state, lp[:0], y, -1.0, [], 8, end=True)               # END on an empty stream: nothing
    assert state["n"] == 0 and state["ended"]


def _plan():
    # C = 100, S = 10, step 80; three windows, the second with a different frame shift (a hand-built plan: only the table matters)
    ws = (Window(start=0, stop=64000, lo=0, hi=90, dst=0, start_s=0.0, shift=0.04),
          Window(start=51200, stop=115200, lo=10, hi=90, dst=90, start_s=3.2, shift=0.05),
          Window(start=102400, stop=150000, lo=10, hi=70, dst=170, start_s=6.4, shift=0.04))
    return WindowPlan(windows=ws, t_total=230, chunk_frames=100, stride_frames=10, step_frames=80)


def _host(n_hits, frames, scores):
    return {"n_hits": np.asarray(n_hits, dtype=np.int32), "hit_frames": np.asarray(frames, dtype=np.int32),
            "hit_score": np.asarray(scores, dtype=np.float32), "status": np.ones(len(n_hits), dtype=np.int32), "flag": False}


def test_stream_frames_become_hits_in_the_windows_they_were_kept_from():
    plan = _plan()
    kws, texts = [[5, 6], [7]], ["аб", "в"]
    # keyword 0: in the first window; across windows 0 / 1; inside window 1.  keyword 1: in the last window (its last frame); 5 found, 3 slots
    h = _host([3, 5], [[[0, 4], [85, 95], [100, 120]], [[229, 229], [91, 91], [170, 171]]],
              [[-0.5, 0.0, -1.0], [0.0, 0.0, -0.25]])
    hits, truncated = keyword_stream_hits(h, kws, texts, plan)
    assert truncated == [1]
    got = [(x.keyword_index, x.segment, x.start_frame, x.end_segment, x.end_frame) for x in hits]
    assert got == [(0, 0, 0, 0, 4), (0, 0, 85, 1, 15), (0, 1, 20, 1, 40), (1, 2, 69, 2, 69), (1, 1, 11, 1, 11), (1, 2, 10, 2, 11)]
    a, b, c, d = hits[0], hits[1], hits[2], hits[3]
    assert isinstance(a, KeywordHit) and a.keyword == "аб"
    assert a.start == 0.0 and a.end == 5 * 0.04 and a.score == -0.5 and a.confidence == pytest.approx(math.exp(-0.25))
    # start in window 0 (shift 0.04), end in window 1 (start 3.2 s, shift 0.05): each time in its own window's terms
    assert b.start == 0.0 + 85 * 0.04 and b.end == 3.2 + 16 * 0.05 and b.segment != b.end_segment and b.confidence == 1.0
    assert c.start == 3.2 + 20 * 0.05 and c.end == 3.2 + 41 * 0.05
    assert d.start == 6.4 + 69 * 0.04 and d.end == 6.4 + 70 * 0.04
    order = sort_keyword_hits(hits)
    assert [x.start for x in order] == sorted(x.start for x in hits)
    # frames outside the stream are the plan's error, not a silent clamp
    with pytest.raises(ValueError, match="outside"):
        keyword_stream_hits(_host([1], [[[0, 230]]], [[0.0]]), [[5]], ["а"], plan)
    assert keyword_stream_hits(_host([0, 0], np.full((2, 3, 2), -1), np.full((2, 3), NEG)), kws, texts, plan) == ([], [])


def test_keyword_hit_keeps_its_field_order_with_end_segment_last():
    x = KeywordHit("а", 0, 0.0, 0.04, 0.0, 1.0, 0, 0, 3)
    assert x.segment == 3 and x.end_segment is None
    assert list(KeywordHit.__dataclass_fields__)[-2:] == ["segment", "end_segment"]


def test_windowed_route_errors_need_no_gpu():
    import gigaam_amd
    ctc = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=1, n_layers=1), "cpu")
    rnnt = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_rnnt", seed=1, n_layers=1), "cpu")
    call = lambda m, kw, **o: m.find_keywords_longform("no-such-file.wav", kw, vad="windows", **o)      # noqa: E731
    with pytest.raises(TypeError, match="keyword search needs a CTC head"):
        call(rnnt, ["да"])
    for mh in (0, 4097, -1):
        with pytest.raises(ValueError, match=r"max_hits=.* outside \[1, 4096\]"):
            call(ctc, ["да"], max_hits=mh)
    with pytest.raises(ValueError, match=r"max_hits=65 outside \[1, 64\]"):           # the speech-region route keeps its own range
        ctc.find_keywords_longform("no-such-file.wav", ["да"], speech_regions=[(0.0, 1.0)], max_hits=65)
    for more in ({"speech_regions": [(0.0, 1.0)]}, {"max_duration": 10.0}):
        with pytest.raises(ValueError, match='vad="windows" takes no segmentation keywords'):
            call(ctc, ["да"], **more)
    for bad, msg in ((["да", "q"], "characters not in the vocabulary"), ([], "empty"), (["а" * 65], "65 tokens")):
        with pytest.raises(ValueError, match=msg):
            call(ctc, bad)
    with pytest.raises(ValueError, match="threshold"):
        call(ctc, ["да"], threshold=0.0)


_CTYPES = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}


@pytest.mark.parametrize("name,ret", [("gam_op_ctc_kws_stream", "int"), ("gam_ctc_kws_state_bytes", "int64_t")])
def test_lib_declares_the_stream_symbols_with_the_headers_signature(name, ret):
    header = open(os.path.join(ROOT, "include", "gigaam_hip.h")).read()
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in the header"
    want = [C.c_void_p if "*" in a else _CTYPES[a.strip().replace("const ", "").split()[0]] for a in m.group(1).split(",")]
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is _CTYPES[ret] and argtypes == want
    from gigaam_amd.engine import HipEngine, KeywordStream
    assert (KeywordStream.BEGIN, KeywordStream.END) == tuple(int(re.search(r"#define GAM_KWS_STREAM_" + f + r"\s+(\d+)", header).group(1))
                                                             for f in ("BEGIN", "END"))
    assert HipEngine.MAX_KEYWORD_STREAM_HITS == 4096
