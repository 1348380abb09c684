"""GPU: ``transcribe_longform(vad="windows", stream_search=True)`` -- the resumable beam search over the stitched stream -- on a
synthetic 2-layer CTC model.  The expectation is composed as tests/test_hip_longform_windows.py composes its own: the planner's windows
through the same feeder batches, stitched in numpy, searched by ``op_ctc_beam`` as ONE utterance (583 frames: under the batch kernel's
limit) and turned into words and segments by the documented rules.  The same batches give the same log-prob bits and one stream call
equals the batch kernel bit for bit, so every comparison is exact."""
import numpy as np
import pytest
import torch

from beam_common import ctc_hotwords as _hotwords
from test_hip_ctc_align import _wav_file
from test_hip_longform_windows import _as_tuples, _model, _plan, _segments, _stitched, _words

import test_hip_ctc_beam_lm as TL

pytestmark = pytest.mark.gpu

KW = dict(vad="windows", stream_search=True, chunk_length_s=6.0, stride_length_s=1.0, fr_batch_size=2, pause_s=0.3)
W = 4


@pytest.fixture(scope="module")
def v2():
    return _model("v2_ctc")


@pytest.fixture(scope="module")
def long_case(v2, tmp_path_factory):
    """23.3 s, 6 s chunks with 1 s strides, feeder batches of 2: several windows in several batches -> (path, plan, the test's stream)."""
    path = _wav_file(tmp_path_factory.mktemp("beam_windows"), 23.3, 41)
    audio, plan = _plan(v2, path, 6.0, 1.0)
    stream = _stitched(v2, audio, plan, 2)
    assert len(plan.windows) >= 5 and stream.shape[0] == plan.t_total == 583
    return path, plan, stream


def _expect(model, plan, stream, hotwords=(), boost=2.0, lm=None, lm_weight=0.5, word_bonus=1.0):
    """``op_ctc_beam`` on the stream as one utterance -> (words, segments) by the documented rules."""
    eng = model.head.engine
    eng.set_hotwords(list(hotwords), boost)
    eng.set_lm(lm, model.decoding.tokenizer, lm_weight, word_bonus)
    h = eng.op_ctc_beam(torch.from_numpy(stream[None]), torch.tensor([stream.shape[0]], dtype=torch.int32), W).host()
    ids, frames = h["rows"][0]
    assert len(ids) > 20
    words = _words(model, plan, ids, frames)
    return ids, words, _segments(words, pause_s=0.3)


def _check(model, path, want_words, want, **kw):
    res = model.transcribe_longform(path, word_timestamps=True, beam_size=W, **KW, **kw)
    assert _as_tuples(res.words) == want_words
    assert [(s.text, s.start, s.end, _as_tuples(s.words)) for s in res.segments] == want
    plain = model.transcribe_longform(path, beam_size=W, **KW, **kw)
    assert [(s.text, s.start, s.end, s.words) for s in plain.segments] == [(t, a, b, None) for t, a, b, _ in want]


def test_the_stream_search_gives_the_words_of_the_batch_kernel_on_the_stitched_stream(v2, long_case, monkeypatch):
    path, plan, stream = long_case
    _, want_words, want = _expect(v2, plan, stream)
    _check(v2, path, want_words, want)
    # the pushes on the launch stream (the A/B switch) give the same result
    monkeypatch.setenv("GAM_BEAM_STREAM_OVERLAP", "0")
    _check(v2, path, want_words, want)


def test_the_stream_search_with_hotwords(v2, long_case):
    path, plan, stream = long_case
    greedy_ids, _, _ = _expect(v2, plan, stream)
    phrases = _hotwords(np.random.default_rng(5), stream[None], 12)
    ids, want_words, want = _expect(v2, plan, stream, phrases, 3.0)
    _check(v2, path, want_words, want, hotwords=phrases, hotword_boost=3.0)
    # hotwords alone mean a width of 8, as for ``transcribe``
    eng = v2.head.engine
    h = eng.op_ctc_beam(torch.from_numpy(stream[None]), torch.tensor([stream.shape[0]], dtype=torch.int32), 8).host()
    res = v2.transcribe_longform(path, word_timestamps=True, hotwords=phrases, hotword_boost=3.0, **KW)
    assert _as_tuples(res.words) == _words(v2, plan, *h["rows"][0])
    v2.head.engine.set_hotwords([])


def test_the_stream_search_with_an_lm(v2, long_case, tmp_path):
    path, plan, stream = long_case
    tok = v2.decoding.tokenizer
    rng = np.random.default_rng(6)
    lm, _ = TL._make_lm(tmp_path, rng, tok, TL._word_ids(rng, stream[None], TL.token_classes(tok), 60), 3, 0.5, 1.0)
    plain_ids, _, _ = _expect(v2, plan, stream)
    ids, want_words, want = _expect(v2, plan, stream, lm=lm)
    assert ids != plain_ids       # the LM decides something: the route really carries it
    _check(v2, path, want_words, want, lm=lm)
    v2.head.engine.set_lm(None)


def test_a_short_file_gives_the_words_of_transcribe(v2, tmp_path):
    path = _wav_file(tmp_path, 7.0, 17)
    want = v2.transcribe(path, beam_size=W, word_timestamps=True)
    res = v2.transcribe_longform(path, word_timestamps=True, vad="windows", stream_search=True, beam_size=W)
    assert len(want.words) >= 2
    assert _as_tuples(res.words) == [(w.text, round(w.start, 3), round(w.end, 3)) for w in want.words]


def test_what_the_stream_search_route_refuses(v2, tmp_path):
    path = _wav_file(tmp_path, 3.0, 5)
    for kw in (dict(beam_size=4), dict(hotwords=["да"]), dict(lm="missing.arpa")):
        with pytest.raises(ValueError, match="8192"):
            v2.transcribe_longform(path, vad="windows", **kw)
        with pytest.raises(ValueError, match="stream_search"):
            v2.transcribe_longform(path, vad="energy", stream_search=True, **kw)
    with pytest.raises(ValueError, match="stream_search"):
        v2.transcribe_longform(path, stream_search=True, beam_size=4)
    with pytest.raises(ValueError, match="needs beam_size, hotwords or lm"):
        v2.transcribe_longform(path, vad="windows", stream_search=True)
    with pytest.raises(ValueError, match="beam_size"):
        v2.transcribe_longform(path, vad="windows", stream_search=True, beam_size=33)
    rnnt = _model("v2_rnnt")
    with pytest.raises(TypeError, match="windowed longform needs a CTC head"):
        rnnt.transcribe_longform(path, vad="windows", stream_search=True, beam_size=4)
