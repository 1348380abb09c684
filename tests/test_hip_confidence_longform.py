"""GPU: ``GigaAMASR.confidence_longform`` on synthetic two-layer models.  Its words, segments and token fields are pinned to the
existing routes under the same arguments -- ``transcribe_longform(word_timestamps=True)`` without text, ``align_longform`` with text
-- exactly; its token confidences are checked against the float64 reference (tests/confidence_long_ref.py) on the test's OWN
stitched stream (the same feeder batches give the same log-prob bits, so argmaxes and spans are the kernel's), bar
``common.TOL_LOGP``; word, segment and file aggregates follow from the token confidences to 1e-12."""
import numpy as np
import pytest
import torch

from common import TOL_LOGP, report
from confidence_longform_common import DEV, as_tuples, model, plan_of, region_batch, stitched, stream_frames, wav_file

import confidence_long_ref as L
import confidence_ref as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def v2():
    return model("v2_ctc")


@pytest.fixture(scope="module")
def long_case(v2, tmp_path_factory):
    """(b): 23.3 s, 6 s chunks with 1 s strides, feeder batches of 2 -- several windows, several batches."""
    path = wav_file(tmp_path_factory.mktemp("conf_windows"), 23.3, 41)
    audio, plan = plan_of(v2, path, 6.0, 1.0)
    assert len(plan.windows) >= 5
    return path, plan, stitched(v2, audio, plan, 2), dict(vad="windows", chunk_length_s=6.0, stride_length_s=1.0, fr_batch_size=2, pause_s=0.3)


def _same_words(res, base_words, base_segments):
    assert as_tuples(res.words) == as_tuples(base_words)
    assert [(s.text, s.start, s.end, as_tuples(s.words)) for s in res.segments] == \
        [(s.text, s.start, s.end, as_tuples(s.words)) for s in base_segments]


def _check_scores(m, res, plan, stream, measure, agg, wid, what):
    """Token confidences against float64 on ``stream``; words, segments and the file from the token confidences."""
    frames = stream_frames(plan, res.token_segments, res.token_frames)
    assert res.token_times == plan.locate(frames)[2]
    conf, _, ok = L.ctc_confidence_long(stream, res.token_ids, frames, measure, agg, wildcard=wid is not None)
    assert ok == 1 and len(res.token_confidence) == len(res.token_ids)
    stars = [k for k, i in enumerate(res.token_ids) if i == wid]
    assert [k for k, c in enumerate(res.token_confidence) if c is None] == stars
    err = max([abs(c - r) for c, r in zip(res.token_confidence, conf) if c is not None] + [0.0])
    print(f"confidence_longform {what} {measure}/{agg}: {len(conf)} tokens, worst |conf - ref| = {err:.3e}")
    report(f"ctc_confidence_longform_{what}", measure=measure, agg=agg, err=err)
    assert err <= TOL_LOGP, (what, err)
    tok = m.decoding.tokenizer
    tc = res.token_confidence
    groups, a = [], 0
    for b in stars + [len(tc)]:
        groups += [[a + k for k in g] for g in C.word_groups(tok, res.token_ids[a:b])]
        a = b + 1
    assert len(groups) == len(res.words)
    for w, g in zip(res.words, groups):
        assert w.confidence == pytest.approx(C.aggregate([tc[k] for k in g], agg), abs=1e-12)
    pos = {id(w): k for k, w in enumerate(res.words)}
    for sg in res.segments:
        want = C.aggregate([tc[t] for w in sg.words for t in groups[pos[id(w)]]], agg)
        assert (sg.confidence is None) == (want is None) and (want is None or sg.confidence == pytest.approx(want, abs=1e-12))
    want = C.aggregate([c for c in tc if c is not None], agg)
    assert (res.confidence is None) == (want is None) and (want is None or res.confidence == pytest.approx(want, abs=1e-12))
    assert all(c is None or 0.0 <= c <= 1.0 for c in tc)


def test_a_one_chunk_file_gives_the_numbers_of_confidence(v2, tmp_path):
    path = wav_file(tmp_path, 7.0, 17)
    for measure, agg in (("prob", "mean"), ("entropy", "min")):
        want = v2.confidence(path, measure=measure, aggregation=agg)
        res = v2.confidence_longform(path, vad="windows", measure=measure, aggregation=agg)
        assert len(want.words) >= 2 and res.token_ids == want.token_ids and res.token_frames == want.token_frames
        assert res.token_segments == [0] * len(want.token_ids)
        assert as_tuples(res.words) == [(w.text, round(w.start, 3), round(w.end, 3)) for w in want.words]
        assert res.token_confidence == pytest.approx(want.token_confidence, abs=TOL_LOGP)
        assert [w.confidence for w in res.words] == pytest.approx([w.confidence for w in want.words], abs=TOL_LOGP)
        assert res.confidence == pytest.approx(want.confidence, abs=TOL_LOGP)
        assert res.score is None and res.log_likelihood is None and res.gaps == []


@pytest.mark.parametrize("source", ["greedy", "beam", "text"])
def test_several_windows_every_token_source(v2, long_case, source):
    path, plan, stream, kw = long_case
    measure, agg = {"greedy": ("prob", "mean"), "beam": ("entropy", "min"), "text": ("prob", "prod")}[source]
    if source == "text":
        ids = C.ctc_greedy(stream, stream.shape[0])[0]
        akw = {k: v for k, v in kw.items() if k != "pause_s"}
        base = v2.align_longform(path, ids, **akw)
        res = v2.confidence_longform(path, ids, measure=measure, aggregation=agg, **akw)
        assert (res.score, res.log_likelihood, res.gaps) == (base.score, base.log_likelihood, [])
        assert (res.token_ids, res.token_segments, res.token_frames, res.token_times) == \
            (base.token_ids, base.token_segments, base.token_frames, base.token_times)
        _same_words(res, base.words, base.segments)
    else:
        more = dict(stream_search=True, beam_size=4) if source == "beam" else {}
        base = v2.transcribe_longform(path, word_timestamps=True, **kw, **more)
        res = v2.confidence_longform(path, measure=measure, aggregation=agg, **kw, **more)
        assert len(base.segments) >= 1 and res.text == base.text
        _same_words(res, base.words, base.segments)
        if source == "greedy":
            g_ids, g_frames = C.ctc_greedy(stream, stream.shape[0])
            assert res.token_ids == g_ids and stream_frames(plan, res.token_segments, res.token_frames) == g_frames
            assert set(res.token_segments) == set(range(len(plan.windows)))      # the seams are really crossed
        assert res.score is None and res.log_likelihood is None
    assert len(res.token_ids) > 20
    _check_scores(v2, res, plan, stream, measure, agg, None, source)


def test_wildcards_inner_and_leading(v2, long_case):
    path, plan, stream, kw = long_case
    akw = {k: v for k, v in kw.items() if k != "pause_s"}
    ids = C.ctc_greedy(stream, stream.shape[0])[0]
    wid = v2.wildcard_id
    a, b = len(ids) // 3, 2 * len(ids) // 3
    for what, part in (("inner", ids[:a] + [wid] + ids[b:]), ("leading", [wid] + ids[a:])):
        base = v2.align_longform(path, part, wildcard="*", **akw)
        res = v2.confidence_longform(path, part, wildcard="*", measure="prob", aggregation="mean", **akw)
        assert res.token_ids == part and res.gaps == base.gaps and len(res.gaps) == 1
        assert (res.token_segments, res.token_frames, res.token_times, res.score, res.log_likelihood, res.text) == \
            (base.token_segments, base.token_frames, base.token_times, base.score, base.log_likelihood, base.text)
        _same_words(res, base.words, base.segments)
        k = part.index(wid)
        assert res.token_confidence[k] is None and sum(c is None for c in res.token_confidence) == 1
        gap = res.gaps[0]                       # no word spans the gap
        assert all(w.end <= gap.start + 2e-3 or w.start >= gap.end - 2e-3 for w in res.words)      # (times are rounded to 1e-3)
        _check_scores(v2, res, plan, stream, "prob", "mean", wid, f"wildcard_{what}")
    # the same as a string with the wildcard in it
    text = v2.decoding.tokenizer.decode(ids[a:])
    res = v2.confidence_longform(path, "*" + text, wildcard="*", **akw)
    base = v2.align_longform(path, "*" + text, wildcard="*", **akw)
    assert res.text == base.text and res.token_ids == base.token_ids and res.token_confidence[0] is None
    _same_words(res, base.words, base.segments)


def test_past_the_old_limit_of_8192_frames(v2, tmp_path):
    """(d): 340 s on the windows route with its defaults -- T_total > 8192, which no confidence call could take before."""
    path = wav_file(tmp_path, 340.0, 9)
    audio, plan = plan_of(v2, path, 20.0, None)
    assert plan.t_total > 8192
    stream = stitched(v2, audio, plan, 16)
    base = v2.transcribe_longform(path, word_timestamps=True, vad="windows")
    res = v2.confidence_longform(path, vad="windows")
    _same_words(res, base.words, base.segments)
    g_ids, g_frames = C.ctc_greedy(stream, stream.shape[0])
    assert res.token_ids == g_ids and stream_frames(plan, res.token_segments, res.token_frames) == g_frames
    assert max(g_frames) > 8192 and len(g_ids) > 100
    _check_scores(v2, res, plan, stream, "prob", "mean", None, "340s")


REGIONS = dict(speech_regions=[(0.2, 5.6), (6.1, 11.8), (12.0, 15.5)], min_duration=2.0, max_duration=7.0)
# RNN-T: chunks of at most 3 s = 75 frames -- a random transducer emits max_symbols_per_step = 10 tokens at every frame, and the RNN-T
# confidence pass (as the alignment) takes at most 1024 tokens per utterance
SHORT_REGIONS = dict(speech_regions=[(0.2, 2.6), (3.0, 5.8), (6.0, 7.9)], min_duration=1.0, max_duration=3.0)


@pytest.mark.parametrize("name", ["v2_ctc", "v2_rnnt"])
def test_speech_regions_equal_confidence_batch_per_chunk(name, v2, tmp_path):
    m = v2 if name == "v2_ctc" else model(name)
    regions, seconds = (REGIONS, 16.0) if name == "v2_ctc" else (SHORT_REGIONS, 8.0)
    path = wav_file(tmp_path, seconds, 23)
    from gigaam_amd.timestamps_utils import compute_frame_shift
    eng = m.head.engine
    wav, lens, boundaries = region_batch(m, path, **regions)
    assert len(boundaries) >= 2
    for measure, agg in (("prob", "mean"), ("entropy", "prod")):
        want = m.confidence_batch(wav, lens, measure=measure, aggregation=agg)
        assert all(r.feasible and len(r.token_ids) <= 1024 for r in want)
        base = m.transcribe_longform(path, word_timestamps=True, **regions)
        res = m.confidence_longform(path, measure=measure, aggregation=agg, **regions)
        _same_words(res, base.words, base.segments)
        assert res.text == base.text and len(res.segments) == len(want) and sum(len(r.token_ids) for r in want) > 10
        o = 0
        for k, (r, sg, (start, end)) in enumerate(zip(want, res.segments, boundaries)):
            n = len(r.token_ids)
            assert res.token_ids[o:o + n] == r.token_ids and res.token_frames[o:o + n] == r.token_frames
            assert res.token_segments[o:o + n] == [k] * n
            assert res.token_confidence[o:o + n] == r.token_confidence
            assert [w.confidence for w in sg.words] == [w.confidence for w in r.words]
            assert [(w.text, w.start, w.end) for w in sg.words] == [(w.text, round(w.start + start, 3), round(w.end + start, 3)) for w in r.words]
            assert (sg.start, sg.end, sg.text) == (start, end, r.text)
            want_seg = C.aggregate([r.token_confidence[t] for g in C.word_groups(m.decoding.tokenizer, r.token_ids) for t in g], agg)
            assert (sg.confidence is None) == (want_seg is None) and (want_seg is None or sg.confidence == pytest.approx(want_seg, abs=1e-12))
            o += n
        assert o == len(res.token_ids)
        assert res.confidence == pytest.approx(C.aggregate(res.token_confidence, agg), abs=1e-12)
        shifts = [compute_frame_shift(int(n), eng.enc_frames(eng.feat_frames(int(n)))) for n in lens.tolist()]
        assert res.token_times == [boundaries[k][0] + f * shifts[k] for k, f in zip(res.token_segments, res.token_frames)]
    if name == "v2_ctc":          # beam search chunk by chunk: the tokens of transcribe_longform(beam_size=), the numbers of confidence_batch
        want = m.confidence_batch(wav, lens, beam_size=4)
        base = m.transcribe_longform(path, word_timestamps=True, beam_size=4, **regions)
        res = m.confidence_longform(path, beam_size=4, **regions)
        _same_words(res, base.words, base.segments)
        assert res.token_ids == [i for r in want for i in r.token_ids] and res.token_frames == [f for r in want for f in r.token_frames]
        assert res.token_confidence == [c for r in want for c in r.token_confidence]
        assert [w.confidence for w in res.words] == [w.confidence for r in want for w in r.words]
        want = m.confidence_batch(wav, lens)
    if name == "v2_ctc":          # with a text: align_longform's result, scored on the concatenated region stream
        ids = [i for r in want for i in r.token_ids]
        base = m.align_longform(path, ids, **regions)
        res = m.confidence_longform(path, ids, **regions)
        assert (res.token_ids, res.token_segments, res.token_frames, res.token_times, res.score, res.log_likelihood) == \
            (base.token_ids, base.token_segments, base.token_frames, base.token_times, base.score, base.log_likelihood)
        _same_words(res, base.words, base.segments)
        assert all(c is not None and 0.0 <= c <= 1.0 for c in res.token_confidence)
        # the numbers: float64 on the test's own concatenated region stream (the same batch gives the same log-prob bits)
        with torch.inference_mode():
            enc, elen = m._encode_batch(wav, lens)
            lp, elen = eng.ctc_head(enc).cpu().numpy(), elen.cpu().tolist()
        stream = np.concatenate([lp[b, :elen[b]] for b in range(len(elen))])
        offs = np.cumsum([0] + elen).tolist()
        res2 = m.confidence_longform(path, ids, measure="entropy", aggregation="prod", **regions)
        frames = [offs[k] + f for k, f in zip(res2.token_segments, res2.token_frames)]
        conf, _, ok = L.ctc_confidence_long(stream, ids, frames, "entropy", "prod")
        err = float(np.abs(np.asarray(res2.token_confidence) - np.asarray(conf)).max())
        print(f"confidence_longform regions with text: worst |conf - ref| = {err:.3e}")
        report("ctc_confidence_longform_regions_text", err=err)
        assert ok == 1 and err <= TOL_LOGP
        assert res2.confidence == pytest.approx(C.aggregate(res2.token_confidence, "prod"), abs=1e-12)


def test_errors(v2, tmp_path):
    from gigaam_amd._lib import GigaAMHipError
    path = wav_file(tmp_path, 3.0, 5)
    missing = str(tmp_path / "no-such-file.wav")
    # unknown codes: before any audio is read
    with pytest.raises(ValueError, match="unknown confidence measure"):
        v2.confidence_longform(missing, vad="windows", measure="margin")
    with pytest.raises(ValueError, match="unknown confidence aggregation"):
        v2.confidence_longform(missing, speech_regions=[(0.0, 1.0)], aggregation="max")
    # beam options together with a text
    for kw in (dict(beam_size=4), dict(hotwords=["да"]), dict(lm="missing.arpa"), dict(stream_search=True)):
        with pytest.raises(ValueError, match="cannot be combined with a given text"):
            v2.confidence_longform(path, "да", vad="windows", **kw)
    # the windows route's refusals, as transcribe_longform's
    for kw in (dict(beam_size=4), dict(hotwords=["да"]), dict(lm="missing.arpa")):
        with pytest.raises(ValueError, match="8192"):
            v2.confidence_longform(path, vad="windows", **kw)
    with pytest.raises(ValueError, match="needs beam_size, hotwords or lm"):
        v2.confidence_longform(path, vad="windows", stream_search=True)
    with pytest.raises(ValueError, match="stream_search=True searches the stitched stream"):
        v2.confidence_longform(path, stream_search=True, beam_size=4, speech_regions=[(0.0, 1.0)])
    with pytest.raises(ValueError, match="speech_regions"):
        v2.confidence_longform(path, vad="windows", speech_regions=[(0.0, 1.0)])
    with pytest.raises(ValueError, match="speech_regions"):
        v2.confidence_longform(path, "да", vad="windows", speech_regions=[(0.0, 1.0)])
    with pytest.raises(ValueError):
        v2.confidence_longform(path, vad="windows", chunk_length_s=30.0)
    with pytest.raises(ValueError, match="belong to a given text"):
        v2.confidence_longform(path, vad="windows", wildcard="*")
    # align_longform's own errors, with text
    with pytest.raises(ValueError, match="cannot be aligned"):
        v2.confidence_longform(path, [1, 2] * 200, vad="windows")
    with pytest.raises(ValueError, match="can spell"):
        v2.confidence_longform(path, "да", vad="windows", wildcard="а")
    with pytest.raises(ValueError):
        v2.confidence_longform(path, [v2.wildcard_id, 1], vad="windows")
    # RNN-T models
    rnnt = model("v2_rnnt")
    with pytest.raises(TypeError, match="windowed longform needs a CTC head"):
        rnnt.confidence_longform(path, vad="windows")
    with pytest.raises(TypeError, match="windowed longform needs a CTC head"):
        rnnt.confidence_longform(path, [1, 2], vad="windows")
    with pytest.raises(TypeError, match="no long transducer alignment"):
        rnnt.confidence_longform(path, [1, 2], speech_regions=[(0.0, 2.0)])
    with pytest.raises(TypeError, match="beam search needs a CTC head"):
        rnnt.confidence_longform(path, beam_size=4, speech_regions=[(0.0, 2.0)])
    # status 0 from the pass is an error of its own
    eng = v2.head.engine
    lp = torch.log_softmax(torch.randn(50, eng.cfg.num_classes), dim=-1).to(DEV)
    with pytest.raises(GigaAMHipError, match="rejected"):
        v2._confidence_host(eng.op_ctc_confidence_long(lp, [1, 2], [7, 7]), 2)
