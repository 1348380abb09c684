"""GPU: partial transcripts through the model (``align_batch`` / ``align_longform`` with ``wildcard=``) on a synthetic 2-layer CTC
model: the alignment against the float64 reference of tests/ctc_align_star_ref.py run on the model's own log-probs, the gaps, words
and token ids of a greedy transcript with a span cut out, a gap that runs across two speech regions, and the unchanged results of
calls without the keywords."""
import math
import wave

import numpy as np
import pytest
import torch

import ctc_align_star_ref as RS
from test_hip_ctc_align import _bar

pytestmark = pytest.mark.gpu

LN2 = math.log(2)


@pytest.fixture(scope="module")
def model():
    import gigaam_amd
    from gigaam_amd import synth
    return gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=1, n_layers=2), "cuda:0")


@pytest.fixture(scope="module")
def batch(model):
    """Two utterances, their greedy ids, and the model's own log-probs on the host (what the alignment reads)."""
    from gigaam_amd import synth
    wav, wlen = synth.synth_audio(2, 8.0, seed=31, lengths=[128000, 90000])
    with torch.inference_mode():
        enc, elen = model._encode(wav.to("cuda:0"), wlen.to("cuda:0"), wlen)
        ids = [d[1] for d in model.decoding.decode(model.head, enc, elen)]
        lp = model.head.engine.ctc_head(enc).cpu().numpy()
    return wav, wlen, elen.cpu().tolist(), ids, lp


def _partial(tok, ids):
    """A leading wildcard and the middle third of the greedy ids cut out: (text with "*", the span [a, b))."""
    n = len(ids)
    assert n >= 9, n
    a, b = n // 3, 2 * n // 3
    return "*" + tok.decode(ids[:a]) + "*" + tok.decode(ids[b:]), (a, b)


def test_align_batch_with_wildcards_matches_float64_reference(model, batch):
    from gigaam_amd import wildcard as W
    from gigaam_amd.timestamps_utils import compute_frame_shift
    from gigaam_amd.types import AlignmentResult, Gap
    wav, wlen, elen, ids, lp = batch
    tok, V = model.decoding.tokenizer, model.wildcard_id
    assert V == lp.shape[2]
    texts, spans = zip(*[_partial(tok, i) for i in ids])
    res = model.align_batch(wav, wlen, list(texts), wildcard="*")
    for b, r in enumerate(res):
        a, e = spans[b]
        y = [V] + ids[b][:a] + [V] + ids[b][e:]
        T = elen[b]
        star = RS.star_row(lp[b, :T], LN2)
        score, states = RS.viterbi(lp[b, :T], star, y)
        ll = RS.forward_loglik(lp[b, :T], star, y)
        first, last = RS.token_runs(states, len(y))
        assert isinstance(r, AlignmentResult) and r.feasible
        assert r.token_ids == y and r.text == texts[b]
        print("utterance", b, "score", r.score, "ref", score, "loglik", r.log_likelihood, "ref", ll)
        assert abs(r.score - score) <= _bar(score) and abs(r.log_likelihood - ll) <= _bar(ll)
        assert r.token_frames == first
        shift = compute_frame_shift(int(wlen[b]), T)
        words, gaps = W.short_result(tok, y, first, last, shift, V)
        assert r.words == words and r.gaps == gaps
        assert len(r.gaps) == 2 and all(isinstance(g, Gap) and g.start_frame <= g.end_frame for g in r.gaps)
        assert r.gaps[0].start_frame == first[0] and r.gaps[1].start_frame == first[a + 1] and r.gaps[1].end_frame == last[a + 1]
        assert r.gaps[0].end_frame < r.gaps[1].start_frame
        for w in r.words:                                      # no word spans a gap
            assert all(w.end <= g.start + 1e-9 or w.start >= g.end - 1e-9 for g in r.gaps), (w, r.gaps)
    # the same through token ids and the explicit penalty, without a wildcard string
    res2 = model.align_batch(wav, wlen, [r.token_ids for r in res], wildcard_penalty=LN2)
    for r, r2 in zip(res, res2):
        assert r2.token_frames == r.token_frames and r2.gaps == r.gaps and r2.score == r.score and r2.words == r.words


def test_wildcard_errors_need_no_audio(model, batch):
    wav, wlen, _, ids, _ = batch
    V = model.wildcard_id
    with pytest.raises(ValueError, match="can spell"):
        model.align_batch(wav, wlen, ["а", "б"], wildcard="а")
    with pytest.raises(ValueError, match="non-empty"):
        model.align_batch(wav, wlen, ["а", "б"], wildcard="")
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="wildcard_penalty"):
            model.align_batch(wav, wlen, ["а", "б"], wildcard="*", wildcard_penalty=bad)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        model.align_batch(wav, wlen, [[1, V, 2], [1]])
    with pytest.raises(ValueError):
        model.align_batch(wav, wlen, ["а*б", "б"])             # "*" without wildcard=: a character outside the vocabulary


def test_align_batch_without_the_keywords_is_unchanged(model, batch):
    """Field for field what the path without wildcards gives: gam_ctc_align through ``decoding.align`` and ``frames_to_words``."""
    from gigaam_amd.timestamps_utils import compute_frame_shift, frames_to_words
    from gigaam_amd.types import AlignmentResult
    wav, wlen, elen, ids, _ = batch
    tok = model.decoding.tokenizer
    texts = [tok.decode(ids[0]), ids[1]]
    got = model.align_batch(wav, wlen, texts)
    with torch.inference_mode():
        enc, el = model._encode(wav.to("cuda:0"), wlen.to("cuda:0"), wlen)
        rows = model.decoding.align(model.head, enc, el, ids)
    for b, (i, first, _last, score, loglik, ok) in enumerate(rows):
        words = frames_to_words(tok, i, first, compute_frame_shift(int(wlen[b]), elen[b]))
        want = AlignmentResult(text=tok.decode(i), words=words, token_ids=i, token_frames=first, score=score, log_likelihood=loglik,
                               feasible=ok)
        assert got[b] == want and got[b].gaps == [] and got[b].feasible


def test_rnnt_models_raise_type_error_with_wildcards():
    import gigaam_amd
    from gigaam_amd import synth
    m = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_rnnt", seed=1, n_layers=1), "cuda:0")
    wav, wlen = synth.synth_audio(1, 2.0, seed=3)
    with pytest.raises(TypeError, match="forced alignment needs a CTC head"):
        m.align_batch(wav, wlen, ["а*"], wildcard="*")


def test_align_longform_gap_crosses_the_region_boundary(model, tmp_path):
    from gigaam_amd import synth
    from gigaam_amd.types import Gap, LongformAlignmentResult
    wav, _ = synth.synth_audio(1, 12.0, seed=17)
    pcm = (wav[0].numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16)
    wpath = str(tmp_path / "two_regions.wav")
    with wave.open(wpath, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(16000)
        wf.writeframes(pcm.tobytes())
    kw = dict(speech_regions=[(0.2, 5.6), (6.1, 11.8)], min_duration=2.0, max_duration=7.0)
    lf = model.transcribe_longform(wpath, **kw)
    assert len(lf.segments) == 2
    t0, t1 = lf.segments[0].text, lf.segments[1].text
    assert len(t0) >= 8 and len(t1) >= 8
    # the second half of region 0's text and the first half of region 1's are what the transcript leaves out
    k0, k1 = len(t0) // 2, len(t1) // 2
    text = t0[:k0] + "*" + t1[k1:]
    full = model.align_longform(wpath, t0 + t1, **kw)
    res = model.align_longform(wpath, text, wildcard="*", **kw)
    assert isinstance(res, LongformAlignmentResult) and res.feasible and res.text == text and full.gaps == []
    V = model.wildcard_id
    u = res.token_ids.index(V)
    assert u == k0 and res.token_ids.count(V) == 1 and len(res.token_ids) == k0 + 1 + len(t1) - k1
    (g,) = res.gaps
    print("gap", g, "segments", [(s.start, s.end) for s in res.segments])
    assert isinstance(g, Gap) and g.segment == 0 and g.end_segment == 1 and g.segment != g.end_segment
    assert res.token_segments[u] == 0 and res.token_frames[u] == g.start_frame
    s0, s1 = res.segments[0], res.segments[1]
    assert g.start == round(res.token_times[u], 3) and s0.start <= g.start < s0.end
    # the end by the rule of words, in region 1's own frames: region start + (end_frame + 1) x that region's frame shift
    later = [i for i in range(u + 1, len(res.token_ids)) if res.token_segments[i] == 1 and res.token_frames[i] > 0]
    shift1 = (res.token_times[later[-1]] - s1.start) / res.token_frames[later[-1]]
    assert abs(g.end - (s1.start + (g.end_frame + 1) * shift1)) <= 1.5e-3
    assert s1.start < g.end <= s1.end + 0.05 and g.end <= res.token_times[u + 1] + 1e-3
    for w in res.words:                                        # no word spans the gap
        assert w.end <= g.start + 1e-9 or w.start >= g.end - 1e-9, (w, g)
    assert " ".join(w.text for w in res.words).split() == (t0[:k0] + " " + t1[k1:]).split()
