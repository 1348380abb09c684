"""GPU: ``find_keywords_longform(vad="windows")`` -- keyword search over the stitched stream of a recording -- on the synthetic 2-layer
CTC model.  The expectation is composed here: the windows go through the same feeder batches and are stitched in numpy
(test_hip_longform_windows._stitched), the batch kernel (``op_ctc_kws``, T' < 8192) searches that stream as an independent oracle, and
``plan.locate`` maps its frames.  The same batches give the same log-prob bits, so every comparison is exact."""
import dataclasses
import math
import warnings

import pytest
import torch

from ctc_greedy_long_ref import greedy_ref
from test_hip_ctc_align import _wav_file
from test_hip_longform_windows import _model, _plan, _stitched, _words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def v2():
    return _model("v2_ctc")


def _expected(model, plan, stream, keywords, threshold, max_hits):
    """KeywordHits of ``op_ctc_kws`` on the stitched stream, mapped by the documented rules, in the result's order."""
    from gigaam_amd.decoding import keyword_min_scores
    from gigaam_amd.types import KeywordHit
    eng, tok = model.head.engine, model.decoding.tokenizer
    ids = model.decoding.keyword_ids(keywords)
    texts = [w if isinstance(w, str) else tok.decode(i) for w, i in zip(keywords, ids)]
    eng.set_keywords(ids, keyword_min_scores([len(i) for i in ids], threshold))
    h = eng.op_ctc_kws(torch.from_numpy(stream[None]), torch.tensor([stream.shape[0]], dtype=torch.int32), max_hits).host()
    hits, truncated = [], []
    for k, y in enumerate(ids):
        n = int(h["n_hits"][0, k])
        if n > max_hits:
            truncated.append(k)
        for r in range(min(n, max_hits)):
            s, e, sc = int(h["hit_frames"][0, k, r, 0]), int(h["hit_frames"][0, k, r, 1]), float(h["hit_score"][0, k, r])
            (w0, w1), (j0, j1), _ = plan.locate([s, e])
            a, b = plan.windows[w0], plan.windows[w1]
            assert a.lo <= j0 < a.hi and b.lo <= j1 < b.hi
            hits.append(KeywordHit(keyword=texts[k], keyword_index=k, start=a.start_s + j0 * a.shift, end=b.start_s + (j1 + 1) * b.shift,
                                   score=sc, confidence=math.exp(sc / len(y)), start_frame=j0, end_frame=j1, segment=w0, end_segment=w1))
    return sorted(hits, key=lambda x: (x.start, x.keyword_index, x.end)), truncated, texts


def test_several_windows_in_several_batches_match_the_batch_kernel_on_the_stitched_stream(v2, tmp_path, monkeypatch):
    path = _wav_file(tmp_path, 50.0, 41)
    audio, plan = _plan(v2, path, 20.0, None)
    assert len(plan.windows) >= 4 and 1000 < plan.t_total < 8192
    stream = _stitched(v2, audio, plan, 2)
    ids, frames = greedy_ref(stream)
    assert len(ids) > 40
    # (the synthetic model's "words" run to hundreds of tokens: a keyword is the first eight characters of one)
    words = [w[:8] for w, _, _ in _words(v2, plan, ids, frames) if len(w) >= 2]
    assert len(words) >= 3
    # a stretch of the greedy ids whose frames lie on both sides of the seam between windows 1 and 2
    seam = plan.windows[2].dst
    i0 = max(i for i, f in enumerate(frames) if f < seam)
    stretch = ids[i0 - 2:i0 + 3]
    assert len(stretch) == 5 and frames[i0 - 2] < seam <= frames[i0 + 2]
    keywords = [words[0], words[len(words) // 2], words[-1], stretch]
    kw = dict(vad="windows", chunk_length_s=20.0, fr_batch_size=2)
    for thr, mh in ((0.5, 64), (0.05, 2)):
        want, truncated, texts = _expected(v2, plan, stream, keywords, thr, mh)
        res = v2.find_keywords_longform(path, keywords, threshold=thr, max_hits=mh, **kw)
        assert res.keywords == texts and res.truncated == truncated
        assert res.hits == want
        assert all(x.start < x.end for x in res.hits)
    res = v2.find_keywords_longform(path, keywords, max_hits=64, **kw)
    assert {x.keyword_index for x in res.hits} == {0, 1, 2, 3}
    across = [x for x in res.hits if x.keyword_index == 3 and x.score == 0.0 and x.segment != x.end_segment]
    assert across and across[0].segment < across[0].end_segment == 2
    # the A/B switch: the same calls on the launch stream
    monkeypatch.setenv("GAM_KWS_STREAM_OVERLAP", "0")
    assert v2.find_keywords_longform(path, keywords, max_hits=64, **kw).hits == res.hits
    monkeypatch.delenv("GAM_KWS_STREAM_OVERLAP")
    # per-file hit slots beyond the batch kernel's 64
    many = v2.find_keywords_longform(path, [[ids[0]]], threshold=0.01, max_hits=4096, **kw)
    few = v2.find_keywords_longform(path, [[ids[0]]], threshold=0.01, max_hits=3, **kw)
    assert len(many.hits) > 3 and many.truncated == [] and few.truncated == [0] and few.hits == many.hits[:3]


def test_a_short_file_gives_the_hits_of_find_keywords(v2, tmp_path):
    path = _wav_file(tmp_path, 10.0, 17)
    text = v2.transcribe(path).text
    words = [w[:6] for w in text.split() if len(w) >= 2]
    keywords = [words[0], words[-1][-4:], text[:3]]
    want = v2.find_keywords(path, keywords, threshold=0.3)
    got = v2.find_keywords_longform(path, keywords, threshold=0.3, vad="windows")
    assert len(want.hits) >= 2 and got.keywords == want.keywords and got.truncated == want.truncated
    assert all((x.segment, x.end_segment) == (0, 0) for x in got.hits)
    assert [dataclasses.replace(x, segment=None, end_segment=None) for x in got.hits] == want.hits


def test_what_the_windowed_keyword_route_refuses(v2, tmp_path):
    path = _wav_file(tmp_path, 3.0, 5)
    with pytest.raises(ValueError, match="speech_regions"):
        v2.find_keywords_longform(path, ["да"], vad="windows", speech_regions=[(0.0, 1.0)])
    for mh in (0, 4097):
        with pytest.raises(ValueError, match="max_hits"):
            v2.find_keywords_longform(path, ["да"], vad="windows", max_hits=mh)
    with pytest.raises(ValueError, match="chunk_length_s"):
        v2.find_keywords_longform(path, ["да"], vad="windows", chunk_length_s=30.0)
    with pytest.raises(ValueError, match="leaves no step"):
        v2.find_keywords_longform(path, ["да"], vad="windows", chunk_length_s=6.0, stride_length_s=3.0)
    with pytest.raises(TypeError, match="keyword search needs a CTC head"):
        _model("v2_rnnt").find_keywords_longform(path, ["да"], vad="windows")


def test_without_windows_the_speech_region_route_runs_as_before(v2, tmp_path):
    path = _wav_file(tmp_path, 31.0, 23)
    keywords = [w for w in v2.transcribe_longform(path, vad="energy").segments[0].text.split() if len(w) >= 2][:3]
    keywords = [w[:6] for w in keywords]
    assert keywords
    explicit = v2.find_keywords_longform(path, keywords, vad="energy")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (without pyannote the default says that it uses the stand-in)
        default = v2.find_keywords_longform(path, keywords)
        resolved = {}
        v2._default_vad(resolved, "find_keywords_longform")      # what the default resolves to here: pyannote (nothing added) or the stand-in
    same = v2.find_keywords_longform(path, keywords, **resolved)
    assert default.hits == same.hits and default.truncated == same.truncated and default.keywords == same.keywords
    if "vad" in resolved:                                        # the stand-in: the route that ``vad="energy"`` names
        assert default.hits == explicit.hits and default.truncated == explicit.truncated
    assert len(explicit.hits) >= 1 and all(x.end_segment is None and x.segment is not None for x in explicit.hits)
    with pytest.raises(ValueError, match="max_hits"):                  # this route keeps 1..64 per region
        v2.find_keywords_longform(path, keywords, vad="energy", max_hits=65)
    with pytest.raises(TypeError, match="chunk_length_s"):             # the windows' keywords still go to the chunk packer here
        v2.find_keywords_longform(path, keywords, vad="energy", chunk_length_s=20.0)
