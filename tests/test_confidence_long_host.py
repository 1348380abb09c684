"""CPU: the float64 reference of the long confidence pass (tests/confidence_long_ref.py) on hand-made cases -- the wildcard rule
above all -- and the host assembly of ``confidence_longform``'s result (``timestamps_utils.score_longform``): scored words and
segments from made-up token lists, char-wise and SentencePiece-style, None at the wildcards, aggregates to 1e-12.  No GPU."""
import numpy as np
import pytest

import confidence_long_ref as L
import confidence_ref as C

AGGS = ["mean", "min", "prod"]


def _rows(*rows):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(rows, dtype=np.float64)).astype(np.float32)


# V = 4 (blank = 3, wildcard id = 4): the argmaxes of the eight frames are 0 0 0 1 1 3 2 2
LP = _rows([0.7, 0.1, 0.1, 0.1], [0.6, 0.2, 0.1, 0.1], [0.5, 0.2, 0.2, 0.1], [0.1, 0.8, 0.05, 0.05], [0.2, 0.6, 0.1, 0.1],
           [0.1, 0.1, 0.1, 0.7], [0.1, 0.1, 0.7, 0.1], [0.05, 0.05, 0.8, 0.1])


def test_without_wildcards_it_is_the_clip_reference():
    ids, frames = [0, 1, 2], [0, 3, 6]
    for measure in C.MEASURES:
        for agg in AGGS:
            assert L.ctc_confidence_long(LP, ids, frames, measure, agg) == C.ctc_confidence(LP, 8, ids, frames, measure, agg)
            assert L.ctc_confidence_long(LP, ids, frames, measure, agg, wildcard=True) == C.ctc_confidence(LP, 8, ids, frames, measure, agg)
    conf, span, ok = L.ctc_confidence_long(LP, ids, frames, "prob", "mean")
    assert ok == 1 and span == [3, 2, 2]
    assert conf == pytest.approx([(0.7 + 0.6 + 0.5) / 3, 0.7, 0.75], abs=1e-7)


def test_a_wildcard_bounds_its_neighbours_span():
    # token 0 runs over frames 0..2 by argmax; a wildcard at frame 2 cuts the run to 0..1
    conf, span, ok = L.ctc_confidence_long(LP, [0, 4, 1], [0, 2, 3], "prob", "mean", wildcard=True)
    assert ok == 1 and span == [2, 0, 2] and conf[1] == -1.0
    assert conf[0] == pytest.approx(0.65, abs=1e-7) and conf[2] == pytest.approx(0.7, abs=1e-7)
    conf, span, ok = L.ctc_confidence_long(LP, [0, 4, 1], [0, 2, 3], "prob", "min", wildcard=True)
    assert conf[0] == pytest.approx(0.6, abs=1e-7)
    # the wildcard's frame takes part in the increasing check
    assert L.ctc_confidence_long(LP, [0, 4, 1], [0, 3, 3], wildcard=True) == ([-1.0] * 3, [0] * 3, 0)
    assert L.ctc_confidence_long(LP, [0, 4, 1], [2, 1, 3], wildcard=True)[2] == 0
    assert L.ctc_confidence_long(LP, [0, 4], [0, 8], wildcard=True)[2] == 0
    # without the switch id V is invalid
    assert L.ctc_confidence_long(LP, [0, 4, 1], [0, 2, 3]) == ([-1.0] * 3, [0] * 3, 0)


def test_a_wildcard_first_and_last():
    conf, span, ok = L.ctc_confidence_long(LP, [4, 1, 4], [0, 3, 4], "prob", "prod", wildcard=True)
    assert ok == 1 and span == [0, 1, 0] and conf[0] == -1.0 and conf[2] == -1.0
    assert conf[1] == pytest.approx(0.8, abs=1e-7)          # (frame 4 is the last wildcard's: the run stops before it)
    conf, span, ok = L.ctc_confidence_long(LP, [4], [5], "entropy", "mean", wildcard=True)
    assert (conf, span, ok) == ([-1.0], [0], 1)
    assert L.ctc_confidence_long(LP, [], [], wildcard=True) == ([], [], 1)


def test_an_invalid_list_is_all_minus_one():
    for ids, frames in (([0, 1, 3], [0, 3, 6]), ([0, 1, 5], [0, 3, 6]), ([0, -1, 2], [0, 3, 6]), ([0, 1, 2], [0, 3, 8]),
                        ([0, 1, 2], [0, 3, 3]), ([0, 1, 2], [-1, 3, 6])):
        for wildcard in (False, True):
            assert L.ctc_confidence_long(LP, ids, frames, wildcard=wildcard) == ([-1.0] * 3, [0] * 3, 0), (ids, frames)
    assert L.ctc_confidence_long(LP, [0, 1, 2], [0, 3, 6], cap=2)[2] == 0


class _Pieces:
    """A SentencePiece-style tokenizer as far as the word rules read one: ``id_to_str``."""
    charwise = False

    def __init__(self, pieces):
        self.pieces = list(pieces)

    def __len__(self):
        return len(self.pieces)

    def id_to_str(self, i):
        return self.pieces[int(i)]


def _check_scored(tok, ids, conf, words, segments, agg, wid):
    from gigaam_amd.timestamps_utils import score_longform
    from gigaam_amd.types import ScoredSegment, ScoredWord
    token_conf, scored, segs, total = score_longform(tok, ids, conf, words, segments, agg, wid)
    assert token_conf == [None if i == wid else float(c) for i, c in zip(ids, conf)]
    # the reference's word groups, run by run between the wildcards
    groups, a = [], 0
    for b in [k for k, i in enumerate(ids) if i == wid] + [len(ids)]:
        groups += [[a + k for k in g] for g in C.word_groups(tok, ids[a:b])]
        a = b + 1
    assert len(scored) == len(words) == len(groups)
    for w, s, g in zip(words, scored, groups):
        assert isinstance(s, ScoredWord) and (s.text, s.start, s.end) == (w.text, w.start, w.end)
        assert all(ids[k] != wid for k in g)
        assert s.confidence == pytest.approx(C.aggregate([conf[k] for k in g], agg), abs=1e-12)
    assert len(segs) == len(segments)
    pos = {id(w): k for k, w in enumerate(words)}
    for sg, ss in zip(segments, segs):
        assert isinstance(ss, ScoredSegment) and (ss.text, ss.start, ss.end) == (sg.text, sg.start, sg.end)
        ks = [pos[id(w)] for w in sg.words]
        assert ss.words == [scored[k] for k in ks]
        want = C.aggregate([conf[t] for k in ks for t in groups[k]], agg)
        assert (ss.confidence is None) == (want is None)
        if want is not None:
            assert ss.confidence == pytest.approx(want, abs=1e-12)
    want = C.aggregate([c for i, c in zip(ids, conf) if i != wid], agg)
    assert (total is None) == (want is None)
    if want is not None:
        assert total == pytest.approx(want, abs=1e-12)
    return token_conf, scored, segs, total


@pytest.mark.parametrize("agg", AGGS)
def test_scored_words_and_segments_charwise(agg):
    from gigaam_amd import synth
    from gigaam_amd.decoding import Tokenizer
    from gigaam_amd.timestamps_utils import longform_words
    from gigaam_amd.wildcard import longform_result
    tok = Tokenizer(synth.CHAR_VOCAB)
    wid = len(tok) + 1
    rng = np.random.default_rng(3)
    # no wildcard: three regions, words from longform_words
    ids = tok.encode("да нет  кот да")
    frames = list(range(0, 3 * len(ids), 3))
    segs_of = [0] * 5 + [1] * 5 + [2] * (len(ids) - 10)
    bounds, shifts = [(0.0, 1.0), (2.0, 3.0), (5.0, 6.5)], [0.04, 0.04, 0.05]
    words, segments = longform_words(tok, ids, segs_of, frames, bounds, shifts)
    conf = rng.uniform(0.1, 1.0, len(ids)).tolist()
    _, scored, segs, total = _check_scored(tok, ids, conf, words, segments, agg, wid)
    assert [w.text for w in scored] == ["да", "нет", "кот", "да"]
    assert total == pytest.approx(C.aggregate(conf, agg), abs=1e-12)          # the separators count for the file, for no word
    # wildcards: leading, inner (cutting what would be one word in two) and trailing
    ids = [wid] + tok.encode("да не") + [wid] + tok.encode("т кот") + [wid]
    frames = list(range(0, 2 * len(ids), 2))
    segs_of = [0 if f < 12 else 1 for f in frames]
    words, segments, gaps = longform_result(tok, ids, segs_of, frames, segs_of, [f + 1 for f in frames], bounds[:2], shifts[:2], wid)
    conf = rng.uniform(0.1, 1.0, len(ids)).tolist()
    token_conf, scored, segs, total = _check_scored(tok, ids, conf, words, segments, agg, wid)
    assert [w.text for w in scored] == ["да", "не", "т", "кот"] and len(gaps) == 3
    assert [k for k, c in enumerate(token_conf) if c is None] == [0, 6, len(ids) - 1]
    # nothing at all, and wildcards only
    assert _check_scored(tok, [], [], [], [], agg, wid) == ([], [], [], None)
    assert _check_scored(tok, [wid], [-1.0], [], [], agg, wid) == ([None], [], [], None)


@pytest.mark.parametrize("agg", AGGS)
def test_scored_words_and_segments_sentencepiece(agg):
    from gigaam_amd.timestamps_utils import longform_words
    from gigaam_amd.windows import segment_words
    from gigaam_amd.types import Segment
    tok = _Pieces(["<unk>", "▁при", "вет", "▁", "мир", "▁да", "ть", "▁о"])
    wid = len(tok) + 1
    ids = [1, 2, 3, 4, 5, 6, 6, 7, 1]                       # привет | мир | датьть | о | при
    frames = [0, 2, 10, 11, 40, 41, 43, 90, 95]
    words, _ = longform_words(tok, ids, [0] * len(ids), frames, [(0.0, 0.0)], [0.04])
    assert [w.text for w in words] == ["привет", "мир", "дать" + "ть", "о", "при"]
    # segments as the windowed route cuts them: runs of words
    segments = [Segment(text=" ".join(w.text for w in r), start=r[0].start, end=r[-1].end, words=r) for r in segment_words(words, 1.0, 22.0)]
    assert len(segments) >= 2
    conf = np.random.default_rng(5).uniform(0.05, 1.0, len(ids)).tolist()
    _, scored, segs, total = _check_scored(tok, ids, conf, words, segments, agg, wid)
    assert scored[0].confidence == pytest.approx(C.aggregate(conf[0:2], agg), abs=1e-12)
    assert scored[1].confidence == pytest.approx(C.aggregate(conf[2:4], agg), abs=1e-12)      # a lone marker piece belongs to the word it starts
    assert sum(len(s.words) for s in segs) == len(words)
    with pytest.raises(ValueError):
        from gigaam_amd.timestamps_utils import score_longform
        score_longform(tok, ids, conf, words[:-1], segments, agg, wid)


def test_dataclasses_and_argument_errors():
    import gigaam_amd
    from gigaam_amd.types import LongformConfidenceResult, ScoredSegment, ScoredWord
    assert gigaam_amd.LongformConfidenceResult is LongformConfidenceResult and gigaam_amd.ScoredSegment is ScoredSegment
    w = ScoredWord("да", 0.0, 0.4, 0.9)
    sg = ScoredSegment("да", 0.0, 0.4, [w], 0.9)
    r = LongformConfidenceResult(text="да", segments=[sg], words=[w], token_ids=[5, 1], token_segments=[0, 0], token_frames=[0, 3],
                                 token_times=[0.0, 0.12], token_confidence=[0.8, 1.0], confidence=0.9)
    assert str(r) == "да" and len(r) == 1 and list(r) == [sg] and r.gaps == [] and r.score is None and r.log_likelihood is None
    assert hasattr(gigaam_amd.GigaAMASR, "confidence_longform")
    from gigaam_amd.engine import HipEngine
    assert hasattr(HipEngine, "op_ctc_confidence_long")
    from gigaam_amd._lib import SIGNATURES
    assert len(SIGNATURES["gam_op_ctc_confidence_long"][1]) == 15
