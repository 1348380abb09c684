"""CPU: the float64 confidence reference (tests/confidence_ref.py) on hand-computed cases, word grouping against
``frames_to_words``, and the Python surface's dataclasses and argument checks.  No GPU."""
import math
import os

import numpy as np
import pytest
import torch

from common import ROOT

import confidence_ref as C

NEG = -np.inf


def _rows(*rows):
    """Log-prob rows from probability rows (float32, as the device stores them)."""
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(rows, dtype=np.float64)).astype(np.float32)


def test_entropy_of_one_hot_and_uniform_frames():
    V = 8
    one_hot = np.full((1, V), NEG, dtype=np.float32)
    one_hot[0, 3] = 0.0
    uniform = np.full((1, V), -math.log(V), dtype=np.float32)
    c, s, ok = C.ctc_confidence(one_hot, 1, [3], [0], "entropy", "mean")
    assert ok == 1 and s == [1] and c == [1.0]
    c, s, ok = C.ctc_confidence(uniform, 1, [3], [0], "entropy", "mean")
    assert ok == 1 and s == [1] and abs(c[0]) < 1e-6
    assert C.ctc_confidence(one_hot, 1, [3], [0], "prob", "min")[0] == [1.0]
    assert C.ctc_confidence(uniform, 1, [3], [0], "prob", "prod")[0] == [pytest.approx(1.0 / V, rel=1e-6)]
    # two classes at 1/2 each out of V = 4: H = ln 2, 1 - ln 2 / ln 4 = 1/2
    half = _rows([0.5, 0.5, 0.0, 0.0])
    assert C.ctc_confidence(half, 1, [0], [0], "entropy")[0] == [pytest.approx(0.5, abs=1e-7)]


def test_span_rule_with_a_tie_and_an_entry_frame_of_another_argmax():
    # V = 4 (blank = 3).  Token 1 enters at frame 0 whose argmax is token 0; frames 1, 2 have argmax 1; frame 3 ties 0.4 / 0.4
    # between ids 0 and 1: the tie goes to id 0, so the span of token 1 ends there.  Token 2 enters at frame 4; frame 5 is blank.
    lp = _rows([0.6, 0.3, 0.05, 0.05],
               [0.1, 0.7, 0.1, 0.1],
               [0.2, 0.5, 0.2, 0.1],
               [0.4, 0.4, 0.1, 0.1],
               [0.1, 0.1, 0.6, 0.2],
               [0.1, 0.1, 0.1, 0.7])
    assert [C.argmax_low(r) for r in lp] == [0, 1, 1, 0, 2, 3]
    conf, span, ok = C.ctc_confidence(lp, 6, [1, 2], [0, 4], "prob", "mean")
    assert ok == 1 and span == [3, 1]
    assert conf[0] == pytest.approx((0.3 + 0.7 + 0.5) / 3, rel=1e-6) and conf[1] == pytest.approx(0.6, rel=1e-6)
    assert C.ctc_confidence(lp, 6, [1, 2], [0, 4], "prob", "min")[0] == [pytest.approx(0.3, rel=1e-6), pytest.approx(0.6, rel=1e-6)]
    assert C.ctc_confidence(lp, 6, [1, 2], [0, 4], "prob", "prod")[0] == [pytest.approx(0.3 * 0.7 * 0.5, rel=1e-6), pytest.approx(0.6, rel=1e-6)]
    # with id 0 at frame 3 the tie frame IS its entry; the span of token 1 stops at frames[u + 1] whatever the argmax
    conf, span, ok = C.ctc_confidence(lp, 6, [1, 0, 2], [0, 3, 4], "prob", "mean")
    assert ok == 1 and span == [3, 1, 1] and conf[1] == pytest.approx(0.4, rel=1e-6)
    conf, span, ok = C.ctc_confidence(lp, 6, [1, 1], [0, 2], "prob", "mean")       # the next token's entry bounds the span
    assert ok == 1 and span == [2, 1]
    # the last token's span is bounded by T, not by the array
    assert C.ctc_confidence(lp, 2, [1], [0], "prob", "mean")[1] == [2]
    # entropy of the span: the mean of the frames' own values
    e = [C.measure_logp(lp[f], 1, "entropy") for f in range(3)]
    assert C.ctc_confidence(lp, 6, [1, 2], [0, 4], "entropy", "mean")[0][0] == pytest.approx(sum(e) / 3, rel=1e-12)
    # the greedy decode's spans are its runs
    ids, frames = C.ctc_greedy(lp, 6)
    assert (ids, frames) == ([0, 1, 0, 2], [0, 1, 3, 4])
    assert C.ctc_confidence(lp, 6, ids, frames)[1] == [1, 2, 1, 1]


def test_aggregations():
    assert C.aggregate([0.5, 0.25, 1.0], "mean") == pytest.approx(1.75 / 3)
    assert C.aggregate([0.5, 0.25, 1.0], "min") == 0.25
    assert C.aggregate([0.5, 0.25, 1.0], "prod") == 0.125
    assert C.aggregate([], "mean") is None and C.aggregate([], "prod") is None
    with pytest.raises(ValueError):
        C.aggregate([1.0], "median")
    from gigaam_amd.timestamps_utils import aggregate_confidence
    for how in ("mean", "min", "prod"):
        assert aggregate_confidence([0.5, 0.25, 1.0], how) == pytest.approx(C.aggregate([0.5, 0.25, 1.0], how), rel=1e-15)
        assert aggregate_confidence([], how) is None
    with pytest.raises(ValueError, match="unknown confidence aggregation"):
        aggregate_confidence([1.0], "median")


@pytest.mark.parametrize("ids,frames,T,cap,why", [
    ([3], [0], 4, None, "the blank as an id"),
    ([-1], [0], 4, None, "a negative id"),
    ([0], [4], 4, None, "a frame at T"),
    ([0], [-1], 4, None, "a negative frame"),
    ([0, 1], [2, 2], 4, None, "CTC frames not strictly increasing"),
    ([0, 1], [2, 1], 4, None, "frames decreasing"),
    ([0, 1, 2], [0, 1, 2], 4, 2, "more tokens than cap"),
    ([0], [0], 0, None, "a token with T = 0"),
])
def test_invalid_rows_get_status_0(ids, frames, T, cap, why):
    lp = _rows(*[[0.25, 0.25, 0.25, 0.25]] * 4)
    conf, span, ok = C.ctc_confidence(lp, T, ids, frames, cap=cap)
    assert ok == 0 and conf == [-1.0] * len(ids) and span == [0] * len(ids), why
    if why != "CTC frames not strictly increasing":
        assert not C.valid(ids, frames, T, 4, False, cap), why
    else:
        assert C.valid(ids, frames, T, 4, False, cap)          # several tokens on one frame: a transducer path


def test_empty_rows_are_valid():
    lp = _rows([0.25, 0.25, 0.25, 0.25])
    assert C.ctc_confidence(lp, 0, [], []) == ([], [], 1)
    assert C.ctc_confidence(lp, 1, [], []) == ([], [], 1)


def test_rnnt_reference_on_a_small_head():
    import rnnt_align_ref as A
    import rnnt_beam_ref as R
    from beam_common import small_sd
    rng = np.random.default_rng(4)
    V, T = 6, 5
    head = R.head_from_state_dict(small_sd(rng, V), 1)
    encp = rng.standard_normal((T, 8))
    ids, frames = [1, 0, 4], [0, 0, 3]
    conf, ok = C.rnnt_confidence(head, encp, T, ids, frames, "prob")
    lat = A.lattice(head, encp, ids, T)
    assert ok == 1
    for u in range(3):      # p(token) is exp(le) of the lattice node the token was emitted from
        assert conf[u] == pytest.approx(math.exp(lat[frames[u], u, 1]), rel=1e-12)
    ent, ok = C.rnnt_confidence(head, encp, T, ids, frames, "entropy")
    assert ok == 1 and all(0.0 <= e <= 1.0 for e in ent)
    assert C.rnnt_confidence(head, encp, T, [1, 5], [0, 1])[1] == 0           # the blank as an id
    assert C.rnnt_confidence(head, encp, T, [1, 2], [2, 1])[1] == 0           # frames decrease
    assert C.rnnt_confidence(head, encp, T, [1], [5])[1] == 0
    assert C.rnnt_confidence(head, encp, 0, [], []) == ([], 1)


def _check_groups(tok, ids):
    from gigaam_amd.timestamps_utils import frames_to_words, word_token_groups
    frames = list(range(0, 2 * len(ids), 2))
    words = frames_to_words(tok, ids, frames, 0.04)
    for groups in (C.word_groups(tok, ids), word_token_groups(tok, ids)):
        assert len(groups) == len(words)
        for g, w in zip(groups, words):
            text = "".join(tok.id_to_str(ids[i]) for i in g).replace("▁", " ").strip()
            assert text == w.text
            assert w.start == pytest.approx(frames[g[0]] * 0.04) and w.end == pytest.approx((frames[g[-1]] + 1) * 0.04)
    return C.word_groups(tok, ids), words


def test_word_groups_charwise_exclude_the_separator():
    from gigaam_amd import synth
    from gigaam_amd.decoding import Tokenizer
    tok = Tokenizer(synth.CHAR_VOCAB)
    sp = synth.CHAR_VOCAB.index(" ")
    ids = tok.encode(" да  нет кот ")
    groups, words = _check_groups(tok, ids)
    assert [w.text for w in words] == ["да", "нет", "кот"] and [len(g) for g in groups] == [2, 3, 3]
    assert all(ids[i] != sp for g in groups for i in g)
    conf = [0.5 if i == sp else 1.0 for i in ids]          # the separators' confidences reach no word
    assert C.word_confidences(tok, ids, conf, "min") == [1.0, 1.0, 1.0]
    assert _check_groups(tok, [sp, sp])[0] == [] and _check_groups(tok, [])[0] == []


def test_word_groups_sentencepiece():
    pytest.importorskip("sentencepiece")
    from gigaam_amd.decoding import Tokenizer
    tok = Tokenizer([], os.path.join(ROOT, "tests", "golden", "spm256.model"))
    rng = np.random.default_rng(1)
    starts = [i for i in range(len(tok)) if tok.id_to_str(i).startswith("▁")]
    assert starts
    n = 0
    for _ in range(20):
        ids = rng.integers(3, len(tok), int(rng.integers(1, 30))).tolist()
        ids[int(rng.integers(0, len(ids)))] = starts[int(rng.integers(0, len(starts)))]
        groups, words = _check_groups(tok, ids)
        n += len(words)
        for g in groups[1:]:
            assert tok.id_to_str(ids[g[0]]).startswith("▁")       # a marker piece belongs to the word it starts
    assert n > 20
    ids = rng.integers(3, len(tok), 12).tolist()
    again = tok.encode(tok.decode(ids))                    # a round trip through text keeps the words
    assert len(_check_groups(tok, again)[0]) == len(tok.decode(ids).split())


def test_dataclasses():
    import gigaam_amd
    from gigaam_amd.types import ConfidenceResult, ScoredWord, Word
    w = ScoredWord("да", 0.0, 0.4, 0.9)
    r = ConfidenceResult(text="да", words=[w], token_ids=[5, 1], token_frames=[0, 3], token_confidence=[0.8, 1.0], confidence=0.9, feasible=True)
    assert str(r) == "да" and r.words[0].confidence == 0.9 and (w.text, w.start, w.end) == ("да", 0.0, 0.4)
    assert Word("да", 0.0, 0.4) == Word(text="да", start=0.0, end=0.4)          # Word stays as it is
    assert gigaam_amd.ConfidenceResult is ConfidenceResult and gigaam_amd.ScoredWord is ScoredWord
    assert ConfidenceResult("", [], [], [], [], None, True).confidence is None


def test_confidence_argument_checks_need_no_gpu():
    import gigaam_amd
    from gigaam_amd import synth
    from gigaam_amd.engine import HipEngine
    assert HipEngine._confidence_codes("prob", "mean") == (0, 0) and HipEngine._confidence_codes("entropy", "prod") == (1, 2)
    assert HipEngine._confidence_codes("prob", "min") == (0, 1)
    wav, wlen = synth.synth_audio(2, 0.5, seed=3)
    ctc = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=1, n_layers=1), "cpu")
    rnnt = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_rnnt", seed=1, n_layers=1), "cpu")
    for model in (ctc, rnnt):
        with pytest.raises(ValueError, match="unknown confidence measure"):
            model.confidence_batch(wav, wlen, measure="margin")
        with pytest.raises(ValueError, match="unknown confidence aggregation"):
            model.confidence_batch(wav, wlen, aggregation="median")
        with pytest.raises(ValueError, match="unknown confidence measure"):
            model.confidence("no-such-file.wav", measure="margin")
        with pytest.raises(ValueError, match="unknown confidence aggregation"):
            model.confidence("no-such-file.wav", "да", aggregation="max")
        with pytest.raises(ValueError, match="1 texts for a batch of 2"):
            model.confidence_batch(wav, wlen, ["а"])
        with pytest.raises(ValueError, match="characters not in the vocabulary"):
            model.confidence_batch(wav, wlen, ["а", "q~"])
    for kw in (dict(beam_size=4), dict(hotwords=["а"])):
        with pytest.raises(TypeError, match="beam search needs a CTC head"):
            rnnt.confidence_batch(wav, wlen, **kw)
        with pytest.raises(TypeError, match="beam search needs a CTC head"):
            rnnt.confidence("no-such-file.wav", **kw)
        with pytest.raises(ValueError, match="cannot be combined with a given text"):
            ctc.confidence_batch(wav, wlen, ["а", "б"], **kw)
    rnnt.set_decoding(beam_size=4)          # whatever the decoding object, the per-call options stay CTC-only
    with pytest.raises(TypeError, match="beam search needs a CTC head"):
        rnnt.confidence_batch(wav, wlen, beam_size=4)
