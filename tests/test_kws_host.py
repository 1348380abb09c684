"""CPU: the float64 keyword-search reference (tests/kws_ref.py) on planted occurrences and hand-made score rows, and the host side
of GigaAMASR.find_keywords -- thresholds, tokenisation, every error raised before a kernel runs, times from frames, the order of
the hits, and the ctypes declarations against the header."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from common import ROOT

import kws_inputs as I
import kws_ref as R
from gigaam_amd import _lib, synth
from gigaam_amd.decoding import CTCGreedyDecoding, keyword_hits, keyword_min_scores, sort_keyword_hits
from gigaam_amd.types import KeywordHit, KeywordSearchResult

NEG = -np.inf


@pytest.mark.parametrize("V,T", [(34, 160), (257, 400), (1025, 625)])
def test_reference_recovers_planted_occurrences_exactly(V, T):
    rng = np.random.default_rng(V + T)
    kws = [I.keyword(rng, U, V) for U in (1, 2, 5, 17, 40, 64)]
    kws[3][4] = kws[3][3]                                    # an adjacent repeat: needs its blank
    top = I.background(rng, T, V)
    planted, pos = {}, 4
    for k, y in enumerate(kws):
        r = I.plant(rng, top, V, y, pos, T)
        if r is not None:
            planted[k] = r[:2]
            pos = r[2]
    assert len(planted) >= 5
    lp = I.log_probs(rng, 1, T, V, "peaked", top[None])[0]
    for k, y in enumerate(kws):
        E, S = R.dense(lp, y)
        assert (E[np.isfinite(E)] <= 0).all()
        assert ((S >= 0) == np.isfinite(E)).all() and (S <= np.arange(T)).all()
        hits, n = R.pick(E, S, len(y) * math.log(0.5), 64)
        assert n == len(hits)
        if k in planted:
            s, e = planted[k]
            assert [(a, b, sc) for a, b, sc in hits if a <= e and b >= s] == [(s, e, 0.0)], (k, hits)
            assert R.span_score(lp, y, s, e) == 0.0
            assert R.span_score(lp, y, s - 1, e) < -1.0 and R.span_score(lp, y, s, e + 1) < -1.0
        fin = np.nonzero(np.isfinite(E))[0]
        assert np.allclose(R.span_scores(lp, y, S[fin], fin), E[fin], rtol=0, atol=1e-9)      # E_t is the score of (S_t, t)


def test_reference_keyword_longer_than_the_audio_scores_nothing():
    rng = np.random.default_rng(1)
    lp = I.log_probs(rng, 1, 5, 9, "flat")[0]
    E, S = R.dense(lp, [0, 1, 2, 3, 4, 5])
    assert (E == NEG).all() and (S == -1).all()
    assert R.pick(E, S, -100.0, 4) == ([], 0)
    E, S = R.dense(lp, [3, 3, 3])                            # three equal tokens need five frames
    assert np.isfinite(E).tolist() == [False] * 4 + [True] and S[4] == 0
    assert R.span_score(lp, [0, 1], 3, 2) == NEG and R.span_score(lp, [0, 1], -1, 3) == NEG


def test_reference_ties_keep_the_earliest_start_and_the_stay():
    V = 4
    lp = np.full((6, V), -2.0)
    for t, v in enumerate([0, 0, 3, 1, 1, 3]):
        lp[t, v] = 0.0
    E, S = R.dense(lp, [0, 1])
    assert E.tolist() == [NEG, -2.0, -2.0, 0.0, 0.0, -2.0]
    assert S.tolist() == [-1, 0, 0, 0, 0, 0]
    assert R.pick(E, S, 2 * math.log(0.5), 8) == ([(0, 4, 0.0)], 1)


def test_pick_rules_on_hand_made_rows():
    E = np.array([NEG, -3.0, -1.0, -2.0, NEG, -0.5, -0.5, NEG, -1.0])
    S = np.array([-1, 0, 0, 1, -1, 4, 5, -1, 8])
    # open at 1; frame 2 overlaps and is better: replace; frame 3 overlaps and is worse: drop; frame 5 starts past the end: emit
    # and open; frame 6 (start 5 <= end 5, equal score): replace; frame 8: emit and open; the end: flush
    hits, n = R.pick(E, S, -3.0, 8)
    assert hits == [(0, 2, -1.0), (5, 6, -0.5), (8, 8, -1.0)] and n == 3
    assert R.pick(E, S, -3.0, 2) == ([(0, 2, -1.0), (5, 6, -0.5)], 3)       # truncated: the count is of all
    assert R.pick(E, S, -0.75, 8) == ([(5, 6, -0.5)], 1)
    assert R.pick(E, S, 0.0, 8) == ([], 0)
    assert R.pick(np.array([-1.0]), np.array([0]), -1.0, 1) == ([(0, 0, -1.0)], 1)


def test_threshold_becomes_min_score_in_float32():
    ms = keyword_min_scores([1, 4, 64], 0.5)
    assert ms.dtype == np.float32 and ms.tolist() == [np.float32(u * math.log(0.5)) for u in (1, 4, 64)]
    assert keyword_min_scores([3], 1.0).tolist() == [0.0]
    assert keyword_min_scores([2, 2], [0.5, 0.25]).tolist() == [np.float32(2 * math.log(0.5)), np.float32(2 * math.log(0.25))]
    for bad in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="threshold"):
            keyword_min_scores([3], bad)
    with pytest.raises(ValueError, match="threshold"):
        keyword_min_scores([3, 3], [0.5, 0.5, 0.5])


def test_keywords_are_tokenised_without_normalisation():
    dec = CTCGreedyDecoding(synth.CHAR_VOCAB)
    ids = dec.keyword_ids(["да", "кредитная карта", [12, 7, 30]])
    assert ids[0] == dec.tokenizer.encode("да") and ids[2] == [12, 7, 30]
    assert dec.tokenizer.encode(" ")[0] in ids[1]            # the space is a token: a word boundary inside the keyword
    for bad, msg in ((["Да"], "characters not in the vocabulary"), ([""], "empty"), ([[]], "empty"), ([], "empty"),
                     (["а" * 65], "65 tokens"), ([[1]] * 4097, "4097 keywords"), ([[dec.blank_id]], "token id"),
                     ([[-1]], "token id"), ("да", "list of keywords")):
        with pytest.raises(ValueError, match=msg):
            dec.keyword_ids(bad)
    assert len(dec.keyword_ids(["а" * 64])[0]) == 64 and len(dec.keyword_ids([[1]] * 4096)) == 4096


def test_model_layer_errors_need_no_gpu():
    import gigaam_amd
    wav, wlen = synth.synth_audio(2, 0.5, seed=3)
    ctc = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=1, n_layers=1), "cpu")
    rnnt = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_rnnt", seed=1, n_layers=1), "cpu")
    for call in (lambda m, kw, **o: m.find_keywords("no-such-file.wav", kw, **o),
                 lambda m, kw, **o: m.find_keywords_batch(wav, wlen, kw, **o),
                 lambda m, kw, **o: m.find_keywords_longform("no-such-file.wav", kw, speech_regions=[(0.0, 1.0)], **o)):
        with pytest.raises(TypeError, match="keyword search needs a CTC head"):
            call(rnnt, ["да"])
        with pytest.raises(ValueError, match="characters not in the vocabulary"):
            call(ctc, ["да", "q"])
        with pytest.raises(ValueError, match="empty"):
            call(ctc, ["да", ""])
        with pytest.raises(ValueError, match="empty"):
            call(ctc, [])
        with pytest.raises(ValueError, match="65 tokens"):
            call(ctc, ["а" * 65])
        with pytest.raises(ValueError, match="4097 keywords"):
            call(ctc, [[1]] * 4097)
        for thr in (0.0, 1.01, [0.5, 0.5, 0.5]):
            with pytest.raises(ValueError, match="threshold"):
                call(ctc, ["да"], threshold=thr)
        for mh in (0, 65):
            with pytest.raises(ValueError, match="max_hits"):
                call(ctc, ["да"], max_hits=mh)
    assert gigaam_amd.KeywordSearchResult is KeywordSearchResult and gigaam_amd.KeywordHit is KeywordHit


def _host(n_hits, frames, scores):
    return {"n_hits": np.asarray(n_hits, dtype=np.int32), "hit_frames": np.asarray(frames, dtype=np.int32),
            "hit_score": np.asarray(scores, dtype=np.float32)}


def test_hits_take_times_from_frames_and_sort_by_start_then_keyword():
    kws, texts = [[5, 6], [7], [8, 9, 10]], ["аб", "в", "где"]
    h = _host([[2, 3, 1]],
              [[[[10, 14], [30, 31]], [[10, 10], [2, 2]], [[0, 9], [-1, -1]]]],
              [[[-0.5, 0.0], [0.0, -0.25], [-1.5, NEG]]])
    hits, truncated = keyword_hits(h, 0, kws, texts, 0.04)
    assert truncated == [1]                                  # three found, two slots
    assert [(x.keyword_index, x.start_frame, x.end_frame) for x in hits] == [(0, 10, 14), (0, 30, 31), (1, 10, 10), (1, 2, 2), (2, 0, 9)]
    a = hits[0]
    assert a.keyword == "аб" and a.start == 10 * 0.04 and a.end == 15 * 0.04 and a.segment is None
    assert a.score == -0.5 and a.confidence == pytest.approx(math.exp(-0.25))
    assert hits[1].confidence == 1.0 and hits[4].confidence == pytest.approx(math.exp(-0.5))
    order = sort_keyword_hits(hits)
    assert [(x.keyword_index, x.start_frame) for x in order] == [(2, 0), (1, 2), (0, 10), (1, 10), (0, 30)]
    # a longform region: file time = region start + frame x the region's shift, frames stay local
    lf, _ = keyword_hits(h, 0, kws, texts, 0.05, offset=100.0, segment=3)
    assert lf[0].start == pytest.approx(100.5) and lf[0].end == pytest.approx(100.75) and lf[0].segment == 3
    assert (lf[0].start_frame, lf[0].end_frame) == (10, 14)
    res = KeywordSearchResult(hits=order, truncated=truncated, keywords=texts)
    assert len(res) == 5 and list(res) == order


_CTYPES = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}


@pytest.mark.parametrize("name", ["gam_ctc_kws", "gam_op_ctc_kws", "gam_set_keywords"])
def test_lib_declares_the_keyword_symbols_with_the_headers_signature(name):
    header = open(os.path.join(ROOT, "include", "gigaam_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in the header"
    want = [C.c_void_p if "*" in a else _CTYPES[a.strip().replace("const ", "").split()[0]] for a in m.group(1).split(",")]
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int and argtypes == want
