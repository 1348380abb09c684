"""GPU: CTC prefix beam search with hotword boosting (gam_op_ctc_beam / gam_ctc_beam, gigaam_amd/csrc/gam_beam.h) against the
float64 reference of tests/ctc_beam_ref.py, brute-force MAP, greedy best path, the forward log-likelihood of gam_op_ctc_align,
on another stream, at its limits, on the golden CTC cases, on the full-size 32 x 20 s batch and through the model.

Margin rule: the kernel ranks in fp32 (renormalised every frame), the reference in fp64, so where two hypotheses rank within
rounding of each other either may be kept.  ids / frames are compared on every utterance whose smallest decision margin (each
frame's cut: W-th kept minus (W+1)-th candidate, and the final pick) exceeds MARGIN; the op-level tests require that at least
90 % of their utterances qualify.  score / logp are compared on those utterances within 1e-3 * max(1, |ref|)."""
import itertools

import numpy as np
import pytest
import torch

from beam_common import ctc_hotwords as _hotwords, ctc_op_engine, fullsize_ctc_model as _fullsize_model, log_probs as _log_probs
from beam_common import bar as _bar, compare, run_ctc_op as _run_op, wav_file as _wav_file
from common import load_case, make_engine as _make_engine, report

import ctc_align_ref as A
import ctc_beam_ref as R

pytestmark = pytest.mark.gpu

MODES = ["f16x3", "f32"]
CTC_CASES = ["v1_ctc_l2", "v2_ctc_l2", "v3_ctc_l2", "v3_e2e_ctc_l2"]
MARGIN = 2e-5           # op level: T' <= 40 frames of O(1) relative ranks
MARGIN_LONG = 1e-4      # model level: up to 500 frames


def _op_engine():
    return ctc_op_engine(__name__)


def _compare(h, b, ref, errs, margin):
    return compare(h, b, ref, errs, margin, R.min_margin)


def _greedy(lp, T):
    """Best path as gam_ctc_greedy decodes it: first maximum per frame, repeats collapsed, blanks dropped; frames = first of run."""
    V = lp.shape[1]
    lab = np.argmax(lp[:T], axis=1)
    ids, frames, prev = [], [], V - 1
    for t, v in enumerate(lab.tolist()):
        if v != V - 1 and v != prev:
            ids.append(v)
            frames.append(t)
        prev = v
    return ids, frames


def test_op_beam_is_exact_map_when_nothing_is_pruned():
    """V = 3, T <= 4, W = 32: every prefix (at most 31) stays in the beam, so the result is the MAP label sequence -- with and
    without hotwords."""
    eng = _op_engine()
    rng = np.random.default_rng(21)
    V, Tp, B = 3, 4, 16
    errs = {}
    for hot in ([], [[0, 1]], [[1], [0, 0, 1]]):
        eng.set_hotwords(hot, 1.25)
        lp = np.log(rng.dirichlet(np.ones(V) * 0.7, size=(B, Tp))).astype(np.float32)
        enc_len = [1 + b % Tp for b in range(B)]
        h = _run_op(eng, lp, enc_len, 32)
        trie = R.Trie(hot)
        for b in range(B):
            T = enc_len[b]
            best, best_y, ll = -np.inf, None, None
            for n in range(T + 1):
                for y in itertools.product(range(V - 1), repeat=n):
                    l_ = A.forward_loglik(lp[b], list(y), T)
                    if l_ > -np.inf and l_ + trie.bonus(y, 1.25) > best:
                        best, best_y, ll = l_ + trie.bonus(y, 1.25), list(y), l_
            assert h["rows"][b][0] == best_y, (hot, b, h["rows"][b], best_y)
            for k, want in (("score", best), ("logp", ll)):
                errs[k] = max(errs.get(k, 0.0), abs(float(h[k][b]) - want))
                assert abs(float(h[k][b]) - want) <= 1e-5, (hot, b, k)
    eng.set_hotwords([])
    report("ctc_beam_exact_map", **errs)


@pytest.mark.parametrize("V", [34, 257, 1025])
@pytest.mark.parametrize("kind", ["peaked", "flat"])
def test_op_beam_matches_float64_reference(V, kind):
    eng = _op_engine()
    rng = np.random.default_rng(V * 3 + (1 if kind == "flat" else 0))
    T = 24 if kind == "flat" else 40
    B = 6
    errs, n, ok = {}, 0, 0
    for W in (1, 4, 8, 32):
        for hot in (False, True):
            lp = _log_probs(rng, B, T + 3, V, kind)
            enc_len = [T, T - 5, T, 1, T, T + 3]
            phrases = _hotwords(rng, lp, 8) if hot else []
            eng.set_hotwords(phrases, 1.5)
            h = _run_op(eng, lp, enc_len, W)
            for b in range(B):
                ref = R.beam_search(lp[b], W, enc_len[b], phrases, 1.5)
                ok += _compare(h, b, ref, errs, MARGIN)
                n += 1
    eng.set_hotwords([])
    report(f"ctc_beam_op_{V}_{kind}", qualified=f"{ok}/{n}", **errs)
    assert ok >= 0.9 * n, (ok, n)


@pytest.mark.parametrize("V", [34, 257, 1025])
def test_op_beam_on_peaked_log_probs_is_greedy(V):
    eng = _op_engine()
    rng = np.random.default_rng(V + 5)
    B, Tp = 8, 60
    lp = _log_probs(rng, B, Tp, V, "peaked")
    enc_len = [Tp, 50, 1, Tp, 33, Tp, 59, Tp]
    for W in (1, 4, 8):
        h = _run_op(eng, lp, enc_len, W)
        for b in range(B):
            assert h["rows"][b] == _greedy(lp[b], enc_len[b]), (W, b)


def test_op_beam_logp_is_at_most_the_forward_loglik():
    """logp sums the paths the beam kept: never more than log p(ids) over all paths (gam_op_ctc_align)."""
    eng = _op_engine()
    rng = np.random.default_rng(4)
    B, Tp, V = 8, 80, 34
    lp = _log_probs(rng, B, Tp, V, "flat")
    enc_len = [Tp, 70, Tp, 41, Tp, 2, Tp, 64]
    for W in (1, 8):
        h = _run_op(eng, lp, enc_len, W)
        ids = [r[0] for r in h["rows"]]
        al = eng.op_ctc_align(torch.from_numpy(lp), torch.tensor(enc_len, dtype=torch.int32), ids).host()
        for b in range(B):
            assert int(al["status"][b]) == 1
            assert float(h["logp"][b]) <= float(al["loglik"][b]) + 1e-4 * max(1.0, abs(float(al["loglik"][b]))), (W, b)
            assert float(h["score"][b]) == float(h["logp"][b])


def test_op_beam_is_bit_identical_on_another_stream():
    eng = _op_engine()
    rng = np.random.default_rng(9)
    V, Tp = 257, 120
    lp = _log_probs(rng, 4, Tp, V, "flat")
    eng.set_hotwords(_hotwords(rng, lp, 20), 1.0)
    a = _run_op(eng, lp, [Tp, 100, Tp, 7], 8)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        b = _run_op(eng, lp, [Tp, 100, Tp, 7], 8)
    torch.cuda.synchronize()
    eng.set_hotwords([])
    assert a["rows"] == b["rows"]
    for k in ("score", "logp"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_library_rejects_beam_search_beyond_the_limits():
    from gigaam_amd._lib import GigaAMHipError
    eng = _op_engine()
    lp = torch.zeros((1, 10, 5))
    one = torch.tensor([10], dtype=torch.int32)
    for W in (0, 33):
        with pytest.raises(GigaAMHipError, match="beam_size"):
            eng.op_ctc_beam(lp, one, W)
    rc = eng.lib.gam_op_ctc_beam(eng._h, lp.cuda().data_ptr(), one.cuda().data_ptr(), 1, 10, 5, 33, *([None] * 5), None)
    assert rc != 0 and b"beam width" in eng.lib.gam_last_error(eng._h)
    with pytest.raises(GigaAMHipError, match="T'=8193"):
        eng.op_ctc_beam(torch.zeros((1, 8193, 3)), one, 4)
    with pytest.raises(GigaAMHipError, match="V=1026"):
        eng.op_ctc_beam(torch.zeros((1, 4, 1026)), one, 4)
    with pytest.raises(GigaAMHipError, match="phrases"):
        eng.set_hotwords([[1]] * 1025)
    with pytest.raises(GigaAMHipError, match="16384 tokens"):
        eng.set_hotwords([[1] * 20] * 1000)
    with pytest.raises(GigaAMHipError, match="outside"):
        eng.set_hotwords([[0, -1]])
    with pytest.raises(GigaAMHipError, match="empty"):
        eng.set_hotwords([[0], []])
    eng.set_hotwords([[0, 7]])                 # id 7 > V - 2 = 3 for V = 5: refused at the search
    with pytest.raises(GigaAMHipError, match="hotword token id 7"):
        eng.op_ctc_beam(lp, one, 4)
    eng.set_hotwords([])
    eng.op_ctc_beam(lp, one, 4).host()


def _head_engine_lp(eng, enc):
    return eng.ctc_head(enc).double().cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CTC_CASES)
def test_encoded_beam_on_golden_cases_matches_reference(name, mode):
    ck, _, _, gold = load_case(name)
    eng = _make_engine(ck["cfg"], ck["state_dict"], mode)
    enc = torch.from_numpy(gold["encoded"])
    elen = torch.from_numpy(gold["enc_len"])
    lp = _head_engine_lp(eng, enc)
    errs, ok, n = {}, 0, 0
    for W, hot in ((1, False), (8, False), (8, True)):
        rng = np.random.default_rng(len(name) + W)
        phrases = _hotwords(rng, lp, 10) if hot else []
        eng.set_hotwords(phrases, 2.0)
        h = eng.ctc_beam(enc, elen, W).host()
        assert not h["flag"]
        for b in range(lp.shape[0]):
            ref = R.beam_search(lp[b], W, int(gold["enc_len"][b]), phrases, 2.0)
            ok += _compare(h, b, ref, errs, MARGIN_LONG)
            n += 1
    report(f"ctc_beam_golden_{name}_{mode}", qualified=f"{ok}/{n}", **errs)
    assert ok >= 0.5 * n, (ok, n)


@pytest.mark.parametrize("mode", MODES)
def test_fullsize32_transcribe_batch_beam_matches_reference(mode):
    """The 32 x 20 s, 16-layer batch: transcribe_batch(beam_size=8) against the reference beam run on HipEngine.ctc_head's
    log-probs of the same encoder output; word timestamps come from the beam's token frames.  Also times the beam kernel alone."""
    from gigaam_amd import workloads
    from gigaam_amd.timestamps_utils import compute_frame_shift, frames_to_words
    model = _fullsize_model()
    model.set_arithmetic(mode)
    wav, wlen = workloads.config2_batch(32, 20.0, rank=0)
    got = model.transcribe_batch(wav, wlen, word_timestamps=True, beam_size=8)
    eng = model.head.engine
    with torch.inference_mode():
        enc, elen = model._encode(wav.to("cuda:0"), wlen.to("cuda:0"), wlen)
        lp_d = eng.ctc_head(enc)
    lp = lp_d.double().cpu().numpy()
    el = elen.cpu().tolist()
    tok = model.decoding.tokenizer
    ok = 0
    for b in range(32):
        ref = R.beam_search(lp[b], 8, el[b])
        if R.min_margin(ref) <= MARGIN_LONG:
            continue
        ok += 1
        text, words = got[b]
        assert text == tok.decode(ref["ids"]), b
        assert words == frames_to_words(tok, ref["ids"], ref["frames"], compute_frame_shift(int(wlen[b]), el[b])), b
    # the kernel alone on the head's log-probs, device events
    for _ in range(2):
        eng.op_ctc_beam(lp_d, elen, 8)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        eng.op_ctc_beam(lp_d, elen, 8)
    e1.record()
    torch.cuda.synchronize()
    report(f"ctc_beam_fullsize32_{mode}", qualified=f"{ok}/32", op_beam_w8_ms=e0.elapsed_time(e1) / 5)
    assert ok >= 16, ok


def test_model_hotword_makes_a_chosen_word_appear(tmp_path):
    """A word built from runner-up characters of the clip: greedy does not produce it, a boosted beam search does; without
    hotwords a beam of width 1 on this clip reads like greedy where the frames are confident."""
    import gigaam_amd
    from gigaam_amd import synth
    ck = synth.make_checkpoint("v2_ctc", seed=1, n_layers=2)
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    wpath = _wav_file(tmp_path, 8.0, 31)
    greedy = model.transcribe(wpath).text
    tok = model.decoding.tokenizer
    wav, wlen = model._prepare_wav_f32(wpath)
    with torch.inference_mode():
        enc, elen = model._encode(wav, wlen)
        lp = model.head.engine.ctc_head(enc)[0].double().cpu().numpy()[: int(elen[0])]
    order = np.argsort(-lp[:, :-1], axis=1, kind="stable")
    word = None
    for t in range(lp.shape[0] - 3):
        cand = [int(order[t + i, 1]) for i in range(3)]
        text = tok.decode(cand)
        if " " not in text and cand[0] != cand[1] and cand[1] != cand[2] and text not in greedy:
            word = text
            break
    assert word is not None
    res = model.transcribe(wpath, hotwords=[word], hotword_boost=6.0, word_timestamps=True)
    assert word in res.text, (word, res.text, greedy)
    assert word not in greedy
    assert all(w.start <= w.end for w in res.words)
    # the same through the batch API with token ids, and the hotword set is cleared again by a plain beam call
    got = model.transcribe_batch(wav, wlen, beam_size=8, hotwords=[tok.encode(word)], hotword_boost=6.0)
    assert got[0][0] == res.text
    plain = model.transcribe_batch(wav, wlen, beam_size=8)
    assert model.head.engine._hotwords_key[0] == ()
    assert word not in plain[0][0] or word in greedy


def test_model_beam_longform_and_greedy_default(tmp_path):
    """transcribe_longform takes the beam options; without them every path is the greedy one."""
    import gigaam_amd
    from gigaam_amd import synth
    ck = synth.make_checkpoint("v2_ctc", seed=1, n_layers=2)
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    wpath = _wav_file(tmp_path, 12.0, 41)
    regions = [(0.0, 5.0), (5.0, 12.0)]
    g = model.transcribe_longform(wpath, speech_regions=regions)
    b = model.transcribe_longform(wpath, speech_regions=regions, beam_size=4, word_timestamps=True)
    assert len(g.segments) == len(b.segments) >= 1
    for s in b.segments:
        assert s.words is not None
    wav, wlen = synth.synth_audio(2, 3.0, seed=5, lengths=[48000, 31000])
    plain = model.transcribe_batch(wav, wlen)
    with torch.inference_mode():
        enc, elen = model._encode(wav.to("cuda:0"), wlen.to("cuda:0"), wlen)
        dec = model.decoding.decode(model.head, enc, elen)
        beam = model.decoding.decode_beam(model.head, enc, elen, beam_size=4)
    assert [t for t, _ in plain] == [d[0] for d in dec]
    for (text, ids, frames, score, logp), d in zip(beam, dec):
        assert text == model.decoding.tokenizer.decode(ids) and len(frames) == len(ids)
        assert score == logp and logp <= 0.0
