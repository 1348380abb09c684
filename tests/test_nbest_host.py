"""CPU: the float64 N-best references (tests/nbest_ref.py) against the 1-best references and brute force, their qualification rate on
the inputs tests/test_hip_nbest.py runs, the ``Hypothesis`` / ``NBestResult`` types and the argument checks of ``transcribe_nbest``."""
import math
import types

import numpy as np
import pytest

import ctc_beam_ref as CR
import nbest_inputs as I
import nbest_ref as N
import rnnt_beam_ref as RR


def _same(h0, ref):
    assert h0["ids"] == ref["ids"] and h0["frames"] == ref["frames"], (h0, ref["ids"], ref["frames"])
    assert h0["score"] == ref["score"] and h0["logp"] == ref["logp"], (h0, ref["score"], ref["logp"])


@pytest.mark.parametrize("V", [34, 1025])
def test_ctc_reference_hypothesis_0_is_the_1best_reference(V):
    """On the hypothesis-0 inputs (plain, hotwords, LM) and on the float64-comparison inputs (with and without hotwords)."""
    n = 0
    for variant, (lp, enc_len, phrases, lm) in I.ctc_hyp0_inputs(V).items():
        spec = lm[1] if lm else None
        for W in (1, 4, 32):
            for b in range(len(enc_len)):
                res = N.ctc_nbest(lp[b], W, enc_len[b], phrases, I.BETA, spec)
                ref = CR.beam_search(lp[b], W, enc_len[b], phrases, I.BETA, spec)
                _same(res["hyps"][0], ref)
                assert res["margins"] == ref["margins"]
                assert 1 <= len(res["hyps"]) <= W
                n += 1
    for W, lp, enc_len, phrases in I.ctc_ref_inputs(V, "flat"):
        for b in range(len(enc_len)):
            _same(N.ctc_nbest(lp[b], W, enc_len[b], phrases, I.BETA)["hyps"][0], CR.beam_search(lp[b], W, enc_len[b], phrases, I.BETA))
            n += 1
    assert n == 3 * 3 * 6 + 8 * 6


@pytest.mark.parametrize("V", [34, 1025])
def test_rnnt_reference_hypothesis_0_is_the_1best_reference(V):
    _, _, head = I.rnnt_head(V)
    for variant, (encp, enc_len, phrases, lm) in I.rnnt_hyp0_inputs(V).items():
        spec = lm[1] if lm else None
        for W, S in ((1, 10), (4, 1), (4, 10), (32, 1)):
            for b in range(len(enc_len)):
                e64 = encp[b].astype(np.float64)
                res = N.rnnt_nbest(head, e64, W, S, enc_len[b], phrases, I.BETA, lm=spec)
                ref = RR.beam_search(head, e64, W, S, enc_len[b], phrases, I.BETA, lm=spec)
                _same(res["hyps"][0], ref)
                assert res["margins"] == ref["margins"]
                assert sorted(tuple(h["ids"]) for h in res["hyps"]) == sorted(y for y, _ in ref["beam"])


def _check_against_brute(hyps, brute, what):
    assert len(hyps) == len(brute), (what, len(hyps), len(brute))
    for r, (h, (val, y, ll)) in enumerate(zip(hyps, brute)):
        assert abs(h["score"] - val) <= 1e-9 and abs(h["logp"] - ll) <= 1e-9, (what, r, h, val, ll)
    # the order: wherever the brute-force values are apart, the sequences agree
    vals = [v for v, _, _ in brute]
    for r, h in enumerate(hyps):
        apart = (r == 0 or vals[r - 1] - vals[r] > 1e-9) and (r + 1 == len(vals) or vals[r] - vals[r + 1] > 1e-9)
        if apart:
            assert h["ids"] == brute[r][1], (what, r, h["ids"], brute[r][1])


def test_ctc_reference_is_the_brute_force_list_when_nothing_is_pruned():
    """V = 3, T <= 4, W = 32: every prefix with a finite value is in the final beam."""
    for hot, lp, enc_len in I.ctc_exact_inputs():
        for b, T in enumerate(enc_len):
            res = N.ctc_nbest(lp[b], 32, T, hot, I.EXACT_BETA)
            _check_against_brute(res["hyps"], N.ctc_brute(lp[b].astype(np.float64), T, hot, I.EXACT_BETA), (hot, b))


def test_rnnt_reference_is_the_brute_force_list_when_nothing_is_pruned():
    """V = 3, S = 1, T <= 4, W = 32."""
    _, _, head = I.rnnt_head(3, 1, 0.0)
    for hot, encp, enc_len in I.rnnt_exact_inputs():
        for b, T in enumerate(enc_len):
            res = N.rnnt_nbest(head, encp[b].astype(np.float64), 32, 1, T, hot, I.EXACT_BETA)
            _check_against_brute(res["hyps"], N.rnnt_brute(head, encp[b], T, hot, I.EXACT_BETA), (hot, b))


@pytest.mark.parametrize("V,kind", I.CTC_REF_SETS)
def test_ctc_inputs_qualify_for_nbest_comparison(V, kind):
    """The GPU test's cap -- at least 90 % of each parameter set's utterances qualify at N = W -- holds on the reference alone."""
    n = ok = 0
    for W, lp, enc_len, phrases in I.ctc_ref_inputs(V, kind):
        for b in range(len(enc_len)):
            ok += N.qualifies(N.ctc_nbest(lp[b], W, enc_len[b], phrases, I.BETA), W, N.CTC_MARGIN)
            n += 1
    print(f"ctc {V} {kind}: {ok}/{n} qualify")
    assert ok >= 0.9 * n, (ok, n)


@pytest.mark.parametrize("V,kind,L", I.RNNT_REF_SETS)
def test_rnnt_inputs_qualify_for_nbest_comparison(V, kind, L):
    _, _, head = I.rnnt_head(V, L, 14.0 if kind == "blank" else None)
    n = ok = 0
    for W, S, encp, enc_len in I.rnnt_ref_inputs(V, kind, L):
        for b in range(len(enc_len)):
            ok += N.qualifies(N.rnnt_nbest(head, encp[b].astype(np.float64), W, S, enc_len[b]), W, N.RNNT_MARGIN)
            n += 1
    print(f"rnnt {V} {kind} L{L}: {ok}/{n} qualify")
    assert ok >= 0.9 * n, (ok, n)


def test_hypothesis_and_nbest_result():
    from gigaam_amd.types import Hypothesis, NBestResult, nbest_posteriors
    scores = [-3.25, -4.0, -4.0, -11.5]
    post = nbest_posteriors(scores)
    assert abs(math.fsum(post) - 1.0) <= 1e-12
    assert all(post[i] >= post[i + 1] for i in range(len(post) - 1)) and post[1] == post[2]
    z = math.fsum(math.exp(s) for s in scores)
    assert all(abs(p - math.exp(s) / z) <= 1e-12 for p, s in zip(post, scores))
    assert nbest_posteriors([-1234.5]) == [1.0]          # (far below exp's range: the maximum is subtracted first)
    assert nbest_posteriors([]) == []
    hyps = [Hypothesis(text=f"t{r}", token_ids=[r], token_frames=[r], score=s, logp=s - 1.0, posterior=p) for r, (s, p) in enumerate(zip(scores, post))]
    res = NBestResult(hyps)
    assert len(res) == 4 and res.best is hyps[0] and res.text == "t0" and str(res) == "t0" and list(res) == hyps
    assert res.best.words is None and str(res.best) == "t0"
    assert NBestResult([]).text == "" and len(NBestResult([])) == 0


def test_transcribe_nbest_checks_its_arguments_without_a_device():
    from gigaam_amd import decoding, synth
    from gigaam_amd.model import GigaAMASR
    ctc = types.SimpleNamespace(decoding=decoding.CTCGreedyDecoding(synth.CHAR_VOCAB))
    width = lambda m, *a: GigaAMASR._nbest_width(m, *a)     # noqa: E731
    assert width(ctc, 5, None, None, None) == 8 and width(ctc, 12, None, None, None) == 12 and width(ctc, 3, 4, None, None) == 4
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match="n_best"):
            width(ctc, bad, None, None, None)
    with pytest.raises(ValueError, match="exceeds beam_size"):
        width(ctc, 5, 4, None, None)
    with pytest.raises(ValueError, match="beam_size"):
        width(ctc, 5, 33, None, None)
    greedy = types.SimpleNamespace(decoding=decoding.RNNTGreedyDecoding(synth.CHAR_VOCAB))
    with pytest.raises(ValueError, match=r"set_decoding\(beam_size="):
        width(greedy, 2, None, None, None)
    with pytest.raises(TypeError):
        width(greedy, 2, 4, None, None)
    beam = types.SimpleNamespace(decoding=decoding.RNNTBeamDecoding(synth.CHAR_VOCAB, beam_size=4))
    assert width(beam, 4, None, None, None) == 4
    with pytest.raises(ValueError, match="exceeds the beam width"):
        width(beam, 5, None, None, None)
    with pytest.raises(TypeError):
        width(beam, 2, None, ["да"], None)
