"""CPU: the float64 RNN-T beam search reference (tests/rnnt_beam_ref.py) -- with nothing pruned its scores are the exact log P_S(y | x)
and its pick the exact MAP, on peaked joints it is the oracle's greedy decode -- and the decoding object / set_decoding API without a
GPU."""
import itertools

import numpy as np
import pytest
import torch

from beam_common import small_sd as _small_sd
from common import O

import rnnt_beam_ref as R
from ctc_beam_ref import Trie


@pytest.mark.parametrize("hot", [False, True])
def test_unpruned_scores_are_the_exact_loglik_and_the_pick_is_the_map(hot):
    """V = 3, S = 1, T <= 4, W = 32: at most 31 distinct hypotheses, nothing is pruned.  Every final beam entry's score is log P_1(y | x)
    by the (t, u, symbols-in-frame) DP, and the pick is the argmax of log P + committed bonus over every y."""
    rng = np.random.default_rng(7 if hot else 3)
    n = 0
    for trial in range(6):
        V, S = 3, 1
        sd = _small_sd(rng, V, L=1 + trial % 2, out_gain=0.8)
        head = R.head_from_state_dict(sd)
        T = 1 + trial % 4
        encp = R.encoder_projection(head, rng.standard_normal((6, T)))
        hw = [rng.integers(0, V - 1, int(rng.integers(1, 3))).tolist() for _ in range(2)] if hot else []
        res = R.beam_search(head, encp, 32, S, hotwords=hw, beta=1.5)
        pred = R.Predictor(head)
        joint = lambda t, y: R.joint_lp(head, encp[t], pred(y))     # noqa: E731
        assert len(res["beam"]) == sum(2 ** k for k in range(T + 1))
        for y, sc in res["beam"]:
            assert sc == pytest.approx(R.exact_loglik(joint, y, T, S), abs=1e-9), (y, T)
        trie = Trie(hw)
        best, best_y = -np.inf, None
        for k in range(T * S + 1):
            for y in itertools.product(range(V - 1), repeat=k):
                v = R.exact_loglik(joint, y, T, S) + trie.bonus(y, 1.5)
                if v > best:
                    best, best_y = v, list(y)
        assert res["ids"] == best_y
        assert res["score"] == pytest.approx(best, abs=1e-9)
        assert res["logp"] == pytest.approx(best - trie.bonus(best_y, 1.5), abs=1e-9)
        assert len(res["frames"]) == len(res["ids"]) and res["frames"] == sorted(res["frames"])
        n += 1
    assert n == 6


def test_exact_loglik_sums_to_one_over_every_sequence():
    """The DP is a distribution over label sequences: at V = 3, S = 2, T = 2 the probabilities of every y of length <= 4 sum to 1."""
    rng = np.random.default_rng(1)
    head = R.head_from_state_dict(_small_sd(rng, 3))
    encp = R.encoder_projection(head, rng.standard_normal((6, 2)))
    pred = R.Predictor(head)
    joint = lambda t, y: R.joint_lp(head, encp[t], pred(y))     # noqa: E731
    tot = -np.inf
    for k in range(5):
        for y in itertools.product(range(2), repeat=k):
            tot = np.logaddexp(tot, R.exact_loglik(joint, y, 2, 2))
    assert tot == pytest.approx(0.0, abs=1e-12)


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("S", [1, 3])
def test_peaked_joints_give_the_oracle_greedy_decode(L, S):
    """One class dominant in every joint call: every width gives oracle.rnnt_greedy's ids and frames, the max-symbols rule included."""
    rng = np.random.default_rng(10 * L + S)
    V, D, T = 6, 6, 14
    sd = _small_sd(rng, V, L=L, out_gain=25.0, blank_bias=2.0)
    head = R.head_from_state_dict(sd)
    enc = (rng.standard_normal((2, D, T)) * 2.0).astype(np.float32).astype(np.float64)
    lens = [T, 9]
    want = O.rnnt_greedy(sd, torch.from_numpy(enc.astype(np.float32)), torch.tensor(lens), max_symbols=S, n_layers=L)
    assert sum(len(ids) for ids, _ in want) > 3      # (the case emits)
    for b in range(2):
        encp = R.encoder_projection(head, enc[b])
        for W in (1, 4):
            res = R.beam_search(head, encp, W, S, T=lens[b])
            assert (res["ids"], res["frames"]) == (want[b][0], want[b][1]), (b, W, L, S)


def test_empty_utterance():
    rng = np.random.default_rng(0)
    head = R.head_from_state_dict(_small_sd(rng, 4))
    res = R.beam_search(head, np.zeros((3, 8)), 4, 2, T=0)
    assert res["ids"] == [] and res["frames"] == [] and res["score"] == 0.0 and res["logp"] == 0.0


def _rnnt_model(decoding=None):
    import gigaam_amd
    from gigaam_amd import synth
    ck = synth.make_checkpoint("v2_rnnt", seed=1, n_layers=1)
    if decoding is not None:
        ck["cfg"]["decoding"] = decoding
    return gigaam_amd.model_from_checkpoint(ck, "cpu")


def test_cfg_target_instantiates_beam_decoding():
    from gigaam_amd import synth
    from gigaam_amd.decoding import RNNTBeamDecoding
    model = _rnnt_model({"_target_": "gigaam.decoding.RNNTBeamDecoding", "vocabulary": synth.CHAR_VOCAB, "max_symbols_per_step": 10,
                         "beam_size": 8, "hotwords": ["да"], "hotword_boost": 3.0})
    d = model.decoding
    assert isinstance(d, RNNTBeamDecoding)
    assert (d.beam_size, d.max_symbols, d.hotwords, d.hotword_boost) == (8, 10, ["да"], 3.0)
    assert d.hotword_ids(d.hotwords) == [d.tokenizer.encode("да")]
    with pytest.raises(ValueError):
        RNNTBeamDecoding(synth.CHAR_VOCAB, beam_size=33)
    with pytest.raises(ValueError):
        RNNTBeamDecoding(synth.CHAR_VOCAB, max_symbols_per_step=17)


def test_set_decoding_switches_and_validates():
    import gigaam_amd
    from gigaam_amd import synth
    from gigaam_amd.decoding import RNNTBeamDecoding, RNNTGreedyDecoding
    model = _rnnt_model()
    greedy = model.decoding
    assert type(greedy) is RNNTGreedyDecoding
    model.set_decoding(hotwords=["да"])
    assert isinstance(model.decoding, RNNTBeamDecoding) and model.decoding.beam_size == 4
    assert model.decoding.hotwords == ["да"] and model.decoding.hotword_boost == 2.0
    model.set_decoding(beam_size=16, hotword_boost=5.0)
    assert model.decoding.beam_size == 16 and model.decoding.hotwords == [] and model.decoding.hotword_boost == 5.0
    assert model.decoding.tokenizer is greedy.tokenizer and model.decoding.max_symbols == greedy.max_symbols
    for w in (0, 33):
        with pytest.raises(ValueError):
            model.set_decoding(beam_size=w)
    model.set_decoding()
    assert type(model.decoding) is RNNTGreedyDecoding
    assert model.decoding.tokenizer is greedy.tokenizer and model.decoding.max_symbols == greedy.max_symbols
    # per-call beam keywords stay CTC-only, whatever the decoding object
    model.set_decoding(beam_size=4)
    wav, wlen = synth.synth_audio(1, 1.0, seed=3)
    with pytest.raises(TypeError, match="beam search needs a CTC head"):
        model.transcribe_batch(wav, wlen, beam_size=4)
    ctc = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=1, n_layers=1), "cpu")
    with pytest.raises(TypeError):
        ctc.set_decoding(beam_size=4)
    with pytest.raises(TypeError):
        ctc.set_decoding()
