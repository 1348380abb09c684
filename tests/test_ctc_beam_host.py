"""CPU: the float64 CTC prefix beam search reference (tests/ctc_beam_ref.py) -- an unbounded beam is the exact MAP over label
sequences (brute force with tests/ctc_align_ref.forward_loglik), hotword commit and rollback on hand-built cases -- and the
beam options of the model API without a GPU."""
import itertools

import numpy as np
import pytest

import ctc_align_ref as A
import ctc_beam_ref as R


def _lp(rows):
    """Probabilities per frame -> log-probs [T, V] (blank last)."""
    p = np.asarray(rows, dtype=np.float64)
    return np.log(p / p.sum(axis=1, keepdims=True))


def _brute_map(lp, T, hotwords=(), beta=2.0):
    """argmax over every label sequence of length <= T of log p(y) (forward algorithm) + committed hotword bonus."""
    V = lp.shape[1]
    trie = R.Trie(hotwords)
    best, best_y, ll_best = -np.inf, None, None
    for n in range(T + 1):
        for y in itertools.product(range(V - 1), repeat=n):
            ll = A.forward_loglik(lp, list(y), T)
            if ll == -np.inf:
                continue
            v = ll + trie.bonus(y, beta)
            if v > best:
                best, best_y, ll_best = v, list(y), ll
    return best_y, best, ll_best


@pytest.mark.parametrize("hot", [False, True])
def test_unbounded_beam_is_exact_map(hot):
    rng = np.random.default_rng(11 if hot else 5)
    n = 0
    for V in (3, 4):
        for T in range(1, 6 if V == 3 else 5):
            for _ in range(4):
                lp = np.log(rng.dirichlet(np.ones(V) * 0.7, size=T))
                hw = [rng.integers(0, V - 1, int(rng.integers(1, 3))).tolist() for _ in range(2)] if hot else []
                res = R.beam_search(lp, None, hotwords=hw, beta=1.5)
                y, val, ll = _brute_map(lp, T, hw, 1.5)
                assert res["ids"] == y, (V, T, hw, res["ids"], y)
                assert res["score"] == pytest.approx(val, abs=1e-9)
                assert res["logp"] == pytest.approx(ll, abs=1e-9)
                # frames: strictly increasing, one per token, inside the utterance
                assert len(res["frames"]) == len(y) and all(0 <= f < T for f in res["frames"])
                assert res["frames"] == sorted(set(res["frames"]))
                n += 1
    assert n == 36


def test_beam_logp_is_the_forward_loglik_when_nothing_is_pruned():
    rng = np.random.default_rng(2)
    lp = np.log(rng.dirichlet(np.ones(4), size=5))
    res = R.beam_search(lp, None)
    assert res["logp"] == pytest.approx(A.forward_loglik(lp, res["ids"]), abs=1e-12)


def test_empty_utterance_and_width_one():
    lp = _lp([[0.1, 0.2, 0.7]] * 3)
    res = R.beam_search(lp, 4, T=0)
    assert res["ids"] == [] and res["frames"] == [] and res["score"] == 0.0 and res["logp"] == 0.0
    # W = 1 on a peaked input is greedy best path: collapse repeats, drop blanks
    lp = _lp([[0.8, 0.1, 0.1], [0.8, 0.1, 0.1], [0.1, 0.1, 0.8], [0.1, 0.8, 0.1], [0.8, 0.1, 0.1]])
    res = R.beam_search(lp, 1)
    assert res["ids"] == [0, 1, 0] and res["frames"] == [0, 3, 4]


# V = 4: tokens 0, 1, 2; blank 3.  "1 2" is a little more likely than "0 2" (0.45 vs 0.40 at frame 0).
_ROLL = [[0.40, 0.45, 0.05, 0.10], [0.02, 0.02, 0.90, 0.06], [0.02, 0.02, 0.02, 0.94]]


def test_hotword_commits_a_complete_phrase():
    lp = _lp(_ROLL)
    assert R.beam_search(lp, 4)["ids"] == [1, 2]
    res = R.beam_search(lp, 4, hotwords=[[0, 2]], beta=1.0)
    assert res["ids"] == [0, 2]
    assert res["score"] == pytest.approx(res["logp"] + 2.0, abs=1e-12)       # both tokens committed


def test_hotword_partial_match_is_rolled_back():
    """Phrase "0 1": "0 2" leaves it after "0", so its pending bonus goes -- "1 2" wins on log p and the score holds no bonus.
    A search that commits (keeps) the partial bonus on the way out picks "0 2" instead."""
    lp = _lp(_ROLL)
    res = R.beam_search(lp, 4, hotwords=[[0, 1]], beta=1.0)
    assert res["ids"] == [1, 2]
    assert res["score"] == res["logp"]

    class Buggy(R.Trie):
        def step(self, state, c, beta):
            node, acc, cb = state
            if node != 0 and c not in self.kids[node]:
                state = (node, 0.0, cb + acc)         # the bug: the partial match is committed instead of rolled back
            return super().step(state, c, beta)

    orig = R.Trie
    try:
        R.Trie = Buggy
        assert R.beam_search(lp, 4, hotwords=[[0, 1]], beta=1.0)["ids"] == [0, 2]
    finally:
        R.Trie = orig


def test_hotword_trie_has_no_failure_links():
    """The documented limitation: phrase "0 0 1" in "0 0 0 1" -- the third 0 finds no child of "0 0", rolls back and restarts at
    "0", then 1 is no child of "0": no bonus.  "0 0 1" itself is boosted."""
    trie = R.Trie([[0, 0, 1]])
    assert trie.bonus([0, 0, 1], 2.0) == 6.0
    assert trie.bonus([0, 0, 0, 1], 2.0) == 0.0
    assert trie.bonus([2, 0, 0, 1], 2.0) == 6.0
    # a phrase that is a prefix of another: both commit
    trie = R.Trie([[0, 1], [0, 1, 2]])
    assert trie.bonus([0, 1, 2], 1.0) == 3.0
    assert trie.bonus([0, 1, 1], 1.0) == 2.0


def test_transcribe_beam_needs_a_ctc_head():
    import gigaam_amd
    from gigaam_amd import synth
    model = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_rnnt", seed=1, n_layers=1), "cpu")
    wav, wlen = synth.synth_audio(1, 1.0, seed=3)
    for kw in (dict(beam_size=4), dict(hotwords=["а"])):
        with pytest.raises(TypeError, match="beam search needs a CTC head"):
            model.transcribe_batch(wav, wlen, **kw)
        with pytest.raises(TypeError, match="beam search needs a CTC head"):
            model.launch_batch(wav, wlen, **kw)
        with pytest.raises(TypeError, match="beam search needs a CTC head"):
            model.transcribe("no-such-file.wav", **kw)
        with pytest.raises(TypeError, match="beam search needs a CTC head"):
            model.transcribe_longform("no-such-file.wav", speech_regions=[(0.0, 1.0)], **kw)


def test_hotword_strings_are_encoded_with_the_tokenizer():
    from gigaam_amd import synth
    from gigaam_amd.decoding import CTCGreedyDecoding
    dec = CTCGreedyDecoding(synth.CHAR_VOCAB)
    ids = dec.hotword_ids(["да", [3, 4]])
    assert ids == [dec.tokenizer.encode("да"), [3, 4]]
    with pytest.raises(ValueError):
        dec.hotword_ids(["latin"])
