"""CPU: the float64 reference of RNN-T beam search with a word n-gram LM (tests/rnnt_beam_ref.py) -- with zero weights it is
tests/rnnt_beam_ref.py's search exactly, with nothing pruned its pick is the exact MAP of log P_S(y | x) + LM term, merged hypotheses
agree on their LM state -- under char-wise and SentencePiece-style word classes, with and without an <unk> unigram, at orders 1-5;
and the decoding object / set_decoding API with an LM, without a GPU."""
import itertools

import numpy as np
import pytest

from beam_common import small_sd as _small_sd

import ctc_lm_ref as CL
import rnnt_beam_ref as R
from ctc_beam_ref import Trie

# token classes over V - 1 non-blank ids (+ blank, class 0): char-wise letters and a space separator, or SentencePiece-style pieces
# (class 1 starts a word, as a piece beginning with U+2581 does)
CLASSES = {
    "char": {3: [0, 2, 0], 4: [0, 0, 2, 0], 5: [0, 0, 0, 2, 0]},
    "piece": {3: [1, 0, 0], 4: [1, 0, 1, 0], 5: [1, 0, 1, 0, 0]},
}


def _arpa(rng, words, order, unk=True):
    """ARPA text over ``words``: every unigram and random higher-order n-grams (with <s> / </s>), random back-offs."""
    voc = list(words) + ["</s>"]
    ng = {1: {(w,): (-rng.uniform(0.3, 2.5), -rng.uniform(0.0, 1.0)) for w in list(words) + ["<s>"] + (["<unk>"] if unk else [])}}
    ng[1][("</s>",)] = (-rng.uniform(0.3, 2.5), 0.0)
    for n in range(2, order + 1):
        d = {}
        for _ in range(4 * len(voc)):
            k = tuple(["<s>"] * (rng.random() < 0.3) + [voc[rng.integers(0, len(voc) - 1)] for _ in range(n)])[:n - 1]
            d[k + (voc[rng.integers(0, len(voc))],)] = None
        ng[n] = {k: (-rng.uniform(0.05, 1.5), -rng.uniform(0.0, 0.8) if n < order else 0.0) for k in d}
    lines = ["\\data\\"] + [f"ngram {n}={len(ng[n])}" for n in range(1, order + 1)]
    for n in range(1, order + 1):
        lines += ["", f"\\{n}-grams:"]
        for k, (p, b) in ng[n].items():
            lines.append(f"{p:.4f}\t{' '.join(k)}" + (f"\t{b:.4f}" if n < order else ""))
    return "\n".join(lines + ["", "\\end\\", ""])


def _spec(rng, classes, order, alpha, beta, unk=True):
    """An LMSpec whose spelling table names some of the short words the class rule allows (the others are <unk>)."""
    V = len(classes)
    spell = {}
    for n in (1, 2, 3):
        for ids in itertools.product(range(V - 1), repeat=n):
            if any(classes[c] == 2 for c in ids) or any(classes[c] == 1 for c in ids[1:]):
                continue
            if rng.random() < 0.6 or not spell:
                spell[ids] = "w" + "_".join(map(str, ids))
    return CL.LMSpec(CL.ArpaLM(_arpa(rng, sorted(set(spell.values())), order, unk)), classes, spell, alpha, beta)


def _case(seed, V, L=1, out_gain=1.0, blank_bias=0.0, T=6, D=6):
    rng = np.random.default_rng(seed)
    head = R.head_from_state_dict(_small_sd(rng, V, L=L, out_gain=out_gain, blank_bias=blank_bias))
    return rng, head, R.encoder_projection(head, rng.standard_normal((D, T)))


@pytest.mark.parametrize("kind", ["char", "piece"])
def test_zero_weights_equal_the_search_without_lm(kind):
    """alpha = beta = 0: ids, frames, score, logp, the final beam and every margin are those of rnnt_beam_ref.beam_search."""
    n = 0
    for seed, (V, W, S, L, hot) in enumerate(((5, 2, 1, 1, False), (5, 4, 3, 2, True), (4, 8, 2, 1, True), (3, 1, 4, 1, False))):
        rng, head, encp = _case(100 + seed, V, L=L, out_gain=1.5, T=9)
        spec = _spec(rng, CLASSES[kind][V], 3, 0.0, 0.0)
        hw = [[0, 1], [V - 2]] if hot else []
        a = R.beam_search(head, encp, W, S, hotwords=hw, beta=1.5)
        b = R.beam_search(head, encp, W, S, hotwords=hw, beta=1.5, lm=spec)
        for k in ("ids", "frames", "score", "logp", "beam", "margins", "final_margin"):
            assert b[k] == a[k], (seed, k)
        n += 1
    assert n == 4


@pytest.mark.parametrize("unk", [True, False])
@pytest.mark.parametrize("kind", ["char", "piece"])
@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_unbounded_beam_with_lm_is_exact_map(order, kind, unk):
    """Nothing pruned (a beam wider than every hypothesis set): every final score is log P_S(y | x), and the pick is the argmax over
    every y of log P_S(y | x) + committed hotword bonus + the LM term (every word and </s>), at V 3-5 and S 1-2."""
    for trial, (V, T, S) in enumerate(((3, 3, 1), (4, 2, 2), (5, 2, 1))):
        rng, head, encp = _case(1000 * order + 10 * trial + (5 if unk else 0) + (2 if kind == "piece" else 0), V, out_gain=0.8, T=T)
        spec = _spec(rng, CLASSES[kind][V], order, 1.3, 0.7, unk)
        hw = [[0, 1]] if trial == 1 else []
        res = R.beam_search(head, encp, 10 ** 6, S, hotwords=hw, beta=1.0, lm=spec)
        pred = R.Predictor(head)
        joint = lambda t, y: R.joint_lp(head, encp[t], pred(y))     # noqa: E731
        for y, sc in res["beam"]:
            assert sc == pytest.approx(R.exact_loglik(joint, y, T, S), abs=1e-9), y
        trie = Trie(hw)
        best, best_y, ll = -np.inf, None, None
        for k in range(T * S + 1):
            for y in itertools.product(range(V - 1), repeat=k):
                lp = R.exact_loglik(joint, y, T, S)
                v = lp + trie.bonus(y, 1.0) + CL.lm_term(y, spec)
                if v > best:
                    best, best_y, ll = v, list(y), lp
        assert res["ids"] == best_y, (trial, res["ids"], best_y)
        assert res["score"] == pytest.approx(best, abs=1e-9)
        assert res["logp"] == pytest.approx(ll, abs=1e-9)
        assert res["lm"] == pytest.approx(CL.lm_term(best_y, spec), abs=1e-12)


@pytest.mark.parametrize("kind", ["char", "piece"])
def test_merged_hypotheses_agree_on_their_lm_state(kind):
    """Blank-heavy joints with several symbols per frame merge many hypotheses in B; the reference asserts at every merge that the
    contributors' LM states are equal, and every final state is the one the hypothesis's own tokens give."""
    merges = 0
    for seed in range(4):
        rng, head, encp = _case(50 + seed, 5, L=2, out_gain=1.2, blank_bias=3.0, T=10)
        spec = _spec(rng, CLASSES[kind][5], 3, 0.9, 0.4)
        res = R.beam_search(head, encp, 32, 3, lm=spec)
        merges += res["merges"]
        for (y, _), st in zip(res["beam"], res["states"]):
            want = spec.start()
            for c in y:
                want = spec.step(want, c)
            assert st == want, y
    assert merges > 20, merges


def test_lm_changes_the_pick_on_a_near_tie():
    """Hand-made joint: one frame whose two best tokens are near-tied; the LM that prefers the runner-up's word flips the pick."""
    V = 4                      # tokens a, b, " ", blank (char-wise)
    classes = CLASSES["char"][4]

    def joint(t, y):
        p = np.full(V, 1e-3)
        if t == 0 and not y:
            p[0], p[1] = 0.50, 0.48
        elif t == 1 and len(y) == 1:
            p[2] = 0.9
        else:
            p[V - 1] = 0.99
        return np.log(p / p.sum())

    plain = R.beam_search(None, None, 4, 1, T=3, joint=joint)
    assert plain["ids"] == [0, 2]
    arpa = "\\data\\\nngram 1=5\n\n\\1-grams:\n-1.0\t<s>\n-1.0\t</s>\n-3.0\ta\n-0.5\tb\n-2.0\t<unk>\n\n\\end\\\n"
    spec = CL.LMSpec(CL.ArpaLM(arpa), classes, {(0,): "a", (1,): "b"}, 0.5, 0.0)
    res = R.beam_search(None, None, 4, 1, T=3, joint=joint, lm=spec)
    assert res["ids"] == [1, 2]
    assert res["score"] == pytest.approx(res["logp"] + CL.lm_term([1, 2], spec), abs=1e-12)


def test_empty_utterance_with_lm():
    rng, head, _ = _case(0, 4)
    spec = _spec(rng, CLASSES["char"][4], 2, 0.5, 1.0)
    res = R.beam_search(head, np.zeros((3, 8)), 4, 2, T=0, lm=spec)
    assert res["ids"] == [] and res["logp"] == 0.0
    assert res["score"] == pytest.approx(0.5 * spec.lm.lnprob("</s>", ["<s>"]), abs=1e-12)


def _rnnt_model(decoding=None):
    import gigaam_amd
    from gigaam_amd import synth
    ck = synth.make_checkpoint("v2_rnnt", seed=1, n_layers=1)
    if decoding is not None:
        ck["cfg"]["decoding"] = decoding
    return gigaam_amd.model_from_checkpoint(ck, "cpu")


_ARPA = ("\\data\\\nngram 1=5\nngram 2=2\n\n\\1-grams:\n-1.0\t<s>\t-0.3\n-1.0\t</s>\n-1.2\tда\t-0.2\n-1.5\tкот\t-0.2\n-2.0\t<unk>\n\n"
         "\\2-grams:\n-0.2\t<s> да\n-0.3\tда кот\n\n\\end\\\n")


def test_cfg_target_and_set_decoding_take_an_lm(tmp_path):
    from gigaam_amd import lm as LM
    from gigaam_amd import synth
    from gigaam_amd.decoding import RNNTBeamDecoding, RNNTGreedyDecoding
    path = tmp_path / "m.arpa"
    path.write_text(_ARPA, encoding="utf-8")
    model = _rnnt_model({"_target_": "gigaam.decoding.RNNTBeamDecoding", "vocabulary": synth.CHAR_VOCAB, "max_symbols_per_step": 10,
                         "beam_size": 8, "lm": str(path), "lm_weight": 0.3, "word_bonus": 0.2})
    d = model.decoding
    assert isinstance(d, RNNTBeamDecoding) and isinstance(d.lm, LM.NgramLM)
    assert (d.beam_size, d.lm_weight, d.word_bonus) == (8, 0.3, 0.2)
    model = _rnnt_model()
    greedy = model.decoding
    lm = LM.NgramLM.from_arpa(str(path))
    model.set_decoding(lm=lm)
    assert isinstance(model.decoding, RNNTBeamDecoding) and model.decoding.beam_size == 4
    assert model.decoding.lm is lm and (model.decoding.lm_weight, model.decoding.word_bonus) == (0.5, 1.0)
    assert model.decoding.hotwords == []
    lm.save(str(tmp_path / "m.npz"))
    model.set_decoding(beam_size=2, lm=str(tmp_path / "m.npz"), lm_weight=0.7, word_bonus=0.0)
    assert model.decoding.lm.counts == lm.counts and (model.decoding.beam_size, model.decoding.lm_weight) == (2, 0.7)
    model.set_decoding(beam_size=4)
    assert model.decoding.lm is None
    model.set_decoding()
    assert type(model.decoding) is RNNTGreedyDecoding and model.decoding.tokenizer is greedy.tokenizer
    # per-call LM keywords stay CTC-only
    model.set_decoding(lm=lm)
    wav, wlen = synth.synth_audio(1, 1.0, seed=3)
    with pytest.raises(TypeError, match="beam search needs a CTC head"):
        model.transcribe_batch(wav, wlen, lm=lm)
