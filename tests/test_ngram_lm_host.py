"""CPU: the word n-gram LM of the CTC beam search -- the ARPA parser and back-off scores of gigaam_amd/lm.py, its device tables
queried by a host emulation of the kernel's probe (gam_search.h), the spelling hashes against tests/ctc_lm_ref.py for char-wise,
piece and SentencePiece vocabularies, and the float64 reference itself: alpha = beta = 0 is the search without an LM, and an
unbounded beam is the brute-force MAP of log p + LM term."""
import gzip
import itertools
import math

import numpy as np
import pytest

import ctc_align_ref as A
import ctc_beam_ref as R
import ctc_lm_ref as L

from gigaam_amd import lm as LM

LN10 = math.log(10.0)

ARPA3 = """
\\data\\
ngram 1=6
ngram 2=4
ngram 3=2

\\1-grams:
-1.0\t<s>\t-0.5
-0.7\t</s>
-0.6\tда\t-0.3
-0.9\tнет\t-0.2
-1.2\t<unk>
-1.1\tвсе\t-0.1

\\2-grams:
-0.3\t<s> да\t-0.2
-0.4\tда нет\t-0.15
-0.5\tнет </s>
-0.2\tда все

\\3-grams:
-0.1\t<s> да нет
-0.05\tда нет </s>

\\end\\
"""


def _write(tmp_path, text, name="lm.arpa"):
    p = tmp_path / name
    if name.endswith(".gz"):
        with gzip.open(p, "wt", encoding="utf-8") as f:
            f.write(text)
    else:
        p.write_text(text, encoding="utf-8")
    return str(p)


def _no_unk(text):
    return text.replace("ngram 1=6", "ngram 1=5").replace("-1.2\t<unk>\n", "")


def test_arpa_parser_and_hand_computed_backoff(tmp_path):
    lm = LM.NgramLM.from_arpa(_write(tmp_path, ARPA3))
    assert lm.order == 3 and lm.counts == [6, 4, 2]
    assert lm.has_unk and lm.vocab[lm.unk] == "<unk>"
    # <s> да нет </s>: every n-gram listed at the top order
    assert lm.score_words(["да", "нет"]) == pytest.approx((-0.3 - 0.1 - 0.05) * LN10, abs=1e-12)
    # <s> нет: no bigram -> bo(<s>) + p(нет); нет </s>: no trigram (<s> нет </s>), no context bigram (<s> нет) -> p(нет </s>)
    assert lm.score_words(["нет"]) == pytest.approx((-0.5 - 0.9 - 0.5) * LN10, abs=1e-12)
    # <s> да все: trigram missing, bo(<s> да) + p(да все); да все </s>: bo(да все) = 0 (no such context), bo(все) + p(</s>)
    assert lm.score_words(["да", "все"]) == pytest.approx((-0.3 + (-0.2 - 0.2) + (-0.1 - 0.7)) * LN10, abs=1e-12)
    # an out-of-vocabulary word scores <unk>: <s> xyz -> bo(<s>) + p(<unk>); xyz </s> -> p(</s>) (bo(<unk>) = 0)
    assert lm.score_words(["xyz"]) == pytest.approx((-0.5 - 1.2 - 0.7) * LN10, abs=1e-12)
    assert lm.score_words(["xyz"]) == pytest.approx(L.ArpaLM(ARPA3).sentence(["xyz"]), abs=1e-12)
    # without <unk>: a fixed unk_logp (natural log), and the word still enters the history as <unk>
    lm2 = LM.NgramLM.from_arpa(_write(tmp_path, _no_unk(ARPA3), "lm2.arpa.gz"), unk_logp=-7.5)
    assert not lm2.has_unk and lm2.unk == len(lm2.vocab)
    assert lm2.score_words(["xyz"]) == pytest.approx(-7.5 + -0.7 * LN10, abs=1e-12)
    # <s> да; да <unk> -> unk_logp; (да <unk>) нет -> no trigram, no bigram (<unk> нет), p(нет); (<unk> нет) </s> -> p(нет </s>)
    assert lm2.score_words(["да", "xyz", "нет"]) == pytest.approx((-0.3 - 0.9 - 0.5) * LN10 - 7.5, abs=1e-12)
    assert lm2.score_words(["да", "xyz", "нет"]) == pytest.approx(L.ArpaLM(_no_unk(ARPA3), unk_logp=-7.5).sentence(["да", "xyz", "нет"]),
                                                                  abs=1e-12)
    # save / load keep everything
    lm.save(str(tmp_path / "lm.npz"))
    back = LM.NgramLM.open(str(tmp_path / "lm.npz"))
    assert back.vocab == lm.vocab and back.counts == lm.counts and back.unk == lm.unk
    for w in (["да", "нет"], ["все", "xyz", "да"], []):
        assert back.score_words(w) == lm.score_words(w)


def test_arpa_parser_rejects_bad_files(tmp_path):
    with pytest.raises(ValueError, match="order 6"):
        text = "\\data\\\n" + "".join(f"ngram {n}=1\n" for n in range(1, 7)) + "\n\\1-grams:\n-1\t<s>\n"
        LM.NgramLM.from_arpa(_write(tmp_path, text))
    with pytest.raises(ValueError, match="header says"):
        LM.NgramLM.from_arpa(_write(tmp_path, ARPA3.replace("ngram 2=4", "ngram 2=5")))
    with pytest.raises(ValueError, match="not a unigram"):
        LM.NgramLM.from_arpa(_write(tmp_path, ARPA3.replace("-0.2\tда все", "-0.2\tда кот")))


def _kernel_lnprob(t, lm, w, ctx):
    """ln P(w | ctx) the way gam_lm_query computes it, from the device tables (ctx: word ids, oldest first)."""
    s = list(reversed(ctx[-(lm.order - 1):])) if lm.order > 1 else []
    m = lm.order - 1
    s = s + [-1] * (4 - len(s))

    def look(ids):
        h = len(ids)
        for i in ids:
            h = (h * LM.HASH_P + i + 1) & LM.MASK64
        e = LM.probe(t["ngrams"], int(LM.mix64(np.array([h], dtype=np.uint64))[0]), t["ngram_probe"])
        return None if e is None else (float(e[2:3].view(np.float32)[0]), float(e[3:4].view(np.float32)[0]))

    bo = 0.0
    for k in range(m, -1, -1):
        if k > 0 and s[k - 1] < 0:
            continue
        ctx_k = [s[i] for i in range(k - 1, -1, -1)]
        e = look(ctx_k + [w])
        if e is not None:
            return e[0] + bo
        if k >= 1:
            b = look(ctx_k)
            bo += b[1] if b is not None else 0.0
    return lm.unk_logp


@pytest.mark.parametrize("with_unk", [True, False])
def test_device_tables_answer_every_ngram_and_backoff_path(tmp_path, with_unk):
    from gigaam_amd import synth
    from gigaam_amd.decoding import Tokenizer
    lm = LM.NgramLM.from_arpa(_write(tmp_path, ARPA3 if with_unk else _no_unk(ARPA3)))
    t = lm.device_tables(Tokenizer(synth.CHAR_VOCAB))
    for tab in ("words", "ngrams"):
        assert t[tab].dtype == np.uint32 and t[tab].shape[1] == 4
        S = t[tab].shape[0]
        assert S & (S - 1) == 0 and np.count_nonzero(t[tab][:, 0] | t[tab][:, 1]) * 2 <= S      # load <= 0.5
    # every listed n-gram, exactly its f32 values
    for ids, lnp, lnbo in lm.ngrams:
        h = LM.mix64(LM.ngram_hashes(ids))
        for r in range(ids.shape[0]):
            e = LM.probe(t["ngrams"], int(h[r]), t["ngram_probe"])
            assert e is not None
            assert e[2:3].view(np.float32)[0] == np.float32(lnp[r]) and e[3:4].view(np.float32)[0] == np.float32(lnbo[r])
    # every (context, word) over the vocabulary (contexts of length 0..2, <unk> included): the kernel's back-off = the host's
    ids = list(range(len(lm.vocab))) + ([] if lm.has_unk else [lm.unk])
    n = 0
    for L_ in range(3):
        for ctx in itertools.product(ids, repeat=L_):
            for w in ids:
                assert _kernel_lnprob(t, lm, w, list(ctx)) == pytest.approx(lm.lnprob(w, list(ctx)), abs=1e-5), (ctx, w)
                n += 1
    assert n > 200
    # a key absent from the table is reported absent within the longest chain
    assert LM.probe(t["ngrams"], 12345, t["ngram_probe"]) is None


def _sp_tokenizer(tmp_path):
    import sentencepiece as spm
    from gigaam_amd.decoding import Tokenizer
    words = "мама мыла раму папа пил чай кот спал дома".split()
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(" ".join(words[(i * 7 + j) % len(words)] for j in range(6)) for i in range(200)), encoding="utf-8")
    spm.SentencePieceTrainer.train(input=str(corpus), model_prefix=str(tmp_path / "sp"), vocab_size=26, minloglevel=2)
    return Tokenizer([], str(tmp_path / "sp.model"))


def _arpa_unigrams(words):
    lines = ["\\data\\", f"ngram 1={len(words) + 3}", "", "\\1-grams:", "-1.0\t<s>\t-0.3", "-1.0\t</s>", "-2.0\t<unk>"]
    lines += [f"-{1.0 + 0.1 * i:.2f}\t{w}\t-0.2" for i, w in enumerate(words)]
    return "\n".join(lines + ["", "\\end\\", ""])


@pytest.mark.parametrize("kind", ["charwise", "pieces", "sentencepiece"])
def test_spelling_hashes_match_the_reference(tmp_path, kind):
    from gigaam_amd import synth
    from gigaam_amd.decoding import Tokenizer
    if kind == "charwise":
        tok = Tokenizer(synth.CHAR_VOCAB)
        words, oov = ["да", "нет", "мама", "ёж", "hello"], 2               # (ё and latin letters are not in the vocabulary)
    elif kind == "pieces":
        tok = Tokenizer(synth._e2e_vocab(256))                           # "▁t0", "t1", "t2", "▁t3", ...: U+2581 starts a word
        words, oov = ["t0t1", "t3", "t12t13t14", "t1t2", "x9"], 2          # (t1 cannot start a word; x9 is no piece)
    else:
        tok = _sp_tokenizer(tmp_path)
        words, oov = ["мама", "чай", "кот", "мыла", "xyz"], 1
    lm = LM.NgramLM.from_arpa(_write(tmp_path, _arpa_unigrams(words)))
    t = lm.device_tables(tok)
    assert t["oov"] == oov
    classes = t["classes"]
    assert classes.shape[0] == len(tok) + 1
    if kind == "charwise":
        assert classes[0] == 2 and classes[1:].max() == 0
    elif kind == "pieces":
        assert classes[0] == 1 and classes[1] == 0 and classes[3] == 1
    else:
        assert all(classes[i] == (1 if tok.id_to_str(i).startswith("▁") else 0) for i in range(len(tok)))
    found = 0
    for w in words:
        sp = LM.word_spelling(tok, w, classes)
        if sp is None:
            continue
        if kind != "pieces":
            assert sp == tok.encode(w)
        else:
            assert tok.decode(sp) == "▁" + w
        key = int(LM.mix64(np.array([L.spelling_hash(sp)], dtype=np.uint64))[0])
        e = LM.probe(t["words"], key, t["word_probe"])
        assert e is not None and lm.vocab[int(e[2])] == w, w
        assert L.spelling_hash(sp) == LM.spelling_hash(sp)
        found += 1
    assert found == len(words) - oov


# ---- the reference
# V = 5: 0 "a" (continues), 1 "b" (continues), 2 " " (separator), 3 "▁c" (starts a word), blank 4
_CLS = [0, 0, 2, 1, 0]
_SPELL = {(0,): "a", (0, 1): "ab", (1,): "b", (3,): "c", (3, 0): "ca"}
_ARPA_SMALL = """
\\data\\
ngram 1=8
ngram 2=4

\\1-grams:
-1.0\t<s>\t-0.4
-0.8\t</s>
-0.5\ta\t-0.2
-0.9\tab\t-0.1
-0.7\tb\t-0.3
-0.6\tc\t-0.25
-1.3\tca
-1.5\t<unk>

\\2-grams:
-0.2\t<s> a
-0.1\ta b\t-0.05
-0.3\tc </s>
-0.15\tb c
\\end\\
"""


def _spec(alpha, beta, text=_ARPA_SMALL):
    return L.LMSpec(L.ArpaLM(text), _CLS, _SPELL, alpha, beta)


def test_reference_with_zero_weights_is_the_search_without_lm():
    rng = np.random.default_rng(3)
    for trial in range(30):
        T = int(rng.integers(1, 12))
        lp = np.log(rng.dirichlet(np.ones(5) * 0.6, size=T))
        W = [1, 2, 4, 8, None][trial % 5]
        hot = [[0, 1]] if trial % 3 == 0 else []
        a = R.beam_search(lp, W, hotwords=hot, beta=1.5)
        b = R.beam_search(lp, W, hotwords=hot, beta=1.5, lm=_spec(0.0, 0.0))
        for k in ("ids", "frames", "score", "logp", "margins", "final_margin"):
            assert a[k] == b[k], (trial, k)


def test_reference_lm_term_follows_the_word_rule():
    spec = _spec(1.0, 0.5)
    arpa = spec.lm
    # "a b ▁c" = tokens 0 1 3 -> words "ab" (0 1), then "c": <s> ab, ab c, c </s>
    assert L.words_of([0, 1, 3], _CLS) == [(0, 1), (3,)]
    want = arpa.lnprob("ab", ["<s>"]) + arpa.lnprob("c", ["<s>", "ab"]) + arpa.lnprob("</s>", ["ab", "c"]) + 2 * 0.5
    assert L.lm_term([0, 1, 3], spec) == pytest.approx(want, abs=1e-12)
    # separators and repeated separators complete nothing new; an unknown spelling is <unk>
    assert L.lm_term([2, 0, 2, 2, 1, 1, 2], spec) == pytest.approx(
        arpa.lnprob("a", ["<s>"]) + arpa.lnprob("<unk>", ["<s>", "a"]) + arpa.lnprob("</s>", ["a", "<unk>"]) + 2 * 0.5, abs=1e-12)
    assert L.lm_term([], spec) == pytest.approx(arpa.lnprob("</s>", ["<s>"]), abs=1e-12)


def _brute_map(lp, T, spec):
    V = lp.shape[1]
    best, best_y, ll_best = -np.inf, None, None
    for n in range(T + 1):
        for y in itertools.product(range(V - 1), repeat=n):
            ll = A.forward_loglik(lp, list(y), T)
            if ll == -np.inf:
                continue
            v = ll + L.lm_term(y, spec)
            if v > best:
                best, best_y, ll_best = v, list(y), ll
    return best_y, best, ll_best


def test_unbounded_beam_with_lm_is_exact_map():
    rng = np.random.default_rng(17)
    n = 0
    for alpha, beta in ((1.0, 0.5), (2.5, -1.0), (0.7, 3.0)):
        spec = _spec(alpha, beta)
        for T in (1, 2, 3, 4):
            for _ in range(3):
                lp = np.log(rng.dirichlet(np.ones(5) * 0.5, size=T))
                res = R.beam_search(lp, None, lm=spec)
                y, val, ll = _brute_map(lp, T, spec)
                assert res["ids"] == y, (alpha, beta, T, res["ids"], y)
                assert res["score"] == pytest.approx(val, abs=1e-9)
                assert res["logp"] == pytest.approx(ll, abs=1e-9)
                assert res["lm"] == pytest.approx(L.lm_term(y, spec), abs=1e-9)
                n += 1
    assert n == 36


def test_transcribe_lm_needs_a_ctc_head(tmp_path):
    import gigaam_amd
    from gigaam_amd import synth
    model = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_rnnt", seed=1, n_layers=1), "cpu")
    wav, wlen = synth.synth_audio(1, 1.0, seed=3)
    lm = LM.NgramLM.from_arpa(_write(tmp_path, ARPA3))
    for kw in (dict(lm=lm), dict(lm=_write(tmp_path, ARPA3, "x.arpa"), lm_weight=1.0), dict(lm=lm, beam_size=4, word_bonus=0.0)):
        with pytest.raises(TypeError, match="beam search needs a CTC head"):
            model.transcribe_batch(wav, wlen, **kw)
        with pytest.raises(TypeError, match="beam search needs a CTC head"):
            model.launch_batch(wav, wlen, **kw)
        with pytest.raises(TypeError, match="beam search needs a CTC head"):
            model.transcribe("no-such-file.wav", **kw)
        with pytest.raises(TypeError, match="beam search needs a CTC head"):
            model.transcribe_longform("no-such-file.wav", speech_regions=[(0.0, 1.0)], **kw)
    assert gigaam_amd.NgramLM is LM.NgramLM
