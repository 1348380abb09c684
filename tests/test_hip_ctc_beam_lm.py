"""GPU: CTC prefix beam search with a word n-gram LM (gam_set_lm; gam_ctc_beam_kernel<true> of gigaam_amd/csrc/gam_beam.h) against
the float64 reference of tests/ctc_lm_ref.py -- alone and with hotwords, at V 34 / 257 / 1025 --, bit-identity with the kernel
without LM at alpha = beta = 0, an LM that flips a near-tied decision, streams, limits, the full-size 32 x 20 s batch and the model.

Margin rule (tests/test_hip_ctc_beam.py): the kernel ranks in fp32, the reference in fp64, so ids / frames are compared on the
utterances whose smallest decision margin exceeds MARGIN; the op-level tests require at least 90 % of them to qualify.  score /
logp are compared on those utterances within 1e-3 * max(1, |ref|)."""
import numpy as np
import pytest
import torch

from beam_common import arpa as _arpa, ctc_hotwords as _hotwords, ctc_op_engine, fullsize_ctc_model as _fullsize_model
from beam_common import bar as _bar, compare, log_probs as _log_probs, run_ctc_op as _run, tokenizer as _tokenizer, wav_file as _wav_file
from common import report

import ctc_lm_ref as L
import ctc_beam_ref as R

pytestmark = pytest.mark.gpu

MARGIN = 2e-5
MARGIN_LONG = 1e-4


def _op_engine():
    return ctc_op_engine(__name__)


def _compare(h, b, ref, errs, margin):
    return compare(h, b, ref, errs, margin, R.min_margin)


def token_classes(tok):
    from gigaam_amd.lm import token_classes as tc
    return tc(tok)


def _word_ids(rng, lp, classes, n):
    """n words (token-id tuples valid under the class rule) built from the two best non-blank ids of runs of frames -- words the
    beam meets -- and a few random ones."""
    B, T, V = lp.shape
    top2 = np.argsort(-lp[:, :, :-1], axis=2, kind="stable")[:, :, :2]
    out = set()
    piece = classes[0] != 2
    while len(out) < n:
        b, Lw = int(rng.integers(0, B)), int(rng.integers(1, 4))
        t = int(rng.integers(0, max(T - Lw, 1)))
        ids = [int(top2[b, min(t + i, T - 1), rng.integers(0, 2)]) if rng.random() < 0.8 else int(rng.integers(0, V - 1))
               for i in range(Lw)]
        if piece:   # first id starts a word (class 1: id % 3 == 0), the others continue it
            ids = [ids[0] - ids[0] % 3] + [c if classes[c] == 0 else c + 1 for c in ids[1:]]
            ids = [c for c in ids if c < V - 1]
        else:
            ids = [c for c in ids if classes[c] == 0]
        if ids:
            out.add(tuple(ids))
    return sorted(out)


def _make_lm(tmp_path, rng, tok, word_ids, order, alpha, beta, sentences=(), unk=True, name="lm.arpa"):
    """(NgramLM, LMSpec) over words spelt by ``word_ids``; every spelling round-trips through lm.word_spelling."""
    from gigaam_amd import lm as LM
    classes = LM.token_classes(tok)
    words, spell = [], {}
    for ids in word_ids:
        text = tok.decode(list(ids))
        w = text[1:] if text.startswith("▁") else text
        if w in spell.values() or not w:
            continue
        assert LM.word_spelling(tok, w, classes) == list(ids), (w, ids)
        words.append(w)
        spell[tuple(ids)] = w
    text = _arpa(rng, words, order, sentences, unk)
    p = tmp_path / name
    p.write_text(text, encoding="utf-8")
    return LM.NgramLM.from_arpa(str(p)), L.LMSpec(L.ArpaLM(text), classes, spell, alpha, beta)


@pytest.mark.parametrize("V", [34, 257, 1025])
@pytest.mark.parametrize("kind", ["peaked", "flat"])
def test_op_beam_lm_matches_float64_reference(tmp_path, V, kind):
    eng = _op_engine()
    tok = _tokenizer(V)
    rng = np.random.default_rng(V * 7 + (1 if kind == "flat" else 0))
    T, B = (24 if kind == "flat" else 40), 6
    errs, n, ok = {}, 0, 0
    for W, order, hot, unk in ((1, 2, False, True), (4, 3, False, False), (8, 3, True, True), (8, 5, False, True),
                               (32, 4, True, False)):
        lp = _log_probs(rng, B, T + 3, V, kind)
        enc_len = [T, T - 5, T, 1, T, T + 3]
        classes = token_classes(tok)
        lm, spec = _make_lm(tmp_path, rng, tok, _word_ids(rng, lp, classes, 40), order, 0.8, 0.6, unk=unk)
        phrases = _hotwords(rng, lp, 6) if hot else []
        eng.set_hotwords(phrases, 1.5)
        eng.set_lm(lm, tok, 0.8, 0.6)
        h = _run(eng, lp, enc_len, W)
        for b in range(B):
            ref = R.beam_search(lp[b], W, enc_len[b], phrases, 1.5, spec)
            ok += _compare(h, b, ref, errs, MARGIN)
            n += 1
    eng.set_lm(None)
    eng.set_hotwords([])
    report(f"ctc_beam_lm_op_{V}_{kind}", qualified=f"{ok}/{n}", **errs)
    assert ok >= 0.9 * n, (ok, n)


@pytest.mark.parametrize("V", [34, 257])
def test_op_beam_lm_with_zero_weights_is_bit_identical_to_no_lm(tmp_path, V):
    eng = _op_engine()
    tok = _tokenizer(V)
    rng = np.random.default_rng(5 + V)
    lp = _log_probs(rng, 8, 60, V, "flat")
    enc_len = [60, 50, 1, 60, 33, 60, 59, 60]
    classes = token_classes(tok)
    lm, _ = _make_lm(tmp_path, rng, tok, _word_ids(rng, lp, classes, 50), 3, 0.0, 0.0)
    for W in (1, 8, 32):
        eng.set_lm(None)
        a = _run(eng, lp, enc_len, W)
        eng.set_lm(lm, tok, 0.0, 0.0)
        b = _run(eng, lp, enc_len, W)
        assert a["rows"] == b["rows"], W
        for k in ("score", "logp"):
            assert a[k].tobytes() == b[k].tobytes(), (W, k)
    eng.set_lm(None)


def _tied_log_probs(tok):
    """Log-probs [1, 7, 34] that spell "да кот" or "та кот": д and т near-tied at frame 0 (д ahead by ~0.02)."""
    V = len(tok) + 1
    ix = {c: tok.encode(c)[0] for c in "датко "}
    rows = []
    for spec in ({"д": 0.45, "т": 0.44}, {"а": 0.95}, {" ": 0.95}, {"к": 0.95}, {"о": 0.95}, {"т": 0.95}, {}):
        p = np.full(V, 1e-4)
        for c, v in spec.items():
            p[ix[c]] = v
        p[V - 1] = max(1.0 - p[:-1].sum(), 1e-4)
        rows.append(np.log(p / p.sum()))
    return np.asarray(rows, dtype=np.float32)[None]


def test_lm_flips_a_near_tied_decision(tmp_path):
    """Without an LM the beam reads "да кот"; an ARPA that prefers "та кот" makes it win, and the swapped ARPA turns it back."""
    from gigaam_amd import lm as LM
    eng = _op_engine()
    tok = _tokenizer(34)
    lp = _tied_log_probs(tok)
    eng.set_lm(None)
    plain = _run(eng, lp, [7], 8)
    assert tok.decode(plain["rows"][0][0]) == "да кот"

    def arpa(good, bad):
        return ("\\data\\\nngram 1=5\nngram 2=3\n\n\\1-grams:\n-1.0\t<s>\t-0.3\n-1.0\t</s>\n"
                f"-1.0\t{good}\t-0.2\n-3.0\t{bad}\t-0.2\n-1.0\tкот\t-0.2\n\n\\2-grams:\n"
                f"-0.2\t<s> {good}\n-0.3\t{good} кот\n-0.2\tкот </s>\n\\end\\\n")

    for good, bad in (("та", "да"), ("да", "та")):
        p = tmp_path / f"{good}.arpa"
        p.write_text(arpa(good, bad), encoding="utf-8")
        lm = LM.NgramLM.from_arpa(str(p))
        eng.set_lm(lm, tok, 0.5, 1.0)
        h = _run(eng, lp, [7], 8)
        assert tok.decode(h["rows"][0][0]) == f"{good} кот", (good, h["rows"][0])
        spec = L.LMSpec(L.ArpaLM(arpa(good, bad)), LM.token_classes(tok), {tuple(tok.encode(w)): w for w in ("да", "та", "кот")},
                        0.5, 1.0)
        ref = R.beam_search(lp[0], 8, 7, lm=spec)
        assert ref["ids"] == h["rows"][0][0]
        assert abs(float(h["score"][0]) - ref["score"]) <= 1e-4 and abs(float(h["logp"][0]) - ref["logp"]) <= 1e-4
        assert float(h["score"][0]) != float(h["logp"][0])
    eng.set_lm(None)


def test_op_beam_lm_is_bit_identical_on_another_stream(tmp_path):
    eng = _op_engine()
    tok = _tokenizer(257)
    rng = np.random.default_rng(9)
    lp = _log_probs(rng, 4, 120, 257, "flat")
    classes = token_classes(tok)
    lm, _ = _make_lm(tmp_path, rng, tok, _word_ids(rng, lp, classes, 60), 4, 1.0, 0.5)
    eng.set_lm(lm, tok, 1.0, 0.5)
    eng.set_hotwords(_hotwords(rng, lp, 10), 1.0)
    a = _run(eng, lp, [120, 100, 120, 7], 8)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        b = _run(eng, lp, [120, 100, 120, 7], 8)
    torch.cuda.synchronize()
    eng.set_lm(None)
    eng.set_hotwords([])
    assert a["rows"] == b["rows"]
    for k in ("score", "logp"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_library_rejects_lm_beyond_the_limits():
    from gigaam_amd._lib import GigaAMHipError
    eng = _op_engine()
    V = 5
    cls = np.zeros(V, dtype=np.int32)
    tab = np.zeros((16, 4), dtype=np.uint32)

    def call(cls_=cls, order=3, slots=16, probe=1, v=V):
        return eng.lib.gam_set_lm(eng._h, cls_.ctypes.data, v, tab.ctypes.data, slots, probe, tab.ctypes.data, slots, probe, order, 0, 1,
                                  2, -10.0, 0.5, 1.0)

    rc = call(order=6)
    assert rc != 0 and b"order 6" in eng.lib.gam_last_error(eng._h)
    bad = cls.copy()
    bad[2] = 3
    rc = call(cls_=bad)
    assert rc != 0 and b"token class 3" in eng.lib.gam_last_error(eng._h)
    rc = call(slots=12)
    assert rc != 0 and b"powers of two" in eng.lib.gam_last_error(eng._h)
    rc = call(probe=0)
    assert rc != 0 and b"probe" in eng.lib.gam_last_error(eng._h)
    assert call() == 0                          # an empty LM for V = 5: a search with another V is refused
    with pytest.raises(GigaAMHipError, match="V=5"):
        eng.op_ctc_beam(torch.zeros((1, 4, 7)), torch.tensor([4], dtype=torch.int32), 4)
    assert eng.lib.gam_set_lm(eng._h, None, 0, None, 0, 0, None, 0, 0, 0, 0, 0, 0, -10.0, 0.0, 0.0) == 0     # (cleared)
    eng.op_ctc_beam(torch.zeros((1, 4, 7)), torch.tensor([4], dtype=torch.int32), 4).host()


def test_fullsize32_transcribe_batch_lm_matches_reference(tmp_path):
    """The 32 x 20 s, 16-layer batch with an LM built from the batch's own greedy transcripts (so lookups hit every order) plus
    random words: transcribe_batch(lm=...) against the reference on the head's log-probs.  Also times the beam kernel alone."""
    from gigaam_amd import lm as LM
    from gigaam_amd import workloads
    model = _fullsize_model()
    wav, wlen = workloads.config2_batch(32, 20.0, rank=0)
    greedy = [t for t, _ in model.transcribe_batch(wav, wlen)]
    tok = model.decoding.tokenizer
    rng = np.random.default_rng(1)
    sents = [t.split() for t in greedy]
    vocab = sorted({w for s in sents for w in s})
    letters = [c for c in tok.vocab if c != " "]
    vocab += ["".join(rng.choice(letters, int(rng.integers(2, 6)))) for _ in range(200)]
    vocab = sorted(set(vocab))
    text = _arpa(rng, vocab, 3, sents)
    p = tmp_path / "batch.arpa"
    p.write_text(text, encoding="utf-8")
    lm = LM.NgramLM.from_arpa(str(p))
    spec = L.LMSpec(L.ArpaLM(text), LM.token_classes(tok), {tuple(tok.encode(w)): w for w in vocab}, 0.5, 1.0)
    got = model.transcribe_batch(wav, wlen, lm=lm)
    eng = model.head.engine
    with torch.inference_mode():
        enc, elen = model._encode(wav.to("cuda:0"), wlen.to("cuda:0"), wlen)
        lp_d = eng.ctc_head(enc)
    lp = lp_d.double().cpu().numpy()
    el = elen.cpu().tolist()
    ok = 0
    for b in range(32):
        ref = R.beam_search(lp[b], 8, el[b], lm=spec)
        if R.min_margin(ref) <= MARGIN_LONG:
            continue
        ok += 1
        assert got[b][0] == tok.decode(ref["ids"]), b
    for _ in range(2):
        eng.op_ctc_beam(lp_d, elen, 8)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        eng.op_ctc_beam(lp_d, elen, 8)
    e1.record()
    torch.cuda.synchronize()
    report("ctc_beam_lm_fullsize32", qualified=f"{ok}/32", ngrams=lm.counts, op_beam_lm_w8_ms=e0.elapsed_time(e1) / 5)
    assert ok >= 16, ok


def test_model_lm_transcribe_batch_longform_and_greedy_default(tmp_path):
    """transcribe(lm=path), transcribe_batch(lm=...) on mixed lengths against the reference, transcribe_longform(lm=...), and
    every call without the beam options stays greedy."""
    import gigaam_amd
    from gigaam_amd import lm as LM
    from gigaam_amd import synth
    model = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=1, n_layers=2), "cuda:0")
    tok = model.decoding.tokenizer
    wav, wlen = synth.synth_audio(3, 4.0, seed=7, lengths=[64000, 41000, 23000])
    greedy = [t for t, _ in model.transcribe_batch(wav, wlen)]
    wpath = _wav_file(tmp_path, 6.0, 13)
    regions = [(0.0, 2.5), (2.5, 6.0)]
    lf_greedy = [s.text for s in model.transcribe_longform(wpath, speech_regions=regions).segments]
    rng = np.random.default_rng(2)
    sents = [t.split() for t in greedy]
    vocab = sorted({w for s in sents for w in s} | {"да", "нет"})
    text = _arpa(rng, vocab, 3, sents)
    path = tmp_path / "m.arpa"
    path.write_text(text, encoding="utf-8")
    lm = LM.NgramLM.from_arpa(str(path))
    spec = L.LMSpec(L.ArpaLM(text), LM.token_classes(tok), {tuple(tok.encode(w)): w for w in vocab}, 0.7, 0.5)
    got = model.transcribe_batch(wav, wlen, lm=lm, lm_weight=0.7, word_bonus=0.5, word_timestamps=True)
    assert model.head.engine._lm_key is not None
    with torch.inference_mode():
        enc, elen = model._encode(wav.to("cuda:0"), wlen.to("cuda:0"), wlen)
        lp = model.head.engine.ctc_head(enc).double().cpu().numpy()
        dec = model.decoding.decode_beam(model.head, enc, elen, lm=lm, lm_weight=0.7, word_bonus=0.5)
    el = elen.cpu().tolist()
    ok = 0
    for b in range(3):
        ref = R.beam_search(lp[b], 8, el[b], lm=spec)
        assert dec[b][0] == got[b][0]
        if R.min_margin(ref) <= MARGIN_LONG:
            continue
        ok += 1
        assert got[b][0] == tok.decode(ref["ids"]), b
        assert abs(dec[b][3] - ref["score"]) <= _bar(ref["score"]) and abs(dec[b][4] - ref["logp"]) <= _bar(ref["logp"])
        assert all(w.start <= w.end for w in got[b][1])
    assert ok >= 2, ok
    # a path (ARPA or .npz) works as the model; lm alone means beam_size=8
    lm.save(str(tmp_path / "m.npz"))
    r1 = model.transcribe(wpath, lm=str(path), lm_weight=0.7, word_bonus=0.5)
    r2 = model.transcribe(wpath, lm=str(tmp_path / "m.npz"), lm_weight=0.7, word_bonus=0.5, beam_size=8)
    assert r1.text == r2.text
    lf = model.transcribe_longform(wpath, speech_regions=regions, lm=lm, word_timestamps=True)
    assert len(lf.segments) >= 1 and all(s.words is not None for s in lf.segments)
    # the greedy default is untouched by an LM held on the engine
    assert [t for t, _ in model.transcribe_batch(wav, wlen)] == greedy
    assert [s.text for s in model.transcribe_longform(wpath, speech_regions=regions).segments] == lf_greedy
    plain = model.transcribe_batch(wav, wlen, beam_size=8)
    assert model.head.engine._lm_key is None
    assert len(plain) == 3
