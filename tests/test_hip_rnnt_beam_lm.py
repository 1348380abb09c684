"""GPU: RNN-T beam search with a word n-gram LM (gam_set_lm; gam_rnnt_beam_kernel<true> of gigaam_amd/csrc/gam_rnnt_beam.h) against
the float64 reference of tests/rnnt_beam_ref.py -- alone and with hotwords, at V 34 / 257 / 1025 and L 1 / 2 --, bit-identity with the
kernel without LM at alpha = beta = 0, an LM that flips a near-tied decision, streams, limits, the full-size 32 x 20 s batch and the
model (set_decoding).

Margin rule (tests/test_hip_rnnt_beam.py): the kernel ranks in fp32, the reference in fp64, so ids / frames are compared on the
utterances whose smallest decision margin exceeds MARGIN; the op-level test requires at least 90 % of them to qualify.  score /
logp are compared on those utterances within 1e-3 * max(1, |ref|)."""
import numpy as np
import pytest
import torch

from beam_common import arpa as _arpa, bar as _bar, compare, encp as _encp, fullsize_rnnt_model as _fullsize_model
from beam_common import run_rnnt_op as _run_op, small_rnnt_model as _small_rnnt_model, tokenizer as _tokenizer, wav_file as _wav_file
from common import report

import ctc_lm_ref as CL
import rnnt_beam_ref as R

pytestmark = pytest.mark.gpu

MARGIN = 1e-4
MARGIN_LONG = 5e-4


_ENGINES = {}


def _compare(h, b, ref, errs, margin):
    return compare(h, b, ref, errs, margin, R.min_margin)


def _engine(V, L=1, H=320, blank_bias=None):
    """An engine with a synthetic RNN-T head (one encoder layer): V classes, L predictor layers, pred_hidden = joint_hidden = H."""
    key = (V, L, H, blank_bias)
    if key not in _ENGINES:
        from gigaam_amd import synth
        from gigaam_amd.engine import HipEngine, build_config
        cfg = synth.model_cfg("v3_e2e_rnnt" if V > 34 else "v2_rnnt", n_layers=1)
        cfg["head"]["decoder"]["num_classes"] = cfg["head"]["joint"]["num_classes"] = V
        cfg["head"]["decoder"]["pred_rnn_layers"] = L
        cfg["head"]["decoder"]["pred_hidden"] = cfg["head"]["joint"]["pred_hidden"] = cfg["head"]["joint"]["joint_hidden"] = H
        sd = synth.make_state_dict(cfg, seed=V + L + 3, rnnt_blank_bias=blank_bias)
        eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), sd, torch.device("cuda:0"))
        _ENGINES[key] = (eng, R.head_from_state_dict(sd, L), cfg, sd)
    return _ENGINES[key]


def _words(tok, classes, id_lists, rng, n_random):
    """Words (token-id tuples whose text spells back to them: lm.word_spelling) of the given id lists, plus random valid ones."""
    from gigaam_amd import lm as LM
    V = len(classes)
    start = [c for c in range(V - 1) if classes[c] == 1]
    cont = [c for c in range(V - 1) if classes[c] == 0]
    cands = [w for ids in id_lists for w in CL.words_of(ids, classes)]
    for _ in range(n_random):
        k = int(rng.integers(0, 3))
        cands.append(tuple(([int(rng.choice(start))] if start else [int(rng.choice(cont))]) + [int(rng.choice(cont)) for _ in range(k)]))
    out = {}
    for ids in cands:
        text = tok.decode(list(ids))
        w = text[1:] if text.startswith("▁") else text
        if w and w not in out.values() and " " not in w and LM.word_spelling(tok, w, classes) == list(ids):
            out[tuple(ids)] = w
    return out


def _make_lm(tmp_path, rng, tok, id_lists, order, alpha, beta, unk=True, name="lm.arpa"):
    """(NgramLM, LMSpec): the words of ``id_lists`` and random ones; the id lists' word sequences as sentences (n-grams that hit)."""
    from gigaam_amd import lm as LM
    classes = [int(c) for c in LM.token_classes(tok)]
    spell = _words(tok, classes, id_lists, rng, 30)
    sents = [[spell[w] for w in CL.words_of(ids, classes) if w in spell] for ids in id_lists]
    text = _arpa(rng, sorted(spell.values()), order, [s for s in sents if s], unk)
    p = tmp_path / name
    p.write_text(text, encoding="utf-8")
    return LM.NgramLM.from_arpa(str(p)), CL.LMSpec(CL.ArpaLM(text), classes, spell, alpha, beta)


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("V", [34, 257, 1025])
def test_op_beam_lm_matches_float64_reference(tmp_path, V, L):
    """Seeded encp; W in {1, 4, 8, 32} x S in {1, 3, 10}, LM orders 2-5, with and without hotwords and an <unk> unigram; the LM's
    words and sentences come from the search without LM, so its lookups hit every order."""
    eng, head, cfg, _ = _engine(V, L)
    JH = cfg["head"]["joint"]["joint_hidden"]
    tok = _tokenizer(V)
    rng = np.random.default_rng(V * 11 + L)
    B = 4
    errs, n, ok = {}, 0, 0
    for W, S, order, hot, unk in ((1, 3, 2, False, True), (4, 1, 3, True, False), (4, 10, 5, False, True), (8, 3, 4, True, True),
                                  (8, 10, 3, False, False), (32, 1, 2, True, True), (32, 3, 5, False, True)):
        T = 10 if W >= 8 else 16
        encp = _encp(rng, B, T, JH)
        enc_len = [T, T - 3, 1, T]
        plain = [R.beam_search(head, encp[b].astype(np.float64), W, S, enc_len[b])["ids"] for b in range(B)]
        lm, spec = _make_lm(tmp_path, rng, tok, plain, order, 0.8, 0.6, unk=unk)
        phrases = [p[:3] for p in plain if p][:4] if hot else []
        eng.set_hotwords(phrases, 1.5)
        eng.set_lm(lm, tok, 0.8, 0.6)
        h = _run_op(eng, encp, enc_len, W, S)
        for b in range(B):
            ref = R.beam_search(head, encp[b].astype(np.float64), W, S, enc_len[b], phrases, 1.5, lm=spec)
            ok += _compare(h, b, ref, errs, MARGIN)
            n += 1
    eng.set_lm(None)
    eng.set_hotwords([])
    report(f"rnnt_beam_lm_op_{V}_L{L}", qualified=f"{ok}/{n}", **errs)
    assert ok >= 0.9 * n, (ok, n)


@pytest.mark.parametrize("V", [34, 257])
def test_op_beam_lm_with_zero_weights_is_bit_identical_to_no_lm(tmp_path, V):
    eng, head, cfg, _ = _engine(V, 1)
    tok = _tokenizer(V)
    rng = np.random.default_rng(17 + V)
    encp = _encp(rng, 6, 30, cfg["head"]["joint"]["joint_hidden"])
    enc_len = [30, 25, 1, 30, 12, 30]
    plain = [R.beam_search(head, encp[b].astype(np.float64), 4, 3, enc_len[b])["ids"] for b in range(2)]
    lm, _ = _make_lm(tmp_path, rng, tok, plain, 3, 0.0, 0.0)
    eng.set_hotwords([[1, 2], [3]], 1.0)
    for W, S in ((1, 1), (4, 3), (8, 10), (32, 2)):
        eng.set_lm(None)
        a = _run_op(eng, encp, enc_len, W, S)
        eng.set_lm(lm, tok, 0.0, 0.0)
        b = _run_op(eng, encp, enc_len, W, S)
        assert a["rows"] == b["rows"], (W, S)
        for k in ("score", "logp"):
            assert a[k].tobytes() == b[k].tobytes(), (W, S, k)
    eng.set_lm(None)
    eng.set_hotwords([])


def _direct_engine():
    """V = 34 with the joint made a table lookup: W_pred = 0, b_pred = 0, W_out = [I | 0], b_out = 0, so lp(t, y) =
    log_softmax(relu(encp[t, :34])) whatever y -- the test writes the joint's log-probs (shifted positive) into encp."""
    if "direct" not in _ENGINES:
        from gigaam_amd import synth
        from gigaam_amd.engine import HipEngine, build_config
        cfg = synth.model_cfg("v2_rnnt", n_layers=1)
        sd = synth.make_state_dict(cfg, seed=2)
        JH, V = cfg["head"]["joint"]["joint_hidden"], 34
        sd["head.joint.pred.weight"] = torch.zeros_like(sd["head.joint.pred.weight"])
        sd["head.joint.pred.bias"] = torch.zeros_like(sd["head.joint.pred.bias"])
        sd["head.joint.joint_net.1.weight"] = torch.eye(V, JH)
        sd["head.joint.joint_net.1.bias"] = torch.zeros(V)
        eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), sd, torch.device("cuda:0"))
        _ENGINES["direct"] = (eng, R.head_from_state_dict(sd, 1), cfg, sd)
    return _ENGINES["direct"]


def _tied_encp(tok, JH):
    """encp [1, 7, JH] whose joint spells "да кот" or "та кот" at one symbol per frame: д and т near-tied at frame 0 (д ahead)."""
    V = len(tok) + 1
    ix = {c: tok.encode(c)[0] for c in "датко "}
    rows = np.zeros((7, JH), dtype=np.float32)
    for t, spec in enumerate(({"д": 0.45, "т": 0.44}, {"а": 0.95}, {" ": 0.95}, {"к": 0.95}, {"о": 0.95}, {"т": 0.95}, {})):
        p = np.full(V, 1e-4)
        for c, v in spec.items():
            p[ix[c]] = v
        p[V - 1] = max(1.0 - p[:-1].sum(), 1e-4)
        rows[t, :V] = np.log(p / p.sum()) + 20.0
    return rows[None]


def test_lm_flips_a_near_tied_decision(tmp_path):
    """Without an LM the beam reads "да кот"; an ARPA that prefers "та кот" makes it win, and the swapped ARPA turns it back."""
    from gigaam_amd import lm as LM
    eng, head, cfg, _ = _direct_engine()
    tok = _tokenizer(34)
    encp = _tied_encp(tok, cfg["head"]["joint"]["joint_hidden"])
    eng.set_lm(None)
    plain = _run_op(eng, encp, [7], 8, 1)
    assert tok.decode(plain["rows"][0][0]) == "да кот"

    def arpa(good, bad):
        return ("\\data\\\nngram 1=5\nngram 2=3\n\n\\1-grams:\n-1.0\t<s>\t-0.3\n-1.0\t</s>\n"
                f"-1.0\t{good}\t-0.2\n-3.0\t{bad}\t-0.2\n-1.0\tкот\t-0.2\n\n\\2-grams:\n"
                f"-0.2\t<s> {good}\n-0.3\t{good} кот\n-0.2\tкот </s>\n\\end\\\n")

    for good, bad in (("та", "да"), ("да", "та")):
        p = tmp_path / f"{good}.arpa"
        p.write_text(arpa(good, bad), encoding="utf-8")
        eng.set_lm(LM.NgramLM.from_arpa(str(p)), tok, 0.5, 1.0)
        h = _run_op(eng, encp, [7], 8, 1)
        assert tok.decode(h["rows"][0][0]) == f"{good} кот", (good, h["rows"][0])
        spec = CL.LMSpec(CL.ArpaLM(arpa(good, bad)), LM.token_classes(tok), {tuple(tok.encode(w)): w for w in ("да", "та", "кот")},
                         0.5, 1.0)
        ref = R.beam_search(head, encp[0].astype(np.float64), 8, 1, 7, lm=spec)
        assert ref["ids"] == h["rows"][0][0] and ref["frames"] == h["rows"][0][1]
        assert abs(float(h["score"][0]) - ref["score"]) <= 1e-4 and abs(float(h["logp"][0]) - ref["logp"]) <= 1e-4
        assert float(h["score"][0]) != float(h["logp"][0])
    eng.set_lm(None)


def test_op_beam_lm_is_bit_identical_run_to_run_and_on_another_stream(tmp_path):
    eng, head, cfg, _ = _engine(257, 2)
    tok = _tokenizer(257)
    rng = np.random.default_rng(9)
    encp = _encp(rng, 4, 60, cfg["head"]["joint"]["joint_hidden"])
    plain = [R.beam_search(head, encp[b].astype(np.float64), 4, 3, 30)["ids"] for b in range(2)]
    lm, _ = _make_lm(tmp_path, rng, tok, plain, 4, 1.0, 0.5)
    eng.set_lm(lm, tok, 1.0, 0.5)
    eng.set_hotwords([[1, 2], [5], [7, 7, 3]], 1.0)
    a = _run_op(eng, encp, [60, 45, 60, 7], 8, 10)
    b = _run_op(eng, encp, [60, 45, 60, 7], 8, 10)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = _run_op(eng, encp, [60, 45, 60, 7], 8, 10)
    torch.cuda.synchronize()
    eng.set_lm(None)
    eng.set_hotwords([])
    for o in (b, c):
        assert a["rows"] == o["rows"]
        for k in ("score", "logp"):
            assert a[k].tobytes() == o[k].tobytes(), k


def test_library_rejects_rnnt_beam_lm_beyond_the_limits(tmp_path):
    from gigaam_amd._lib import GigaAMHipError
    eng, _, cfg, _ = _engine(34, 1)
    JH = cfg["head"]["joint"]["joint_hidden"]
    one = torch.tensor([4], dtype=torch.int32)
    # an LM whose classes are for V = 5: the search on a V = 34 model is refused
    cls = np.zeros(5, dtype=np.int32)
    tab = np.zeros((16, 4), dtype=np.uint32)
    assert eng.lib.gam_set_lm(eng._h, cls.ctypes.data, 5, tab.ctypes.data, 16, 1, tab.ctypes.data, 16, 1, 3, 0, 1, 2, -10.0, 0.5,
                              1.0) == 0
    with pytest.raises(GigaAMHipError, match="V=5"):
        eng.op_rnnt_beam(torch.zeros((1, 4, JH)), one, 4, 10)
    assert eng.lib.gam_set_lm(eng._h, None, 0, None, 0, 0, None, 0, 0, 0, 0, 0, 0, -10.0, 0.0, 0.0) == 0     # (cleared)
    eng.op_rnnt_beam(torch.zeros((1, 4, JH)), one, 4, 10).host()
    # H = JH = 512, L = 2, W = 32, S = 10: 152048 bytes of LDS without the LM, 167072 with it
    big, _, _, _ = _engine(34, 2, H=512)
    tok = _tokenizer(34)
    lm, _ = _make_lm(tmp_path, np.random.default_rng(3), tok, [tok.encode("да кот")], 3, 0.5, 1.0)
    enc = torch.zeros((1, 4, 512))
    big.op_rnnt_beam(enc, one, 32, 10).host()
    big.set_lm(lm, tok, 0.5, 1.0)
    with pytest.raises(GigaAMHipError, match="with the LM need 167072 bytes"):
        big.op_rnnt_beam(enc, one, 32, 10)
    big.op_rnnt_beam(enc, one, 32, 4).host()
    big.set_lm(None)


def test_every_width_and_max_symbols_is_accepted_at_the_head_shapes_with_lm_and_1024_hotwords(tmp_path):
    """H = JH = 320, L = 2, V = 1025 with the LM and 1024 hotword phrases: every W <= 32 and S <= 16 runs."""
    eng, _, cfg, _ = _engine(1025, 2)
    tok = _tokenizer(1025)
    rng = np.random.default_rng(4)
    encp = _encp(rng, 2, 3, cfg["head"]["joint"]["joint_hidden"])
    lm, _ = _make_lm(tmp_path, rng, tok, [[int(c) for c in rng.integers(0, 1024, 12)]], 4, 0.5, 1.0)
    eng.set_lm(lm, tok, 0.5, 1.0)
    eng.set_hotwords([[int(c) for c in rng.integers(0, 1024, int(rng.integers(1, 4)))] for _ in range(1024)], 1.0)
    n = 0
    for W in range(1, 33):
        for S in range(1, 17):
            h = _run_op(eng, encp, [3, 2], W, S)
            assert all(len(i) <= 3 * S for i, _ in h["rows"]) and np.isfinite(h["score"]).all()
            n += 1
    eng.set_lm(None)
    eng.set_hotwords([])
    assert n == 512


def test_fullsize32_transcribe_batch_beam_lm_matches_reference(tmp_path):
    """32 x 20 s v2_rnnt at W = 4 with an LM built from the batch's own greedy transcripts plus random words (set_decoding(lm=...))
    against the reference on the GPU encoder's output.  Also times the beam kernel alone with and without the LM."""
    from gigaam_amd import lm as LM
    from gigaam_amd import workloads
    model, sd = _fullsize_model()
    wav, wlen = workloads.config2_batch(32, 20.0, rank=0)
    greedy = [t for t, _ in model.transcribe_batch(wav, wlen)]
    tok = model.decoding.tokenizer
    rng = np.random.default_rng(1)
    sents = [t.split() for t in greedy]
    vocab = sorted({w for s in sents for w in s})
    letters = [c for c in tok.vocab if c != " "]
    vocab = sorted(set(vocab + ["".join(rng.choice(letters, int(rng.integers(2, 6)))) for _ in range(200)]))
    text = _arpa(rng, vocab, 3, sents)
    p = tmp_path / "batch.arpa"
    p.write_text(text, encoding="utf-8")
    lm = LM.NgramLM.from_arpa(str(p))
    spec = CL.LMSpec(CL.ArpaLM(text), LM.token_classes(tok), {tuple(tok.encode(w)): w for w in vocab}, 0.5, 1.0)
    model.set_decoding(beam_size=4, lm=lm)
    got = model.transcribe_batch(wav, wlen)
    eng = model.head.engine
    with torch.inference_mode():
        enc, elen = model._encode(wav.to("cuda:0"), wlen.to("cuda:0"), wlen)
    head = R.head_from_state_dict(sd, 1)
    encd = enc.double().cpu().numpy()
    el = elen.cpu().tolist()
    ok = 0
    for b in range(32):
        ref = R.beam_search(head, R.encoder_projection(head, encd[b]), 4, 10, el[b], lm=spec)
        if R.min_margin(ref) <= MARGIN_LONG:
            continue
        ok += 1
        assert got[b][0] == tok.decode(ref["ids"]), b
    times = {}
    for key, use in (("beam_w4_ms", None), ("beam_lm_w4_ms", lm)):
        eng.set_lm(use, tok, 0.5, 1.0)
        for _ in range(2):
            eng.rnnt_beam(enc, elen, 4, 10)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            eng.rnnt_beam(enc, elen, 4, 10)
        e1.record()
        torch.cuda.synchronize()
        times[key] = e0.elapsed_time(e1) / 3
    report("rnnt_beam_lm_fullsize32", qualified=f"{ok}/32", ngrams=lm.counts, **times)
    assert ok >= 16, ok


def test_model_set_decoding_lm_paths_and_greedy_restore(tmp_path):
    """set_decoding(lm=...) with an NgramLM, an .arpa path and an .npz path (alone: width 4), a cfg target naming an LM;
    transcribe, transcribe_batch(word_timestamps=True) and transcribe_longform decode with it (decode_beam's score includes the LM
    term and matches the reference); set_decoding() restores greedy output byte for byte; per-call lm= stays CTC-only."""
    from gigaam_amd import lm as LM
    from gigaam_amd import synth
    from gigaam_amd.decoding import RNNTBeamDecoding
    model, sd = _small_rnnt_model()
    fresh, _ = _small_rnnt_model()
    tok = model.decoding.tokenizer
    wpath = _wav_file(tmp_path, 6.0, 43)
    wav, wlen = synth.synth_audio(3, 4.0, seed=5, lengths=[64000, 41000, 23000])
    regions = [(0.0, 2.5), (2.5, 6.0)]
    greedy = (fresh.transcribe(wpath, word_timestamps=True), fresh.transcribe_batch(wav, wlen, word_timestamps=True),
              fresh.transcribe_longform(wpath, speech_regions=regions, word_timestamps=True))
    model.set_decoding(beam_size=4)
    plain = [t for t, _ in model.transcribe_batch(wav, wlen)]
    rng = np.random.default_rng(2)
    sents = [t.split() for t in plain]
    vocab = sorted({w for s in sents for w in s} | {"да", "нет"})
    text = _arpa(rng, vocab, 3, [s for s in sents if s])
    path = tmp_path / "m.arpa"
    path.write_text(text, encoding="utf-8")
    lm = LM.NgramLM.from_arpa(str(path))
    lm.save(str(tmp_path / "m.npz"))
    spec = CL.LMSpec(CL.ArpaLM(text), LM.token_classes(tok), {tuple(tok.encode(w)): w for w in vocab}, 0.7, 0.5)
    model.set_decoding(lm=lm, lm_weight=0.7, word_bonus=0.5)
    assert isinstance(model.decoding, RNNTBeamDecoding) and model.decoding.beam_size == 4
    batch = model.transcribe_batch(wav, wlen, word_timestamps=True)
    assert model.head.engine._lm_key is not None
    with torch.inference_mode():
        enc, elen = model._encode(wav.to("cuda:0"), wlen.to("cuda:0"), wlen)
        dec = model.decoding.decode_beam(model.head, enc, elen)
    head = R.head_from_state_dict(sd, 1)
    encd = enc.double().cpu().numpy()
    el = elen.cpu().tolist()
    ok = 0
    for b in range(3):
        assert dec[b][0] == batch[b][0]
        assert all(w.start <= w.end for w in batch[b][1])
        ref = R.beam_search(head, R.encoder_projection(head, encd[b]), 4, 10, el[b], lm=spec)
        if R.min_margin(ref) <= MARGIN_LONG:
            continue
        ok += 1
        assert dec[b][0] == tok.decode(ref["ids"]), b
        assert abs(dec[b][3] - ref["score"]) <= _bar(ref["score"]) and abs(dec[b][4] - ref["logp"]) <= _bar(ref["logp"])
    assert ok >= 2, ok
    r0 = model.transcribe(wpath, word_timestamps=True)
    model.set_decoding(lm=str(path), lm_weight=0.7, word_bonus=0.5)
    r1 = model.transcribe(wpath, word_timestamps=True)
    model.set_decoding(lm=str(tmp_path / "m.npz"), lm_weight=0.7, word_bonus=0.5)
    r2 = model.transcribe(wpath, word_timestamps=True)
    assert r0.text == r1.text == r2.text and r0.words is not None
    lf = model.transcribe_longform(wpath, speech_regions=regions, word_timestamps=True)
    assert len(lf.segments) == len(greedy[2].segments) >= 1 and all(s.words is not None for s in lf.segments)
    with pytest.raises(TypeError):
        model.transcribe(wpath, lm=lm)
    cfgm, _ = _small_rnnt_model({"_target_": "gigaam.decoding.RNNTBeamDecoding", "vocabulary": synth.CHAR_VOCAB,
                                 "max_symbols_per_step": 10, "beam_size": 4, "lm": str(path), "lm_weight": 0.7, "word_bonus": 0.5})
    assert cfgm.transcribe(wpath).text == r0.text
    model.set_decoding()
    again = (model.transcribe(wpath, word_timestamps=True), model.transcribe_batch(wav, wlen, word_timestamps=True),
             model.transcribe_longform(wpath, speech_regions=regions, word_timestamps=True))
    assert repr(again) == repr(greedy)
