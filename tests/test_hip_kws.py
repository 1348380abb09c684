"""GPU: keyword search over CTC log-probs (gam_op_ctc_kws / gam_ctc_kws, gigaam_amd/csrc/gam_kws.h) against the float64 reference
of tests/kws_ref.py: the per-frame scores and starts, the hit rule applied to the kernel's own rows, exact ties, planted
occurrences, truncation, padding, streams, the library's errors, the golden CTC cases and the model API."""
import math
import os

import numpy as np
import pytest
import torch

from common import ROOT, load_case, make_engine, report

import kws_inputs as I
import kws_ref as R

pytestmark = pytest.mark.gpu

MODES = ["f16x3", "f32"]
THRESHOLDS = [0.5, 0.1, 0.9]


def _bar(ref):
    return 1e-3 * max(1.0, abs(ref))


_OP_ENGINE = []


def _op_engine():
    if not _OP_ENGINE:
        from gigaam_amd import synth
        _OP_ENGINE.append(make_engine(synth.model_cfg("v2_ctc"), {}, head=False))
    return _OP_ENGINE[0]


def _min_scores(kws, thr):
    from gigaam_amd.decoding import keyword_min_scores
    return keyword_min_scores([len(y) for y in kws], thr)


def _run(eng, lp, enc_len, kws, thr=0.5, max_hits=8, dense=True):
    eng.set_keywords(kws, _min_scores(kws, thr))
    return eng.op_ctc_kws(torch.from_numpy(np.ascontiguousarray(lp)), torch.tensor(enc_len, dtype=torch.int32), max_hits, dense).host()


def _check_hits_are_the_rule(h, enc_len, kws, thr, max_hits):
    """Check 2: the hit outputs equal the streaming rule applied to the kernel's own dense rows, exactly."""
    ms = _min_scores(kws, thr)
    for b, T in enumerate(enc_len):
        for k in range(len(kws)):
            E, S = h["dense_score"][b, k], h["dense_start"][b, k]
            assert (E[T:] == -np.inf).all() and (S[T:] == -1).all(), (b, k)
            hits, n = R.pick(E[:T], S[:T], ms[k], max_hits)
            assert int(h["n_hits"][b, k]) == n, (b, k, thr)
            got_f, got_s = h["hit_frames"][b, k], h["hit_score"][b, k]
            for r, (s, e, sc) in enumerate(hits):
                assert (int(got_f[r, 0]), int(got_f[r, 1])) == (s, e), (b, k, r)
                assert got_s[r].tobytes() == np.float32(sc).tobytes(), (b, k, r)
            assert (got_f[len(hits):] == -1).all() and (got_s[len(hits):] == -np.inf).all(), (b, k)


def _check_dense(h, lp, enc_len, kws, errs, exact=False):
    """Check 1 (and 3 with ``exact``): E against float64, -inf exactly where the reference has it, every returned start optimal."""
    for b, T in enumerate(enc_len):
        for k, y in enumerate(kws):
            E, S = h["dense_score"][b, k].astype(np.float64), h["dense_start"][b, k]
            if T == 0:
                assert (E == -np.inf).all() and (S == -1).all() and int(h["n_hits"][b, k]) == 0
                continue
            Er, Sr = R.dense(lp[b, :T], y)
            fin = np.isfinite(Er)
            assert np.array_equal(np.isfinite(E[:T]), fin), (b, k, "-inf pattern")
            assert (E[:T][~fin] == -np.inf).all() and (S[:T][~fin] == -1).all()
            assert (E[:T][fin] <= 0).all()
            if exact:
                assert np.array_equal(E[:T], Er) and np.array_equal(S[:T], Sr), (b, k, "tie rule")
                continue
            if fin.any():
                d = np.abs(E[:T][fin] - Er[fin]) / np.maximum(1.0, np.abs(Er[fin]))
                errs["dense"] = max(errs.get("dense", 0.0), float(d.max()))
                assert (d <= 1e-3).all(), (b, k, float(d.max()))
                sp = R.span_scores(lp[b, :T], y, S[:T][fin], np.nonzero(fin)[0])
                d = np.abs(sp - Er[fin]) / np.maximum(1.0, np.abs(Er[fin]))
                errs["start"] = max(errs.get("start", 0.0), float(d.max()))
                assert (d <= 1e-3).all(), (b, k, "a returned start is not optimal", float(d.max()))


def _planted_case(rng, V, Tp, enc_len, kws, n_plant, kind):
    """Log-probs [B, Tp, V] whose greedy path (peaked) holds the first ``n_plant`` keywords once per utterance that has room."""
    B = len(enc_len)
    top = np.stack([I.background(rng, Tp, V) for _ in range(B)])
    planted = {}
    for b, T in enumerate(enc_len):
        pos = 2
        for k in range(n_plant):
            r = I.plant(rng, top[b], V, kws[k], pos, T)
            if r is not None:
                planted[(b, k)] = r[:2]
                pos = r[2]
    return I.log_probs(rng, B, Tp, V, kind, top), planted


# (V, T', enc_len, token counts (repeats), keywords planted, further random keywords)
CASES = {
    "lanes": (34, 160, [160, 0, 97], [(1, 0), (2, 0), (3, 1), (31, 2), (32, 0), (33, 3), (3, 0)], 4, 0),
    "full": (257, 400, [400], [(64, 0), (63, 5), (17, 2), (5, 0)], 4, 1),
    "many": (1025, 160, [60, 5, 1], [(4, 0), (2, 1), (1, 0), (6, 0)], 4, 126),
    "tiny": (4, 5, [5, 3, 1], [(2, 0)], 1, 0),
}


def _case(name, kind):
    V, Tp, enc_len, plan, n_plant, extra = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + (7 if kind == "flat" else 0))
    kws = [I.keyword(rng, U, V, r) for U, r in plan]
    if name == "full":
        kws.append(list(kws[3]))                                   # two identical keywords
    else:
        kws += [I.keyword(rng, int(rng.integers(1, 7)), V) for _ in range(extra)]
    lp, planted = _planted_case(rng, V, Tp, enc_len, kws, n_plant, kind)
    return V, Tp, enc_len, kws, lp, planted


@pytest.mark.parametrize("kind", ["peaked", "flat"])
@pytest.mark.parametrize("name", list(CASES))
def test_op_kws_matches_float64_reference(name, kind):
    """Checks 1, 2 and 4: lane edges U in {1, 2, 3, 31, 32, 33, 63, 64}, K in {1, 5, 7, 130}, B in {1, 3}, T' in {1, 3, 5, 160, 400},
    ragged lengths with 0 and T', adjacent repeats, two identical keywords."""
    eng = _op_engine()
    V, Tp, enc_len, kws, lp, planted = _case(name, kind)
    errs = {}
    for i, thr in enumerate(THRESHOLDS):
        h = _run(eng, lp, enc_len, kws, thr, max_hits=8)
        if i == 0:
            _check_dense(h, lp, enc_len, kws, errs)
            if name == "full":
                for key in ("n_hits", "hit_frames", "hit_score", "dense_score", "dense_start"):
                    assert np.array_equal(h[key][:, 3], h[key][:, 4]), key
            if kind == "peaked":       # check 4: every planted occurrence comes back exactly, with score 0
                assert planted or name == "tiny"       # (5 frames hold no planted two-token keyword with its guards)
                for (b, k), (s, e) in planted.items():
                    n = min(int(h["n_hits"][b, k]), 8)
                    found = [(int(f[0]), int(f[1]), float(sc)) for f, sc in zip(h["hit_frames"][b, k, :n], h["hit_score"][b, k, :n])]
                    assert (s, e, 0.0) in found, (b, k, (s, e), found)
        _check_hits_are_the_rule(h, enc_len, kws, thr, 8)
        # the search kernel without the dense rows returns the same hits
        g = _run(eng, lp, enc_len, kws, thr, max_hits=8, dense=False)
        for key in ("n_hits", "hit_frames"):
            assert np.array_equal(g[key], h[key]), key
        assert g["hit_score"].tobytes() == h["hit_score"].tobytes()
    report(f"ctc_kws_op_{name}_{kind}", **errs)


@pytest.mark.parametrize("V,Tp", [(4, 40), (34, 120), (4, 3), (4, 1)])
def test_op_kws_exact_ties_follow_the_tie_rule(V, Tp):
    """Check 3: dyadic log-probs -- E, S and the hits equal the reference bit for bit."""
    eng = _op_engine()
    rng = np.random.default_rng(21 + V + Tp)
    kws = [I.keyword(rng, U, V, r) for U, r in ((1, 0), (2, 1), (3, 0), (5, 2), (min(33, Tp), 4))]
    enc_len = [Tp, max(Tp - 9, 1), Tp // 2]
    lp = I.log_probs(rng, 3, Tp, V, "dyadic")
    for thr in (0.5, 0.2):
        h = _run(eng, lp, enc_len, kws, thr, max_hits=4)
        _check_dense(h, lp, enc_len, kws, {}, exact=True)
        ms = _min_scores(kws, thr)
        for b, T in enumerate(enc_len):
            for k, y in enumerate(kws):
                hits, n = R.pick(*R.dense(lp[b, :T], y), ms[k], 4)
                assert int(h["n_hits"][b, k]) == n
                got = [(int(f[0]), int(f[1]), float(sc)) for f, sc in zip(h["hit_frames"][b, k], h["hit_score"][b, k])][:len(hits)]
                assert got == [(s, e, float(sc)) for s, e, sc in hits], (b, k)


@pytest.mark.parametrize("max_hits", [1, 2])
def test_op_kws_truncation_counts_every_hit(max_hits):
    """Check 5 (and 6: the last occurrence ends on the last valid frame and is flushed)."""
    eng = _op_engine()
    rng = np.random.default_rng(3)
    V, Tp, T = 34, 70, 61
    y = [7]
    top = np.where(rng.random(Tp) < 0.5, V - 1, rng.integers(8, V, Tp))       # (the background never holds the keyword's token)
    spans = [(4, 5), (10, 10), (20, 22), (40, 40), (T - 2, T - 1)]
    for s, e in spans:
        top[s - 1] = V - 1
        top[s:e + 1] = 7
        if e + 1 < Tp:
            top[e + 1] = V - 1
    top[T:] = 7                                                                # padding frames full of the keyword
    lp = I.log_probs(rng, 1, Tp, V, "peaked", top[None])
    h = _run(eng, lp, [T], [y], 0.5, max_hits)
    assert int(h["n_hits"][0, 0]) == len(spans)
    assert h["hit_frames"][0, 0].tolist() == [list(sp) for sp in spans[:max_hits]]
    assert (h["hit_score"][0, 0] == 0.0).all()
    _check_hits_are_the_rule(h, [T], [y], 0.5, max_hits)
    full = _run(eng, lp, [T], [y], 0.5, 8)
    assert full["hit_frames"][0, 0, :5].tolist() == [list(sp) for sp in spans] and (full["hit_frames"][0, 0, 5:] == -1).all()
    assert (full["hit_score"][0, 0, 5:] == -np.inf).all()


def test_op_kws_padding_frames_never_make_or_extend_a_hit():
    """Check 7: an occurrence that runs across enc_len is cut there; one that lies in the padding is not seen."""
    eng = _op_engine()
    rng = np.random.default_rng(8)
    V, Tp, T = 34, 64, 30
    y = [3, 4, 5]
    top = np.full(Tp, V - 1)
    top[26:32] = [3, 3, 4, 4, 5, 5]          # straddles T = 30: only 3 3 4 4 is inside
    top[40:43] = [3, 4, 5]                   # in the padding
    top[10:13] = [3, 4, 5]
    lp = I.log_probs(rng, 2, Tp, V, "peaked", np.stack([top, top]))
    h = _run(eng, lp, [T, Tp], [y], 0.5, 8)
    assert int(h["n_hits"][0, 0]) == 1 and h["hit_frames"][0, 0, 0].tolist() == [10, 12]
    assert int(h["n_hits"][1, 0]) == 3 and h["hit_frames"][1, 0, :3].tolist() == [[10, 12], [26, 31], [40, 42]]
    _check_dense(h, lp, [T, Tp], [y], {})
    _check_hits_are_the_rule(h, [T, Tp], [y], 0.5, 8)


def test_op_kws_is_bit_identical_on_another_stream():
    eng = _op_engine()
    V, Tp, enc_len, kws, lp, _ = _case("lanes", "flat")
    a = _run(eng, lp, enc_len, kws, 0.3)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        b = _run(eng, lp, enc_len, kws, 0.3)
    torch.cuda.synchronize()
    for k in ("n_hits", "hit_frames", "dense_start"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("hit_score", "dense_score"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_library_rejects_bad_keyword_sets_and_shapes():
    """Check 9."""
    from gigaam_amd import synth
    from gigaam_amd._lib import GigaAMHipError
    eng = make_engine(synth.model_cfg("v2_ctc"), {}, head=False)
    V = 34
    lp, el = torch.zeros((1, 10, V)), torch.tensor([10], dtype=torch.int32)
    with pytest.raises(GigaAMHipError, match="no keyword set"):
        eng.op_ctc_kws(lp, el)
    with pytest.raises(GigaAMHipError, match="65 tokens"):
        eng.set_keywords([[1] * 65], -1.0)
    with pytest.raises(GigaAMHipError, match="empty"):
        eng.set_keywords([[1], []], -1.0)
    with pytest.raises(GigaAMHipError, match="4097 keywords"):
        eng.set_keywords([[1]] * 4097, -1.0)
    for bad in (0.5, float("nan"), -float("inf")):
        with pytest.raises(GigaAMHipError, match="min_score"):
            eng.set_keywords([[1]], bad)
    with pytest.raises(GigaAMHipError, match="no keyword set"):      # a rejected set leaves none behind
        eng.op_ctc_kws(lp, el)
    eng.set_keywords([[1, V - 1]], -1.0)                             # the blank's id: known to be bad once V is
    with pytest.raises(GigaAMHipError, match="token id"):
        eng.op_ctc_kws(lp, el)
    eng.set_keywords([[1, 2]], -1.0)
    for mh in (0, 65):
        with pytest.raises(GigaAMHipError, match="max_hits"):
            eng.op_ctc_kws(lp, el, max_hits=mh)
    with pytest.raises(GigaAMHipError, match="8193"):
        eng.op_ctc_kws(torch.zeros((1, 8193, 4)), torch.tensor([8193], dtype=torch.int32))
    assert int(eng.op_ctc_kws(lp, el).host()["n_hits"][0, 0]) >= 0   # and the handle still works
    eng.set_keywords([], -1.0)
    with pytest.raises(GigaAMHipError, match="no keyword set"):
        eng.op_ctc_kws(lp, el)
    # a handle with a CTC head knows V when the set is made
    ck = synth.make_checkpoint("v2_ctc", seed=1, n_layers=1)
    eng2 = make_engine(ck["cfg"], ck["state_dict"])
    with pytest.raises(GigaAMHipError, match="token id"):
        eng2.set_keywords([[len(synth.CHAR_VOCAB)]], -1.0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["v2_ctc_l2", "v3_e2e_ctc_l2"])
def test_encoded_kws_finds_the_words_of_the_greedy_decode(name, mode):
    """Check 10: the words of this path's own greedy decode, as keywords, on the golden encoder output."""
    from gigaam_amd.decoding import Tokenizer
    from gigaam_amd.engine import HipEngine
    from gigaam_amd.timestamps_utils import word_token_groups
    ck, _, _, gold = load_case(name)
    if name.startswith("v3_e2e"):
        ck["cfg"]["decoding"]["model_path"] = os.path.join(ROOT, "tests", "golden", "spm256.model")
    dec_cfg = ck["cfg"]["decoding"]
    tok = Tokenizer(list(dec_cfg.get("vocabulary") or []), dec_cfg.get("model_path"))
    eng = make_engine(ck["cfg"], ck["state_dict"], mode)
    enc, elen = torch.from_numpy(gold["encoded"]), torch.from_numpy(gold["enc_len"])
    rows, flag = HipEngine.collect(eng.ctc_greedy(enc, elen))
    assert not flag
    kws, origin = [], []
    for b, (ids, frames) in enumerate(rows):
        for grp in word_token_groups(tok, ids)[:6]:
            lo, hi = grp[0], grp[-1]
            if tok.charwise and hi + 1 < len(ids) and tok.id_to_str(ids[hi + 1]) == " ":
                hi += 1                                              # with its trailing space: a whole word
            y = ids[lo:hi + 1][:64]                                  # (a longer word: its first 64 tokens)
            if len(y) >= 2:
                kws.append(y)
                origin.append((b, frames[lo], frames[lo + len(y) - 1]))
        if len(ids) >= 8:                                            # and a stretch from the middle of the transcript
            lo = len(ids) // 2 - 4
            kws.append(ids[lo:lo + 8])
            origin.append((b, frames[lo], frames[lo + 7]))
    assert len(kws) >= len(rows)
    eng.set_keywords(kws, _min_scores(kws, 0.5))
    h = eng.ctc_kws(enc, elen, max_hits=8, dense=True).host()
    assert not h["flag"]
    err = 0.0
    for k, (b, f0, f1) in enumerate(origin):
        T = int(gold["enc_len"][b])
        n = min(int(h["n_hits"][b, k]), 8)
        spans = [(int(f[0]), int(f[1]), float(sc)) for f, sc in zip(h["hit_frames"][b, k, :n], h["hit_score"][b, k, :n])]
        inside = [sp for sp in spans if sp[0] <= f0 and f1 <= sp[1]]
        assert inside, (b, k, (f0, f1), spans)
        s, e, sc = inside[0]
        ref = R.span_score(gold["log_probs"][b][:T], kws[k], s, e)
        err = max(err, abs(sc - ref) / max(1.0, abs(ref)))
        assert abs(sc - ref) <= _bar(ref), (b, k, sc, ref)
    g = eng.op_ctc_kws(eng.ctc_head(enc), elen, max_hits=8, dense=True).host()
    for key in ("n_hits", "hit_frames", "dense_start"):
        assert np.array_equal(g[key], h[key]), key
    for key in ("hit_score", "dense_score"):
        assert g[key].tobytes() == h[key].tobytes(), key
    report(f"ctc_kws_golden_{name}_{mode}", score_rel_err=err, keywords=len(kws))


def _wav_file(tmp_path, wav, name):
    import wave
    pcm = (wav.numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16)
    p = str(tmp_path / name)
    with wave.open(p, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(16000)
        wf.writeframes(pcm.tobytes())
    return p


def test_model_find_keywords(tmp_path):
    """Check 11: the model API on synthetic audio -- the words the model itself hears are found where it hears them."""
    import gigaam_amd
    from gigaam_amd import synth
    from gigaam_amd.types import KeywordHit, KeywordSearchResult
    ck = synth.make_checkpoint("v2_ctc", seed=1, n_layers=2)
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    wav, _ = synth.synth_audio(1, 8.0, seed=17)
    wpath = _wav_file(tmp_path, wav[0], "clip.wav")
    words = [w for w in model.transcribe(wpath, word_timestamps=True).words if 2 <= len(w.text) <= 64]
    assert words
    w = words[0]
    ids = model.decoding.tokenizer.encode(w.text)
    res = model.find_keywords(wpath, [w.text, ids, "ъъъъъъ"], threshold=0.5, max_hits=8)
    assert isinstance(res, KeywordSearchResult) and res.keywords == [w.text, w.text, "ъъъъъъ"]
    assert all(isinstance(x, KeywordHit) and x.segment is None for x in res.hits)
    assert [(x.start, x.keyword_index) for x in res.hits] == sorted((x.start, x.keyword_index) for x in res.hits)
    mine = [x for x in res.hits if x.keyword_index == 0]
    assert any(x.start <= w.start + 1e-9 and w.end <= x.end + 1e-9 and x.score == 0.0 and x.confidence == 1.0 for x in mine), (w, mine)
    assert [(x.start_frame, x.end_frame, x.score) for x in mine] == [(x.start_frame, x.end_frame, x.score) for x in res.hits if x.keyword_index == 1]
    for x in res.hits:
        assert 0.0 < x.confidence <= 1.0 and x.confidence >= 0.5 - 1e-6 and x.score <= 0.0
        assert x.confidence == pytest.approx(math.exp(x.score / len(model.decoding.keyword_ids([x.keyword])[0])))
    # ragged batch: each utterance its own result, times from its own frame shift
    m0 = next(x for x in mine if x.start <= w.start + 1e-9 and w.end <= x.end + 1e-9 and x.score == 0.0)     # the word's own occurrence
    bw, bl = synth.synth_audio(2, 8.0, seed=17, lengths=[128000, 70000])
    out = model.find_keywords_batch(bw, bl, [w.text], threshold=0.5)
    assert len(out) == 2 and any((x.start_frame, x.end_frame, x.score) == (m0.start_frame, m0.end_frame, 0.0) for x in out[0].hits)
    for r, n in zip(out, [128000, 70000]):
        assert all(x.end <= n / 16000 + 1e-6 for x in r.hits)
    # longform with given regions: file times carry the region's offset, frames stay local
    long_wav = torch.cat([torch.zeros(16000), wav[0], torch.zeros(8000), wav[0]])
    lpath = _wav_file(tmp_path, long_wav, "long.wav")
    regions = [(1.0, 9.0), (9.5, 17.5)]
    # min_duration=1.0: the packer closes a chunk once it is past 1 s, so each given region is a chunk of its own (with the default
    # 15 s it would pack the two 8 s regions into ONE chunk, as transcribe_longform does) -- and each chunk is the clip's samples
    lf = model.find_keywords_longform(lpath, [w.text], threshold=0.5, speech_regions=regions, min_duration=1.0)
    m = next(x for x in mine if x.start <= w.start + 1e-9 and w.end <= x.end + 1e-9 and x.score == 0.0)     # the word's own occurrence
    for seg, (r0, _) in enumerate(regions):
        got = [x for x in lf.hits if x.segment == seg and (x.start_frame, x.end_frame, x.score) == (m.start_frame, m.end_frame, 0.0)]
        assert len(got) == 1, (seg, m, lf.hits)
        x = got[0]
        assert x.start == pytest.approx(r0 + m.start, abs=1e-3) and x.end == pytest.approx(r0 + m.end, abs=1e-3), (x, m)   # (rounded to 1 ms)
    assert {x.segment for x in lf.hits} <= {0, 1}
    assert [x.start for x in lf.hits] == sorted(x.start for x in lf.hits)
    # truncation is reported per keyword
    one = model.find_keywords(wpath, [[ids[0]]], threshold=0.9, max_hits=1)
    many = model.find_keywords(wpath, [[ids[0]]], threshold=0.9, max_hits=64)
    assert len(one.hits) == 1 and one.truncated == ([0] if len(many.hits) > 1 else [])
    with pytest.raises(ValueError, match="at most 25 s"):
        model.find_keywords(_wav_file(tmp_path, torch.zeros(26 * 16000), "silence.wav"), [w.text])


def test_model_find_keywords_needs_a_ctc_head():
    import gigaam_amd
    from gigaam_amd import synth
    model = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_rnnt", seed=1, n_layers=1), "cuda:0")
    wav, wlen = synth.synth_audio(1, 2.0, seed=3)
    with pytest.raises(TypeError, match="keyword search needs a CTC head"):
        model.find_keywords_batch(wav, wlen, ["а"])


def test_fullsize32_kws_timing():
    """The search alone on the head's log-probs of the 32 x 20 s batch (device events): K = 10, 100, 1000 keywords of 4-12 tokens."""
    from gigaam_amd import synth, workloads
    ck = synth.make_checkpoint("v2_ctc", seed=0)
    eng = make_engine(ck["cfg"], ck["state_dict"])
    wav, wlen = workloads.config2_batch(32, 20.0, rank=0)
    enc, elen = eng.encode(*eng.frontend(wav, wlen))
    lp = eng.ctc_head(enc)
    V = lp.shape[2]
    rng = np.random.default_rng(0)
    ms = {}
    for K in (10, 100, 1000):
        kws = [I.keyword(rng, int(rng.integers(4, 13)), V) for _ in range(K)]
        eng.set_keywords(kws, _min_scores(kws, 0.5))
        for _ in range(2):
            out = eng.op_ctc_kws(lp, elen)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        n = 5
        for _ in range(n):
            out = eng.op_ctc_kws(lp, elen)
        e1.record()
        torch.cuda.synchronize()
        ms[f"op_kws_ms_K{K}"] = e0.elapsed_time(e1) / n
        h = out.host()
        assert h["n_hits"].shape == (32, K) and (h["n_hits"] >= 0).all()
    report("ctc_kws_fullsize32", frames=int(lp.shape[1]), **ms)
