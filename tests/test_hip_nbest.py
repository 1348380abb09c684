"""GPU: N-best of the CTC and RNN-T beam searches (gam_ctc_beam_nbest / gam_rnnt_beam_nbest and their op twins; the emission:
gigaam_amd/csrc/gam_search.h) -- hypothesis 0 against the 1-best calls bit for bit, the whole list against brute force and the float64
references of tests/nbest_ref.py, truncation and padding, long utterances, determinism, limits, and through the model.

Margin rule (tests/nbest_ref.py): the kernels rank in fp32, the references in fp64; an utterance is compared when every per-frame
margin and every gap among the first min(N + 1, n) final values exceed the margin of the search's 1-best test module (CTC 2e-5, RNN-T
1e-4), and at least 90 % of each parameter set's utterances must qualify (tests/test_nbest_host.py holds that on the CPU)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import beam_common as BC
import nbest_inputs as I
import nbest_ref as N
from common import report

pytestmark = pytest.mark.gpu

_ENGINES = {}


def _ctc_engine():
    return BC.ctc_op_engine(__name__)


def _rnnt_engine(V, L=1, blank_bias=None):
    key = (V, L, blank_bias)
    if key not in _ENGINES:
        from gigaam_amd.engine import HipEngine, build_config
        cfg, sd, head = I.rnnt_head(V, L, blank_bias)
        _ENGINES[key] = (HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), sd, torch.device("cuda:0")), head, cfg)
    return _ENGINES[key]


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _len(enc_len):
    return torch.tensor(enc_len, dtype=torch.int32)


def _ctc_nbest(eng, lp, enc_len, W, n):
    return eng.op_ctc_beam_nbest(_t(lp), _len(enc_len), W, n).host()


def _rnnt_nbest(eng, encp, enc_len, W, S, n):
    return eng.op_rnnt_beam_nbest(_t(encp), _len(enc_len), W, S, n).host()


def _set(eng, tmp_path, tok, phrases, lm):
    from gigaam_amd import lm as LM
    eng.set_hotwords(phrases, I.BETA)
    if lm is None:
        eng.set_lm(None)
    else:
        p = tmp_path / "nbest.arpa"
        p.write_text(lm[0], encoding="utf-8")
        eng.set_lm(LM.NgramLM.from_arpa(str(p)), tok, I.LM_ALPHA, I.LM_BETA)


def _clear(eng):
    eng.set_lm(None)
    eng.set_hotwords([])


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _assert_hyp0(nb, one, what):
    """Row 0 of an N-best result against the 1-best call's: ids, frames, counts, and score / logp as raw bits."""
    for b, row in enumerate(one["rows"]):
        assert int(nb["n_hyp"][b]) >= 1, (what, b)
        assert nb["rows"][b][0] == row, (what, b, nb["rows"][b][0], row)
    for k in ("score", "logp"):
        assert np.array_equal(_bits(nb[k][:, 0]), _bits(one[k])), (what, k, nb[k][:, 0], one[k])


# ---- 1. hypothesis 0 is the 1-best result, bit for bit
@pytest.mark.parametrize("variant", ["plain", "hotwords", "lm"])
@pytest.mark.parametrize("V", [34, 1025])
def test_ctc_hypothesis_0_is_the_1best_result_bit_for_bit(tmp_path, V, variant):
    eng = _ctc_engine()
    lp, enc_len, phrases, lm = I.ctc_hyp0_inputs(V)[variant]
    _set(eng, tmp_path, BC.tokenizer(V), phrases, lm)
    try:
        for W in (1, 4, 32):
            one = BC.run_ctc_op(eng, lp, enc_len, W)
            for n in sorted({1, W}):
                _assert_hyp0(_ctc_nbest(eng, lp, enc_len, W, n), one, (V, variant, W, n))
    finally:
        _clear(eng)


@pytest.mark.parametrize("variant", ["plain", "hotwords", "lm"])
@pytest.mark.parametrize("V", [34, 1025])
def test_rnnt_hypothesis_0_is_the_1best_result_bit_for_bit(tmp_path, V, variant):
    eng, _, _ = _rnnt_engine(V)
    encp, enc_len, phrases, lm = I.rnnt_hyp0_inputs(V)[variant]
    _set(eng, tmp_path, BC.tokenizer(V), phrases, lm)
    try:
        for W, S in itertools.product((1, 4, 32), (1, 10)):
            one = BC.run_rnnt_op(eng, encp, enc_len, W, S)
            for n in sorted({1, W}):
                _assert_hyp0(_rnnt_nbest(eng, encp, enc_len, W, S, n), one, (V, variant, W, S, n))
    finally:
        _clear(eng)


# ---- 2. exact top-N when nothing is pruned
def _assert_brute(h, b, brute, tol, errs, what):
    assert int(h["n_hyp"][b]) == len(brute), (what, b, int(h["n_hyp"][b]), len(brute))
    vals = [v for v, _, _ in brute]
    for r, (val, y, ll) in enumerate(brute):
        apart = (r == 0 or vals[r - 1] - val > 1e-5) and (r + 1 == len(vals) or val - vals[r + 1] > 1e-5)
        if apart:
            assert h["rows"][b][r][0] == y, (what, b, r, h["rows"][b][r][0], y)
        for k, want in (("score", val), ("logp", ll)):
            e = abs(float(h[k][b, r]) - want)
            errs[k] = max(errs.get(k, 0.0), e)
            if apart or k == "score":     # (within a tie the sequences may swap; the values are then equal within the tie's width)
                assert e <= tol(want) + (0.0 if apart else 1e-5), (what, b, r, k, float(h[k][b, r]), want)


def test_ctc_nbest_is_the_exact_list_when_nothing_is_pruned():
    """V = 3, T' <= 4, W = N = 32, B = 16: every prefix with a finite value is returned, in the brute-force order."""
    eng = _ctc_engine()
    errs = {}
    try:
        for hot, lp, enc_len in I.ctc_exact_inputs():
            eng.set_hotwords(hot, I.EXACT_BETA)
            h = _ctc_nbest(eng, lp, enc_len, 32, 32)
            for b, T in enumerate(enc_len):
                _assert_brute(h, b, N.ctc_brute(lp[b].astype(np.float64), T, hot, I.EXACT_BETA), lambda ref: 1e-5, errs, hot)
    finally:
        _clear(eng)
    report("ctc_nbest_exact", **errs)


def test_rnnt_nbest_is_the_exact_list_when_nothing_is_pruned():
    """V = 3, S = 1, T' <= 4, W = N = 32, B = 16."""
    eng, head, _ = _rnnt_engine(3, 1, 0.0)
    errs = {}
    try:
        for hot, encp, enc_len in I.rnnt_exact_inputs():
            eng.set_hotwords(hot, I.EXACT_BETA)
            h = _rnnt_nbest(eng, encp, enc_len, 32, 1, 32)
            for b, T in enumerate(enc_len):
                _assert_brute(h, b, N.rnnt_brute(head, encp[b], T, hot, I.EXACT_BETA), lambda ref: 1e-4 * max(1.0, abs(ref)), errs, hot)
    finally:
        _clear(eng)
    report("rnnt_nbest_exact", **errs)


# ---- 3. against the float64 N-best reference
def _compare_nbest(h, b, ref, n_best, margin, errs):
    if not N.qualifies(ref, n_best, margin):
        return False
    want = ref["hyps"][:n_best]
    assert int(h["n_hyp"][b]) == len(want), (b, int(h["n_hyp"][b]), len(want))
    for r, w in enumerate(want):
        assert h["rows"][b][r] == (w["ids"], w["frames"]), (b, r, h["rows"][b][r], w)
        for k in ("score", "logp"):
            e = abs(float(h[k][b, r]) - w[k])
            errs[k] = max(errs.get(k, 0.0), e / max(1.0, abs(w[k])))
            assert e <= BC.bar(w[k]), (b, r, k, float(h[k][b, r]), w[k])
    return True


@pytest.mark.parametrize("V,kind", I.CTC_REF_SETS)
def test_ctc_nbest_matches_float64_reference(V, kind):
    eng = _ctc_engine()
    errs, n, ok = {}, 0, 0
    try:
        for W, lp, enc_len, phrases in I.ctc_ref_inputs(V, kind):
            eng.set_hotwords(phrases, I.BETA)
            h = _ctc_nbest(eng, lp, enc_len, W, W)
            for b in range(len(enc_len)):
                ok += _compare_nbest(h, b, N.ctc_nbest(lp[b], W, enc_len[b], phrases, I.BETA), W, N.CTC_MARGIN, errs)
                n += 1
    finally:
        _clear(eng)
    report(f"ctc_nbest_op_{V}_{kind}", qualified=f"{ok}/{n}", **errs)
    assert ok >= 0.9 * n, (ok, n)


@pytest.mark.parametrize("V,kind,L", I.RNNT_REF_SETS)
def test_rnnt_nbest_matches_float64_reference(V, kind, L):
    eng, head, _ = _rnnt_engine(V, L, 14.0 if kind == "blank" else None)
    eng.set_hotwords([])
    errs, n, ok = {}, 0, 0
    for W, S, encp, enc_len in I.rnnt_ref_inputs(V, kind, L):
        h = _rnnt_nbest(eng, encp, enc_len, W, S, W)
        for b in range(len(enc_len)):
            ok += _compare_nbest(h, b, N.rnnt_nbest(head, encp[b].astype(np.float64), W, S, enc_len[b]), W, N.RNNT_MARGIN, errs)
            n += 1
    report(f"rnnt_nbest_op_{V}_{kind}_L{L}", qualified=f"{ok}/{n}", **errs)
    assert ok >= 0.9 * n, (ok, n)


# ---- 4. truncation and padding
def _assert_prefix(small, big, n):
    for b in range(len(big["rows"])):
        assert int(small["n_hyp"][b]) == min(n, int(big["n_hyp"][b]))
        assert small["rows"][b] == big["rows"][b][:n], b
    for k in ("score", "logp"):
        assert np.array_equal(_bits(small[k]), _bits(big[k][:, :n])), k


def test_nbest_truncates_and_pads():
    eng = _ctc_engine()
    rng = np.random.default_rng(31)
    lp = BC.log_probs(rng, 4, 30, 34, "flat")
    enc_len = [30, 17, 1, 0]
    big, small = _ctc_nbest(eng, lp, enc_len, 8, 8), _ctc_nbest(eng, lp, enc_len, 8, 3)
    _assert_prefix(small, big, 3)
    assert int(big["n_hyp"][0]) == 8 and int(big["n_hyp"][3]) == 1
    # enc_len = 0: one empty hypothesis with 0 scores, the other rows padded
    assert big["rows"][3] == [([], [])] and float(big["score"][3, 0]) == 0.0 and float(big["logp"][3, 0]) == 0.0
    assert np.all(np.isneginf(big["score"][3, 1:])) and np.all(np.isneginf(big["logp"][3, 1:]))
    # enc_len = 1 at V = 3: at most 3 prefixes exist, so n_hyp < N and the rows past it carry counts 0 and -inf
    lp3 = np.log(rng.dirichlet(np.ones(3), size=(2, 4))).astype(np.float32)
    dev = eng.op_ctc_beam_nbest(_t(lp3), _len([1, 4]), 8, 8)
    h = dev.host()
    nh = int(h["n_hyp"][0])
    assert nh == 3 and len(h["rows"][0]) == 3
    assert dev.counts.cpu()[0, nh:].tolist() == [0] * (8 - nh)
    assert np.all(np.isneginf(h["score"][0, nh:])) and np.all(np.isneginf(h["logp"][0, nh:]))
    assert np.all(np.isfinite(h["score"][0, :nh]))
    # RNN-T: the same truncation; enc_len = 0
    reng, _, cfg = _rnnt_engine(34)
    reng.set_hotwords([])
    encp = BC.encp(rng, 3, 12, cfg["head"]["joint"]["joint_hidden"], 1.0)
    rl = [12, 0, 5]
    rbig, rsmall = _rnnt_nbest(reng, encp, rl, 8, 3, 8), _rnnt_nbest(reng, encp, rl, 8, 3, 3)
    _assert_prefix(rsmall, rbig, 3)
    assert rbig["rows"][1] == [([], [])] and float(rbig["score"][1, 0]) == 0.0 and float(rbig["logp"][1, 0]) == 0.0
    assert np.all(np.isneginf(rbig["score"][1, 1:]))


# ---- 5. structure at length
def _assert_structure(h, one, enc_len, cap, what):
    for b, T in enumerate(enc_len):
        rows = h["rows"][b]
        assert len(rows) == int(h["n_hyp"][b]) >= 2, (what, b)
        assert len({tuple(i) for i, _ in rows}) == len(rows), (what, b, "hypotheses repeat")
        for ids, fr in rows:
            assert len(ids) == len(fr) <= cap
            assert all(0 <= f < T for f in fr) and all(x <= y for x, y in zip(fr, fr[1:])), (what, b)
        sc = h["score"][b, :len(rows)]
        assert np.all(np.isfinite(sc)) and np.all(sc[:-1] >= sc[1:]), (what, b, sc)
    _assert_hyp0(h, one, what)


def test_nbest_structure_on_long_utterances():
    eng = _ctc_engine()
    rng = np.random.default_rng(77)
    Tp = 600
    lp = BC.log_probs(rng, 2, Tp, 34, "peaked")
    enc_len = [Tp, 555]
    dev = eng.op_ctc_beam_nbest(_t(lp), _len(enc_len), 32, 32)
    h = dev.host()
    _assert_structure(h, BC.run_ctc_op(eng, lp, enc_len, 32), enc_len, Tp, "ctc")
    assert dev.copied_bytes < 2 * 2 * 32 * Tp * 4        # (the columns past the longest hypothesis stay on the device)
    reng, _, cfg = _rnnt_engine(34)
    reng.set_hotwords([])
    T, S = 60, 10
    encp = BC.encp(rng, 2, T, cfg["head"]["joint"]["joint_hidden"], 1.0)
    rl = [T, 47]
    rdev = reng.op_rnnt_beam_nbest(_t(encp), _len(rl), 32, S, 32)
    rh = rdev.host()
    _assert_structure(rh, BC.run_rnnt_op(reng, encp, rl, 32, S), rl, T * S, "rnnt")
    assert rdev.copied_bytes < 2 * 2 * 32 * T * S * 4


# ---- 6. determinism
def test_nbest_is_bit_identical_run_to_run_and_on_another_stream():
    eng = _ctc_engine()
    rng = np.random.default_rng(9)
    lp = BC.log_probs(rng, 4, 120, 257, "flat")
    reng, _, cfg = _rnnt_engine(257, 2, None)
    encp = BC.encp(rng, 4, 40, cfg["head"]["joint"]["joint_hidden"], 1.0)
    eng.set_hotwords(BC.ctc_hotwords(rng, lp, 20), 1.0)
    reng.set_hotwords([[1, 2], [5], [7, 7, 3]], 1.0)
    runs = (lambda: _ctc_nbest(eng, lp, [120, 100, 120, 7], 8, 8), lambda: _rnnt_nbest(reng, encp, [40, 31, 40, 7], 8, 10, 8))
    try:
        for run in runs:
            a, b = run(), run()
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                c = run()
            torch.cuda.synchronize()
            for o in (b, c):
                assert a["rows"] == o["rows"] and a["n_hyp"].tolist() == o["n_hyp"].tolist()
                for k in ("score", "logp"):
                    assert a[k].tobytes() == o[k].tobytes(), k
    finally:
        _clear(eng)
        _clear(reng)


# ---- 7. limits
def test_library_and_engine_reject_nbest_beyond_the_limits():
    from gigaam_amd._lib import GigaAMHipError
    eng = _ctc_engine()
    lp = torch.log_softmax(torch.zeros((1, 10, 34)), dim=-1)
    one = _len([10])
    for W, n in ((4, 0), (4, 5), (32, 33), (0, 1), (33, 1)):
        with pytest.raises(GigaAMHipError):
            eng.op_ctc_beam_nbest(lp, one, W, n)
    reng, _, cfg = _rnnt_engine(34)
    encp = torch.zeros((1, 10, cfg["head"]["joint"]["joint_hidden"]))
    for W, S, n in ((4, 10, 0), (4, 10, 5), (32, 10, 33), (0, 10, 1), (33, 10, 1), (4, 0, 1), (4, 17, 1)):
        with pytest.raises(GigaAMHipError):
            reng.op_rnnt_beam_nbest(encp, one, W, S, n)
    with pytest.raises(GigaAMHipError, match="encp must be"):
        reng.op_rnnt_beam_nbest(torch.zeros((1, 10, 8)), one, 4, 10, 2)
    # the library itself: an error code and a message, no launch
    d_lp, d_len = lp.cuda(), one.cuda()
    buf = torch.zeros(4096, dtype=torch.int32, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731

    def ctc(W, n, V=34, Tp=10, ids=buf):
        return eng.lib.gam_op_ctc_beam_nbest(eng._h, p(d_lp), p(d_len), 1, Tp, V, W, n, p(ids), p(buf), p(buf), p(buf), p(buf), p(buf), None)

    for W, n in ((4, 0), (4, 5), (32, 33), (0, 1), (33, 1)):
        assert ctc(W, n) != 0, (W, n)
        assert eng.lib.gam_last_error(eng._h)
    assert ctc(4, 2, V=1026) != 0 and ctc(4, 2, V=1) != 0 and ctc(4, 2, Tp=8193) != 0
    assert eng.lib.gam_op_ctc_beam_nbest(eng._h, p(d_lp), p(d_len), 1, 10, 34, 4, 2, None, p(buf), p(buf), p(buf), p(buf), p(buf), None) != 0
    assert eng.lib.gam_op_ctc_beam_nbest(eng._h, p(d_lp), p(d_len), 1, 10, 34, 4, 2, p(buf), p(buf), p(buf), p(buf), p(buf), None, None) != 0
    d_encp = encp.cuda()

    def rnnt(W, S, n, Tp=10):
        return reng.lib.gam_op_rnnt_beam_nbest(reng._h, p(d_encp), p(d_len), 1, Tp, W, S, n, p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), None)

    for W, S, n in ((4, 10, 0), (4, 10, 5), (32, 10, 33), (0, 10, 1), (33, 10, 1), (4, 0, 1), (4, 17, 1)):
        assert rnnt(W, S, n) != 0, (W, S, n)
    assert rnnt(4, 10, 2, Tp=8193) != 0
    # a CTC-less / RNN-T-less handle refuses the other family's calls
    assert eng.lib.gam_op_rnnt_beam_nbest(eng._h, p(d_encp), p(d_len), 1, 10, 4, 10, 2, p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), None) != 0
    # hotword ids beyond V - 2 and an LM for another V are the 1-best calls' errors
    eng.set_hotwords([[40]], 1.0)
    with pytest.raises(GigaAMHipError, match="hotword"):
        eng.op_ctc_beam_nbest(lp, one, 4, 2)
    eng.set_hotwords([])
    # both handles are usable afterwards
    h = eng.op_ctc_beam_nbest(lp, one, 4, 4).host()
    assert int(h["n_hyp"][0]) >= 1 and h["rows"][0][0] == BC.run_ctc_op(eng, lp.numpy(), [10], 4)["rows"][0]
    rh = reng.op_rnnt_beam_nbest(encp, one, 4, 10, 4).host()
    assert int(rh["n_hyp"][0]) >= 1 and rh["rows"][0][0] == BC.run_rnnt_op(reng, encp.numpy(), [10], 4, 10)["rows"][0]


# ---- 8. through the model
def _check_result(model, res, one, n_best):
    assert 1 <= len(res) <= n_best
    assert res.best.text == one.text == res.text and res.best.words == one.words
    assert abs(sum(h.posterior for h in res) - 1.0) <= 1e-9
    scores = [h.score for h in res]
    assert scores == sorted(scores, reverse=True)
    assert len({tuple(h.token_ids) for h in res}) == len(res)
    for h in res:
        assert h.text == model.decoding.tokenizer.decode(h.token_ids)
        assert h.words is not None and len(h.token_ids) == len(h.token_frames)


def _check_words(model, res, wav_len, enc_len):
    from gigaam_amd.timestamps_utils import compute_frame_shift, frames_to_words
    shift = compute_frame_shift(int(wav_len), int(enc_len))
    for h in res:
        assert h.words == frames_to_words(model.decoding.tokenizer, h.token_ids, h.token_frames, shift)


def _enc_lens(model, wav, wlen):
    with torch.inference_mode():
        return model._encode(wav.to("cuda:0"), wlen.to("cuda:0"), wlen)[1].cpu().tolist()


def test_ctc_model_transcribe_nbest(tmp_path):
    import gigaam_amd
    from gigaam_amd import lm as LM
    from gigaam_amd import synth
    from gigaam_amd.preprocess import load_audio
    model = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=1, n_layers=2), "cuda:0")
    wpath = BC.wav_file(tmp_path, 3.0, 5)
    greedy = model.transcribe(wpath).text
    rng = np.random.default_rng(3)
    vocab = sorted(set(greedy.split()) | {"да", "нет"})
    path = tmp_path / "m.arpa"
    path.write_text(BC.arpa(rng, vocab, 3, [greedy.split()]), encoding="utf-8")
    lm = LM.NgramLM.from_arpa(str(path))
    hot = [w for w in greedy.split() if len(w) > 1][:2] or ["да"]
    clip = load_audio(wpath)
    for kw in (dict(), dict(beam_size=4), dict(hotwords=hot, hotword_boost=3.0), dict(beam_size=16, lm=lm, lm_weight=0.7, word_bonus=0.5)):
        n_best = 4
        res = model.transcribe_nbest(wpath, n_best, word_timestamps=True, **kw)
        one_kw = dict(kw)
        one_kw.setdefault("beam_size", 8)
        _check_result(model, res, model.transcribe(wpath, word_timestamps=True, **one_kw), n_best)
        wl = torch.tensor([clip.shape[-1]])
        _check_words(model, res, clip.shape[-1], _enc_lens(model, clip.unsqueeze(0), wl)[0])
        assert model.transcribe_nbest(wpath, n_best, **kw).best.words is None
    # a ragged batch of 3 equals the per-clip calls
    wav, wlen = synth.synth_audio(3, 3.0, seed=7, lengths=[48000, 31000, 17000])
    pcm = (wav * 32768.0).round().clip(-32768, 32767) / 32768.0       # (what a PCM16 file holds)
    got = model.transcribe_nbest_batch(pcm, wlen, 3, word_timestamps=True, beam_size=8)
    one_batch = model.transcribe_batch(pcm, wlen, word_timestamps=True, beam_size=8)
    for b in range(3):
        p = str(tmp_path / f"r{b}.wav")
        _write_wav(p, pcm[b, : int(wlen[b])])
        solo = model.transcribe_nbest(p, 3, word_timestamps=True, beam_size=8)
        assert [(h.text, h.token_ids, h.token_frames, h.words) for h in got[b]] == [(h.text, h.token_ids, h.token_frames, h.words) for h in solo]
        assert (got[b].best.text, got[b].best.words) == one_batch[b], b
        assert abs(sum(h.posterior for h in got[b]) - 1.0) <= 1e-9
        diffs = [abs(x.score - y.score) for x, y in zip(got[b], solo)]
        print(f"ctc nbest batch-vs-clip b={b} samples={int(wlen[b])} |score diff|={diffs}")
        if int(wlen[b]) == pcm.shape[1]:
            # The scores are compared on the row that fills the batch only.  A shorter row does not hear the same audio in a batch:
            # the frontend (center=True) reflect-pads n_fft / 2 = 200 samples at the end of the BATCH row, so the last feature frames
            # of a shorter row see the zero padding where the per-clip call sees the clip's reflected end (as torch.stft on a collated
            # batch does) -- its last encoder frames and with them every score differ by an amount no kernel tolerance bounds; its
            # hypotheses, frames and words are still compared above.  The full row differs by the packed / padded encoder paths'
            # rounding alone (<= 2e-5 on the encoder output, tests/test_hip_varlen.py): the score bar of the op-level tests.
            # softmax: |d p_i| <= p_i (1 - p_i) * 2 max |d score| <= max |d score| / 2.
            bars = [BC.bar(y.score) for y in solo]
            assert all(d <= t for d, t in zip(diffs, bars)), (b, diffs, bars)
            assert all(abs(x.posterior - y.posterior) <= 0.5 * max(bars) for x, y in zip(got[b], solo)), b
    with pytest.raises(ValueError, match="exceeds beam_size"):
        model.transcribe_nbest(wpath, 5, beam_size=4)
    with pytest.raises(ValueError, match="n_best"):
        model.transcribe_nbest(wpath, 33)


def _write_wav(path, samples):
    """A PCM16 file of float samples that are multiples of 1 / 32768 (the batch call gets the same samples the file holds)."""
    import wave
    pcm = (samples.numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16)
    with wave.open(path, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(16000)
        wf.writeframes(pcm.tobytes())


def test_rnnt_model_transcribe_nbest(tmp_path):
    model, _ = BC.small_rnnt_model()
    wpath = BC.wav_file(tmp_path, 3.0, 5)
    with pytest.raises(ValueError, match=r"set_decoding\(beam_size="):
        model.transcribe_nbest(wpath, 2)
    model.set_decoding(beam_size=4)
    res = model.transcribe_nbest(wpath, 4, word_timestamps=True)
    _check_result(model, res, model.transcribe(wpath, word_timestamps=True), 4)
    from gigaam_amd.preprocess import load_audio
    clip = load_audio(wpath)
    _check_words(model, res, clip.shape[-1], _enc_lens(model, clip.unsqueeze(0), torch.tensor([clip.shape[-1]]))[0])
    with pytest.raises(TypeError):
        model.transcribe_nbest(wpath, 2, beam_size=8)
    with pytest.raises(TypeError):
        model.transcribe_nbest(wpath, 2, hotwords=["да"])
    with pytest.raises(ValueError, match="exceeds the beam width"):
        model.transcribe_nbest(wpath, 5)
    from gigaam_amd import synth
    wav, wlen = synth.synth_audio(3, 3.0, seed=7, lengths=[48000, 31000, 17000])
    pcm = (wav * 32768.0).round().clip(-32768, 32767) / 32768.0       # (what a PCM16 file holds)
    got = model.transcribe_nbest_batch(pcm, wlen, 3, word_timestamps=True)
    one_batch = model.transcribe_batch(pcm, wlen, word_timestamps=True)
    for b in range(3):
        p = str(tmp_path / f"r{b}.wav")
        _write_wav(p, pcm[b, : int(wlen[b])])
        solo = model.transcribe_nbest(p, 3, word_timestamps=True)
        assert [(h.text, h.token_ids, h.token_frames, h.words) for h in got[b]] == [(h.text, h.token_ids, h.token_frames, h.words) for h in solo]
        assert (got[b].best.text, got[b].best.words) == one_batch[b], b
        assert abs(sum(h.posterior for h in got[b]) - 1.0) <= 1e-9
