"""GPU: RNN-T beam search with hotword boosting (gam_op_rnnt_beam / gam_rnnt_beam, gigaam_amd/csrc/gam_rnnt_beam.h) against the
float64 reference of tests/rnnt_beam_ref.py, the exact MAP, the greedy decode on peaked joints, on another stream, at its limits, on the
golden RNN-T cases, on the full-size 32 x 20 s batch and through the model (set_decoding).

Margin rule (as tests/test_hip_ctc_beam.py): the kernel ranks in fp32, the reference in fp64, so where two hypotheses rank within
rounding of each other either may be kept.  ids / frames are compared on every utterance whose smallest decision margin (every top-W
cut, theta comparison, kept merge and the final pick) exceeds MARGIN; the op-level tests require that at least 90 % of their
utterances qualify.  score / logp are compared on those utterances within 1e-3 * max(1, |ref|)."""
import itertools

import numpy as np
import pytest
import torch

from beam_common import bar as _bar, compare, encp as _encp, fullsize_rnnt_model, run_rnnt_op as _run_op, small_rnnt_model, wav_file as _wav_file
from common import load_case, report

import rnnt_beam_ref as R
from ctc_beam_ref import Trie

pytestmark = pytest.mark.gpu

MODES = ["f16x3", "f32"]
RNNT_CASES = ["v1_rnnt_l2", "v2_rnnt_l2", "v3_rnnt_l2", "v3_e2e_rnnt_l2", "v2_rnnt_l2_dense", "v2_rnnt_l2_lstm2", "v3_e2e_rnnt_l2_dense"]
MARGIN = 1e-4           # op level: <= 24 frames; fp32 LSTM and joint against fp64
MARGIN_LONG = 5e-4      # model level: up to 500 frames, the encoder projection in the engine's GEMM mode


_ENGINES = {}


def _compare(h, b, ref, errs, margin):
    return compare(h, b, ref, errs, margin, R.min_margin)


def _fullsize_model():
    return fullsize_rnnt_model()[0]


def _small_rnnt_model():
    return small_rnnt_model()[0]


def _engine(V, L=1, blank_bias=None, out_scale=1.0):
    """An engine with a synthetic RNN-T head (and a one-layer encoder): V classes, L predictor layers; the joint's output layer
    scaled by out_scale (peaked joints) and its blank bias set (None: the synthetic default, emission-heavy)."""
    key = (V, L, blank_bias, out_scale)
    if key not in _ENGINES:
        from gigaam_amd import synth
        from gigaam_amd.engine import HipEngine, build_config
        cfg = synth.model_cfg("v3_e2e_rnnt" if V > 34 else "v2_rnnt", n_layers=1)
        cfg["head"]["decoder"]["num_classes"] = cfg["head"]["joint"]["num_classes"] = V
        cfg["head"]["decoder"]["pred_rnn_layers"] = L
        sd = synth.make_state_dict(cfg, seed=V + L, rnnt_blank_bias=blank_bias)
        sd["head.joint.joint_net.1.weight"] = sd["head.joint.joint_net.1.weight"] * out_scale
        sd["head.joint.joint_net.1.bias"] = sd["head.joint.joint_net.1.bias"] * out_scale
        eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), sd, torch.device("cuda:0"))
        _ENGINES[key] = (eng, R.head_from_state_dict(sd, L), cfg, sd)
    return _ENGINES[key]


def _hotwords(rng, res_ids, V, n):
    """n phrases of 1-3 tokens: runs of tokens the reference emitted (phrases the beam meets), padded with random ones."""
    out = []
    for _ in range(n):
        ids = res_ids[int(rng.integers(0, len(res_ids)))] if res_ids else []
        if len(ids) >= 2:
            i = int(rng.integers(0, len(ids) - 1))
            out.append([int(c) for c in ids[i:i + int(rng.integers(1, 4))]])
        else:
            out.append([int(c) for c in rng.integers(0, V - 1, int(rng.integers(1, 3)))])
    return out


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("kind", ["blank", "dense"])
@pytest.mark.parametrize("V", [34, 257, 1025])
def test_op_beam_matches_float64_reference(V, kind, L):
    """Seeded encp, W in {1, 4, 8, 32} x S in {1, 3, 10}, with and without hotwords: blank-dominant ("blank") and emission-heavy
    ("dense") joints."""
    eng, head, cfg, _ = _engine(V, L, 14.0 if kind == "blank" else None)
    JH = cfg["head"]["joint"]["joint_hidden"]
    rng = np.random.default_rng(V * 7 + L + (1 if kind == "dense" else 0))
    B = 4
    errs, n, ok = {}, 0, 0
    for W, S in itertools.product((1, 4, 8, 32), (1, 3, 10)):
        T = 10 if W >= 8 else 20
        encp = _encp(rng, B, T, JH, 1.0)
        enc_len = [T, T - 3, 1, T]
        hot = (W + S) % 2 == 1
        phrases = []
        if hot:
            plain = [R.beam_search(head, encp[b].astype(np.float64), W, S, enc_len[b])["ids"] for b in range(B)]
            phrases = _hotwords(rng, plain, V, 6)
        eng.set_hotwords(phrases, 1.5)
        h = _run_op(eng, encp, enc_len, W, S)
        for b in range(B):
            ref = R.beam_search(head, encp[b].astype(np.float64), W, S, enc_len[b], phrases, 1.5)
            ok += _compare(h, b, ref, errs, MARGIN)
            n += 1
    eng.set_hotwords([])
    report(f"rnnt_beam_op_{V}_{kind}_L{L}", qualified=f"{ok}/{n}", **errs)
    assert ok >= 0.9 * n, (ok, n)


def test_op_beam_is_exact_map_when_nothing_is_pruned():
    """V = 3, S = 1, T <= 4, W = 32: at most 31 distinct hypotheses, nothing is pruned -- the result is the MAP sequence under
    log P_1(y | x) (+ committed hotword bonus), its logp the exact DP value."""
    eng, head, cfg, _ = _engine(3, 1, 0.0)
    JH = cfg["head"]["joint"]["joint_hidden"]
    rng = np.random.default_rng(21)
    B, Tp = 8, 4
    errs = {}
    for hot in ([], [[0, 1]], [[1], [0, 0, 1]]):
        eng.set_hotwords(hot, 1.25)
        encp = _encp(rng, B, Tp, JH, 0.5)
        enc_len = [1 + b % Tp for b in range(B)]
        h = _run_op(eng, encp, enc_len, 32, 1)
        trie = Trie(hot)
        for b in range(B):
            T = enc_len[b]
            pred = R.Predictor(head)
            e64 = encp[b].astype(np.float64)
            joint = lambda t, y: R.joint_lp(head, e64[t], pred(y))     # noqa: E731
            best, best_y, ll = -np.inf, None, None
            for k in range(T + 1):
                for y in itertools.product(range(2), repeat=k):
                    l_ = R.exact_loglik(joint, y, T, 1)
                    if l_ + trie.bonus(y, 1.25) > best:
                        best, best_y, ll = l_ + trie.bonus(y, 1.25), list(y), l_
            assert h["rows"][b][0] == best_y, (hot, b, h["rows"][b], best_y)
            for k, want in (("score", best), ("logp", ll)):
                errs[k] = max(errs.get(k, 0.0), abs(float(h[k][b]) - want))
                assert abs(float(h[k][b]) - want) <= 1e-4 * max(1.0, abs(want)), (hot, b, k, float(h[k][b]), want)
    eng.set_hotwords([])
    report("rnnt_beam_exact_map", **errs)


@pytest.mark.parametrize("V", [34, 1025])
def test_beam_on_peaked_joints_is_greedy(V):
    """One class dominant in every joint call: gam_rnnt_beam gives gam_rnnt_greedy's ids and frames at every width.  "Dominant" is
    checked on the greedy decode's own joint calls (its log-prob dump): an utterance counts when every call's best class leads the
    runner-up by more than PEAK nats; at least a third of them must (measured: half at V = 34, a third at V = 1025), and every one
    that does must match."""
    PEAK = 6.0
    eng, _, cfg, _ = _engine(V, 1, 3.0, out_scale=400.0)
    rng = np.random.default_rng(V)
    B, Tp = 6, 40
    enc = torch.from_numpy((rng.standard_normal((B, 768, Tp)) * 0.5).astype(np.float32))
    elen = torch.tensor([Tp, 31, 1, Tp, 17, Tp], dtype=torch.int32)
    ok = n = 0
    for S in (1, 3, 10):
        dec = eng.rnnt_greedy(enc, elen, S, dump_cap=Tp * (S + 1))
        g, _ = eng.collect(dec)
        dump, dcount = dec[3].cpu().numpy(), dec[4].cpu().tolist()
        assert sum(len(r[0]) for r in g) > 10
        peaked = []
        for b in range(B):
            lp = np.sort(dump[b, : dcount[b]], axis=1)
            peaked.append(bool(dcount[b] == 0 or (lp[:, -1] - lp[:, -2]).min() > PEAK))
        for W in (1, 4, 8, 32):
            h = eng.rnnt_beam(enc, elen, W, S).host()
            for b in range(B):
                n += 1
                if peaked[b]:
                    ok += 1
                    assert h["rows"][b] == g[b], (S, W, b)
    report(f"rnnt_beam_peaked_{V}", qualified=f"{ok}/{n}")
    assert 3 * ok >= n, (ok, n)


def test_op_beam_is_bit_identical_run_to_run_and_on_another_stream():
    eng, head, cfg, _ = _engine(257, 1, None)
    rng = np.random.default_rng(9)
    encp = _encp(rng, 4, 60, cfg["head"]["joint"]["joint_hidden"], 1.0)
    eng.set_hotwords([[1, 2], [5], [7, 7, 3]], 1.0)
    a = _run_op(eng, encp, [60, 45, 60, 7], 8, 10)
    b = _run_op(eng, encp, [60, 45, 60, 7], 8, 10)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = _run_op(eng, encp, [60, 45, 60, 7], 8, 10)
    torch.cuda.synchronize()
    eng.set_hotwords([])
    for o in (b, c):
        assert a["rows"] == o["rows"]
        for k in ("score", "logp"):
            assert a[k].tobytes() == o[k].tobytes(), k


def test_library_rejects_rnnt_beam_search_beyond_the_limits():
    from gigaam_amd._lib import GigaAMHipError
    eng, _, cfg, _ = _engine(34, 1, None)
    JH = cfg["head"]["joint"]["joint_hidden"]
    encp = torch.zeros((1, 10, JH))
    one = torch.tensor([10], dtype=torch.int32)
    for W in (0, 33):
        with pytest.raises(GigaAMHipError, match="beam_size"):
            eng.op_rnnt_beam(encp, one, W, 10)
    with pytest.raises(GigaAMHipError, match="max_symbols"):
        eng.op_rnnt_beam(encp, one, 4, 17)
    d = encp.cuda()
    o = torch.zeros(1024, dtype=torch.int32, device="cuda:0")
    args = [o.data_ptr()] * 5
    rc = eng.lib.gam_op_rnnt_beam(eng._h, d.data_ptr(), one.cuda().data_ptr(), 1, 10, 33, 10, *args, None)
    assert rc != 0 and b"beam width" in eng.lib.gam_last_error(eng._h)
    rc = eng.lib.gam_op_rnnt_beam(eng._h, d.data_ptr(), one.cuda().data_ptr(), 1, 10, 4, 17, *args, None)
    assert rc != 0 and b"max_symbols" in eng.lib.gam_last_error(eng._h)
    rc = eng.lib.gam_op_rnnt_beam(eng._h, d.data_ptr(), one.cuda().data_ptr(), 1, 8193, 4, 10, *args, None)
    assert rc != 0 and b"T'=8193" in eng.lib.gam_last_error(eng._h)
    eng.set_hotwords([[0, 33]])                 # id 33 > V - 2 = 32: refused at the search
    with pytest.raises(GigaAMHipError, match="hotword token id 33"):
        eng.op_rnnt_beam(encp, one, 4, 10)
    eng.set_hotwords([])
    h = eng.op_rnnt_beam(encp, torch.tensor([0], dtype=torch.int32), 4, 10).host()
    assert h["rows"] == [([], [])] and float(h["score"][0]) == 0.0 and float(h["logp"][0]) == 0.0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", RNNT_CASES)
def test_encoded_beam_on_golden_cases_matches_reference(name, mode):
    from gigaam_amd.engine import HipEngine, build_config
    ck, _, _, gold = load_case(name)
    cfg = ck["cfg"]
    eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), ck["state_dict"], torch.device("cuda:0"))
    eng.set_gemm_mode(mode)
    L = cfg["head"]["decoder"]["pred_rnn_layers"]
    S = cfg["decoding"].get("max_symbols_per_step", 10)
    head = R.head_from_state_dict(ck["state_dict"], L)
    enc = torch.from_numpy(gold["encoded"])
    elen = torch.from_numpy(gold["enc_len"])
    errs, ok, n = {}, 0, 0
    for W, hot in ((1, False), (4, False), (8, True)):
        refs = [R.beam_search(head, R.encoder_projection(head, gold["encoded"][b]), W, S, int(gold["enc_len"][b]))
                for b in range(enc.shape[0])]
        phrases = _hotwords(np.random.default_rng(len(name) + W), [r["ids"] for r in refs], cfg["head"]["joint"]["num_classes"], 8) if hot else []
        if hot:
            refs = [R.beam_search(head, R.encoder_projection(head, gold["encoded"][b]), W, S, int(gold["enc_len"][b]), phrases, 2.0)
                    for b in range(enc.shape[0])]
        eng.set_hotwords(phrases, 2.0)
        h = eng.rnnt_beam(enc, elen, W, S).host()
        assert not h["flag"]
        for b, ref in enumerate(refs):
            ok += _compare(h, b, ref, errs, MARGIN_LONG)
            n += 1
    report(f"rnnt_beam_golden_{name}_{mode}", qualified=f"{ok}/{n}", **errs)
    assert 3 * ok >= n, (ok, n)      # (the emission-heavy *_dense cases hold many near-ties over 100 frames)


def test_fullsize32_transcribe_batch_beam_matches_reference():
    """32 x 20 s v2_rnnt through the model at W = 4 (set_decoding) against the reference run on the GPU encoder's output; word
    timestamps come from the beam's token frames.  Also times the beam kernel alone (device events)."""
    from gigaam_amd import workloads
    from gigaam_amd.timestamps_utils import compute_frame_shift, frames_to_words
    model = _fullsize_model()
    model.set_decoding(beam_size=4)
    wav, wlen = workloads.config2_batch(32, 20.0, rank=0)
    got = model.transcribe_batch(wav, wlen, word_timestamps=True)
    eng = model.head.engine
    with torch.inference_mode():
        enc, elen = model._encode(wav.to("cuda:0"), wlen.to("cuda:0"), wlen)
    head = R.head_from_state_dict(model_state(model), 1)
    encd = enc.double().cpu().numpy()
    el = elen.cpu().tolist()
    tok = model.decoding.tokenizer
    ok = 0
    for b in range(32):
        ref = R.beam_search(head, R.encoder_projection(head, encd[b]), 4, 10, el[b])
        if R.min_margin(ref) <= MARGIN_LONG:
            continue
        ok += 1
        text, words = got[b]
        assert text == tok.decode(ref["ids"]), b
        assert words == frames_to_words(tok, ref["ids"], ref["frames"], compute_frame_shift(int(wlen[b]), el[b])), b
    for _ in range(2):
        eng.rnnt_beam(enc, elen, 4, 10)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        eng.rnnt_beam(enc, elen, 4, 10)
    e1.record()
    torch.cuda.synchronize()
    report("rnnt_beam_fullsize32", qualified=f"{ok}/32", beam_w4_ms=e0.elapsed_time(e1) / 5)
    assert ok >= 16, ok


_STATE = {}


def model_state(model):
    """The synthetic full-size checkpoint's state dict (the model hands its tensors to the library and keeps none)."""
    if "v2_rnnt" not in _STATE:
        import json
        import os

        from common import ROOT
        from gigaam_amd import synth
        meta = json.load(open(os.path.join(ROOT, "tests", "golden", "fullsize_meta.json")))["fullsize_v2_rnnt"]
        _STATE["v2_rnnt"] = synth.make_checkpoint("v2_rnnt", seed=0, rnnt_blank_bias=meta.get("blank_bias"))["state_dict"]
    return _STATE["v2_rnnt"]


def test_model_set_decoding_paths_and_greedy_restore(tmp_path):
    """set_decoding(beam_size=4): transcribe, transcribe_batch(word_timestamps=True) and transcribe_longform(speech_regions=...) decode by
    beam (the same text as decode_beam); set_decoding() restores output byte-identical to a fresh greedy model."""
    from gigaam_amd import synth
    model = _small_rnnt_model()
    fresh = _small_rnnt_model()
    wpath = _wav_file(tmp_path, 6.0, 43)
    wav, wlen = synth.synth_audio(2, 3.0, seed=5, lengths=[48000, 31000])
    regions = [(0.0, 2.5), (2.5, 6.0)]
    greedy = (fresh.transcribe(wpath, word_timestamps=True), fresh.transcribe_batch(wav, wlen, word_timestamps=True),
              fresh.transcribe_longform(wpath, speech_regions=regions, word_timestamps=True))
    model.set_decoding(beam_size=4)
    one = model.transcribe(wpath, word_timestamps=True)
    batch = model.transcribe_batch(wav, wlen, word_timestamps=True)
    lf = model.transcribe_longform(wpath, speech_regions=regions, word_timestamps=True)
    with torch.inference_mode():
        enc, elen = model._encode(wav.to("cuda:0"), wlen.to("cuda:0"), wlen)
        beam = model.decoding.decode_beam(model.head, enc, elen)
    assert [t for t, _ in batch] == [r[0] for r in beam]
    for text, ids, frames, score, logp in beam:
        assert len(frames) == len(ids) and frames == sorted(frames) and score == logp and logp <= 0.0
    assert all(w.start <= w.end for _, ws in batch for w in ws)
    assert one.words is not None and len(lf.segments) == len(greedy[2].segments) >= 1
    model.set_decoding()
    again = (model.transcribe(wpath, word_timestamps=True), model.transcribe_batch(wav, wlen, word_timestamps=True),
             model.transcribe_longform(wpath, speech_regions=regions, word_timestamps=True))
    assert repr(again) == repr(greedy)


def test_model_hotword_makes_a_chosen_word_appear(tmp_path):
    """A word built from runner-up tokens of the clip's joint: greedy does not produce it, the beam with it as a hotword does."""
    model = _small_rnnt_model()
    wpath = _wav_file(tmp_path, 8.0, 31)
    greedy = model.transcribe(wpath).text
    tok = model.decoding.tokenizer
    eng = model.head.engine
    wav, wlen = model._prepare_wav_f32(wpath)
    with torch.inference_mode():
        enc, elen = model._encode(wav, wlen)
        dec = eng.rnnt_greedy(enc, elen, 10, dump_cap=4096)
        eng.collect(dec)
    lp = dec[3][0, : int(dec[4][0])].double().cpu().numpy()     # every joint call of the greedy decode, in order
    order = np.argsort(-lp[:, :-1], axis=1, kind="stable")
    word = None
    for i in range(lp.shape[0] - 3):
        cand = [int(order[i + j, 1]) for j in range(3)]
        text = tok.decode(cand)
        if " " not in text and cand[0] != cand[1] and cand[1] != cand[2] and text not in greedy:
            word = text
            break
    assert word is not None
    model.set_decoding(beam_size=8, hotwords=[word], hotword_boost=8.0)
    res = model.transcribe(wpath, word_timestamps=True)
    assert word in res.text, (word, res.text, greedy)
    assert all(w.start <= w.end for w in res.words)
    model.set_decoding(beam_size=8)
    plain = model.transcribe(wpath).text
    assert model.head.engine._hotwords_key[0] == ()
    assert word not in plain or word in greedy


# ---- greedy decode on a head with pred_hidden = joint_hidden = 512: gam_rnnt_greedy_kernel's eight-rows-per-thread instantiation
# (pred_hidden in (320, 512]), which no published checkpoint and no other test reaches.
GREEDY512_SEED = 0                # chosen on the CPU: by the float64 reference alone no utterance has a near-tie (smallest margin 1.4e-2)
GREEDY512_BLANK_BIAS = 9.0        # between the emission-heavy default and the blank-dominant 14: blanks and tokens both occur
GREEDY_MIN_MARGIN = 2e-3          # tests/golden/cases.py RNNT_MIN_MARGIN


def _greedy512_inputs(L):
    """(cfg, state dict, encoded [4, D, 40], enc_len) of the seeded H = JH = 512, V = 34 head."""
    from gigaam_amd import synth
    cfg = synth.model_cfg("v2_rnnt", n_layers=1)
    cfg["head"]["decoder"]["num_classes"] = cfg["head"]["joint"]["num_classes"] = 34
    cfg["head"]["decoder"]["pred_rnn_layers"] = L
    cfg["head"]["decoder"]["pred_hidden"] = cfg["head"]["joint"]["pred_hidden"] = 512
    cfg["head"]["joint"]["joint_hidden"] = 512
    sd = synth.make_state_dict(cfg, seed=500 + L, rnnt_blank_bias=GREEDY512_BLANK_BIAS)
    rng = np.random.default_rng(GREEDY512_SEED * 10 + L)
    encoded = rng.standard_normal((4, cfg["encoder"]["d_model"], 40)).astype(np.float32)
    return cfg, sd, encoded, [40, 23, 1, 0]


@pytest.mark.parametrize("L", [1, 2])
def test_greedy_with_512_hidden_units_matches_float64_reference(L):
    """eng.rnnt_greedy on the one-workgroup kernel (cluster size 0), ragged lengths with 0 and 1: ids, frames and counts are exact for
    every utterance whose float64 top-1 / top-2 margin exceeds 2e-3 on every step; at most one of the four may fall under it."""
    from gigaam_amd.engine import HipEngine, build_config
    S = 3
    cfg, sd, encoded, enc_len = _greedy512_inputs(L)
    head = R.head_from_state_dict(sd, L)
    eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), sd, torch.device("cuda:0"))
    eng.set_rnnt_cluster(0)
    dec = eng.rnnt_greedy(torch.from_numpy(encoded), torch.tensor(enc_len, dtype=torch.int32), S)
    torch.cuda.synchronize()
    ids, frames, counts = dec.ids.cpu().numpy(), dec.frames.cpu().numpy(), dec.counts.cpu().numpy()
    excused, n_tok, n_blank = 0, 0, 0
    for b, T in enumerate(enc_len):
        want_ids, want_frames, margin = R.greedy_ref(head, encoded[b], T, S)      # (the float64 greedy loop: tests/rnnt_beam_ref.py)
        n_tok += len(want_ids)
        n_blank += T - len(set(want_frames))
        if margin <= GREEDY_MIN_MARGIN:
            excused += 1
            continue
        n = int(counts[b])
        assert n == len(want_ids), (L, b, n, len(want_ids))
        assert ids[b, :n].tolist() == want_ids, (L, b)
        assert frames[b, :n].tolist() == want_frames, (L, b)
    report(f"rnnt_greedy_h512_L{L}", excused=excused, tokens=n_tok, blank_frames=n_blank)
    assert n_tok > 0 and n_blank > 0, (n_tok, n_blank)     # the decode emits both
    assert excused <= 1, excused
