"""GPU: CTC forced alignment (gam_op_ctc_align / gam_ctc_align, gigaam_amd/csrc/gam_align.h) against the float64 reference of
tests/ctc_align_ref.py and torch's CTC loss, on the golden greedy decodes, on the full-size 32 x 20 s batch, and through the model."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from common import ROOT, load_case, report, split_ragged

import ctc_align_ref as R

pytestmark = pytest.mark.gpu

MODES = ["f16x3", "f32"]
CTC_CASES = ["v1_ctc_l2", "v2_ctc_l2", "v3_ctc_l2", "v3_e2e_ctc_l2"]


def _bar(ref):
    return 1e-3 * max(1.0, abs(ref))


def _make_engine(cfg, state_dict, mode="f16x3", head=True):
    from gigaam_amd.engine import HipEngine, build_config
    eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg.get("head") if head else None), state_dict,
                    torch.device("cuda:0"))
    eng.set_gemm_mode(mode)
    return eng


_OP_ENGINE = []


def _op_engine():
    if not _OP_ENGINE:
        from gigaam_amd import synth
        _OP_ENGINE.append(_make_engine(synth.model_cfg("v2_ctc"), {}, head=False))
    return _OP_ENGINE[0]


def _log_probs(rng, B, T, V, kind):
    """Seeded log-probs [B, T, V] (float32, log_softmax units): "peaked" (one dominant class per frame), "flat" (small logits:
    many near-equal paths) or "dyadic" (unnormalised values in {0, -0.5, -1, -2}: exact ties in fp32 and fp64 alike)."""
    if kind == "dyadic":
        return rng.choice(np.array([0.0, -0.5, -1.0, -2.0], dtype=np.float32), size=(B, T, V))
    x = rng.standard_normal((B, T, V)).astype(np.float32) * (0.3 if kind == "flat" else 1.0)
    if kind == "peaked":
        top = rng.integers(0, V, (B, T))
        np.put_along_axis(x, top[..., None], 9.0, axis=2)
    return torch.log_softmax(torch.from_numpy(x), dim=-1).numpy()


def _target(rng, U, V, repeats=0):
    y = rng.integers(0, V - 1, U)
    for i in rng.choice(np.arange(1, U), size=min(repeats, max(U - 1, 0)), replace=False) if U > 1 else []:
        y[i] = y[i - 1]
    return [int(v) for v in y]


def _run_op(eng, lp, enc_len, targets, target_len=None, pad=None):
    """gam_op_ctc_align on numpy inputs -> host dict.  ``pad``: value written into targets past target_len."""
    B = lp.shape[0]
    um = max([len(t) for t in targets] + [0])
    tgt = torch.full((B, um), 0 if pad is None else pad, dtype=torch.int32)
    for i, t in enumerate(targets):
        tgt[i, : len(t)] = torch.tensor(t, dtype=torch.int32)
    tl = torch.tensor([len(t) for t in targets] if target_len is None else target_len, dtype=torch.int32)
    out = eng.op_ctc_align(torch.from_numpy(np.ascontiguousarray(lp)), torch.tensor(enc_len, dtype=torch.int32), tgt, tl)
    return out.host()


def _torch_loglik(lp, T, y):
    V = lp.shape[1]
    if not R.feasible(T, y, V) or T == 0:
        return R.forward_loglik(lp, y, T)
    loss = F.ctc_loss(torch.from_numpy(np.asarray(lp[:T], dtype=np.float64))[:, None, :], torch.tensor([y], dtype=torch.long),
                      torch.tensor([T]), torch.tensor([len(y)]), blank=V - 1, reduction="none", zero_infinity=False)
    return -float(loss[0])


def _check_utterance(h, b, lp, T, y, errs, exact_path=False):
    """Status, score, log-likelihood, path validity and rescore of utterance b of a result against the float64 reference."""
    V = lp.shape[1]
    Tp = h["frame_labels"].shape[1]
    score, states = R.viterbi(lp, y, T)
    ok = states is not None
    assert int(h["status"][b]) == int(ok), (b, T, len(y))
    if not ok:
        assert h["score"][b] == -np.inf and h["loglik"][b] == -np.inf
        assert (h["frame_labels"][b] == -1).all()
        assert (h["tok_first"][b] == -1).all() and (h["tok_last"][b] == -1).all()
        return
    ll = _torch_loglik(lp, T, y)
    e_s, e_l = abs(float(h["score"][b]) - score), abs(float(h["loglik"][b]) - ll)
    errs["score"] = max(errs.get("score", 0.0), e_s / max(1.0, abs(score)))
    errs["loglik"] = max(errs.get("loglik", 0.0), e_l / max(1.0, abs(ll)))
    assert e_s <= _bar(score), (b, float(h["score"][b]), score)
    assert e_l <= _bar(ll), (b, float(h["loglik"][b]), ll)
    labels = h["frame_labels"][b]
    assert (labels[T:] == -1).all()
    got_states = R.path_states(labels[:T].tolist(), y, V - 1)
    assert got_states is not None, (b, "not a CTC path of the target")
    first, last = R.token_runs(got_states, len(y))
    U = len(y)
    assert h["tok_first"][b, :U].tolist() == first and h["tok_last"][b, :U].tolist() == last
    assert (h["tok_first"][b, U:] == -1).all() and (h["tok_last"][b, U:] == -1).all()
    e_r = abs(R.rescore(lp, labels[:T]) - score)
    errs["rescore"] = max(errs.get("rescore", 0.0), e_r / max(1.0, abs(score)))
    assert e_r <= _bar(score), (b, "returned path is not optimal", e_r)
    if exact_path:
        assert got_states == states, (b, "tie rule")
    assert labels.shape[0] == Tp


@pytest.mark.parametrize("V,Tp", [(34, 160), (257, 400), (1025, 625)])
@pytest.mark.parametrize("kind", ["peaked", "flat"])
def test_op_align_matches_float64_reference(V, Tp, kind):
    eng = _op_engine()
    rng = np.random.default_rng(V * 7 + Tp + (1 if kind == "flat" else 0))
    # (U, repeats, T): empty, short, repeated tokens, exactly minimal T (None), near T, T = 0 with U = 0, ragged
    plan = [(0, 0, Tp), (1, 0, Tp // 3), (12, 4, Tp), (40, 10, None), (Tp // 4, 3, Tp - 7), (Tp // 2, 0, Tp),
            (0, 0, 0), (30, 5, Tp // 2)]
    targets = [_target(rng, U, V, r) for U, r, _ in plan]
    enc_len = [T if T is not None else len(y) + sum(y[i] == y[i - 1] for i in range(1, len(y))) for (_, _, T), y in zip(plan, targets)]
    lp = _log_probs(rng, len(plan), Tp, V, kind)
    h = _run_op(eng, lp, enc_len, targets, pad=-12345)
    errs = {}
    for b, y in enumerate(targets):
        _check_utterance(h, b, lp[b], enc_len[b], y, errs)
    assert int(h["status"][3]) == 1       # exactly minimal T aligns
    assert h["score"][6] == 0.0 and h["loglik"][6] == 0.0 and int(h["status"][6]) == 1
    report(f"ctc_align_op_V{V}_T{Tp}_{kind}", **errs)


def test_op_align_large_targets_past_the_lds_budget():
    """U = 600 at T' = 625 (S = 1201: the 2-bit backpointers need 190 KB, beyond the workgroup's LDS) and U = 1024 (the limit)
    use the global backpointer scratch; U = 1024 in 625 frames is infeasible."""
    eng = _op_engine()
    rng = np.random.default_rng(11)
    V, Tp = 1025, 1100
    plan = [(600, 0, 625), (300, 20, 625), (1024, 0, 1100), (1024, 0, 625), (1000, 30, 1100)]
    targets = [_target(rng, U, V, r) for U, r, _ in plan]
    enc_len = [T for _, _, T in plan]
    for kind in ("peaked", "flat"):
        lp = _log_probs(rng, len(plan), Tp, V, kind)
        h = _run_op(eng, lp, enc_len, targets, pad=V + 77)
        errs = {}
        for b, y in enumerate(targets):
            _check_utterance(h, b, lp[b], enc_len[b], y, errs)
        assert h["status"].tolist() == [1, 1, 1, 0, 1]
        report(f"ctc_align_op_large_U_{kind}", **errs)


def test_op_align_infeasible_and_bad_ids():
    eng = _op_engine()
    rng = np.random.default_rng(5)
    V, Tp = 34, 60
    lp = _log_probs(rng, 7, Tp, V, "peaked")
    targets = [
        [1, 1, 1, 2],              # needs 4 + 2 = 6 frames: T = 5 -> infeasible
        [1, 1, 1, 2],              # T = 6 -> exactly feasible
        [3, V - 1, 4],             # the blank id inside a target
        [3, -3, 4],                # negative id
        [3, V + 5, 4],             # beyond the vocabulary
        list(range(30)),           # 30 tokens in 29 frames
        [5, 6, 7],                 # valid, with garbage past target_len (below)
    ]
    enc_len = [5, 6, Tp, Tp, Tp, 29, 40]
    h = _run_op(eng, lp, enc_len, targets)
    assert h["status"].tolist() == [0, 1, 0, 0, 0, 0, 1]
    errs = {}
    for b, y in enumerate(targets):
        _check_utterance(h, b, lp[b], enc_len[b], y, errs)
    # target_len shorter than the row: entries past it are never read, whatever they hold
    um = 8
    tgt = torch.full((2, um), 2 ** 30, dtype=torch.int32)
    tgt[0, :3] = torch.tensor([5, 6, 7])
    tgt[1, :2] = torch.tensor([9, 9])
    out = eng.op_ctc_align(torch.from_numpy(lp[:2]), torch.tensor([40, 40], dtype=torch.int32), tgt,
                           torch.tensor([3, 2], dtype=torch.int32)).host()
    for b, y in enumerate([[5, 6, 7], [9, 9]]):
        _check_utterance(out, b, lp[b], 40, y, errs)
    # target_len outside [0, Umax]: infeasible, not a read past the row
    out = eng.op_ctc_align(torch.from_numpy(lp[:2]), torch.tensor([40, 40], dtype=torch.int32), tgt,
                           torch.tensor([um + 1, -1], dtype=torch.int32)).host()
    assert out["status"].tolist() == [0, 0]


def test_op_align_exact_ties_follow_the_tie_rule():
    eng = _op_engine()
    rng = np.random.default_rng(21)
    for V, Tp in ((4, 40), (34, 120)):
        plan = [(3, 1, 12), (8, 2, Tp), (0, 0, Tp // 2), (15, 5, 40), (5, 0, Tp)]
        targets = [_target(rng, U, V, r) for U, r, _ in plan]
        enc_len = [min(T, Tp) for _, _, T in plan]
        lp = _log_probs(rng, len(plan), Tp, V, "dyadic")
        h = _run_op(eng, lp, enc_len, targets)
        errs = {}
        for b, y in enumerate(targets):
            _check_utterance(h, b, lp[b], enc_len[b], y, errs, exact_path=True)


def test_op_align_is_bit_identical_on_another_stream():
    eng = _op_engine()
    rng = np.random.default_rng(9)
    V, Tp = 257, 300
    targets = [_target(rng, U, V, 3) for U in (20, 100, 140)]
    lp = _log_probs(rng, 3, Tp, V, "flat")
    a = _run_op(eng, lp, [Tp, 250, Tp], targets)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        b = _run_op(eng, lp, [Tp, 250, Tp], targets)
    torch.cuda.synchronize()
    for k in ("frame_labels", "tok_first", "tok_last", "status"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("score", "loglik"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_library_rejects_shapes_beyond_the_limits():
    from gigaam_amd._lib import GigaAMHipError
    eng = _op_engine()
    lp = torch.zeros((1, 10, 5))
    with pytest.raises(GigaAMHipError, match="Umax"):
        eng.op_ctc_align(lp, torch.tensor([10], dtype=torch.int32), torch.zeros((1, 1025), dtype=torch.int32))


def _golden_margins(lp):
    top = np.sort(np.asarray(lp, dtype=np.float64), axis=1)
    return top[:, -1] - top[:, -2]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CTC_CASES)
def test_encoded_align_of_golden_ids_gives_golden_frames(name, mode):
    """The greedy path is the optimum of its own transcript: aligning the golden ids on the golden encoder output gives back the
    golden frames wherever the frame boundary is not a near-tie, and scores the sum of per-frame maxima."""
    ck, _, _, gold = load_case(name)
    eng = _make_engine(ck["cfg"], ck["state_dict"], mode)
    ref = split_ragged(gold["ids"], gold["frames"], gold["counts"].tolist())
    enc = torch.from_numpy(gold["encoded"])
    elen = torch.from_numpy(gold["enc_len"])
    h = eng.ctc_align(enc, elen, [ids for ids, _ in ref]).host()
    assert not h["flag"]
    checked, err = 0, 0.0
    for b, (ids, frames) in enumerate(ref):
        T = int(gold["enc_len"][b])
        lp = gold["log_probs"][b][:T]
        assert int(h["status"][b]) == 1
        best = float(lp.astype(np.float64).max(axis=1).sum())
        err = max(err, abs(float(h["score"][b]) - best) / max(1.0, abs(best)))
        assert abs(float(h["score"][b]) - best) <= _bar(best)
        m = _golden_margins(lp)
        first = h["tok_first"][b, : len(ids)].tolist()
        for u, f in enumerate(frames):
            if min(m[max(f - 1, 0)], m[f]) > 1e-3:
                assert first[u] == f, (b, u)
                checked += 1
        ll = _torch_loglik(lp, T, ids)
        assert abs(float(h["loglik"][b]) - ll) <= _bar(ll)
    assert checked >= 0.8 * len(gold["ids"])
    report(f"ctc_align_golden_{name}_{mode}", score_rel_err=err, tokens_checked=checked, tokens=int(len(gold["ids"])))


def test_fullsize32_align_of_golden_ids():
    """The 32 x 20 s, 16-layer batch of test_hip_fullsize.py: align the golden greedy ids on this path's own encoder output; the
    best path scores the sum of the head's per-frame maxima and gives back the golden frames (min margin per utterance: the
    golden min_margin).  Also times the alignment kernel alone on the head's log-probs."""
    from gigaam_amd import synth, workloads
    path = os.path.join(ROOT, "tests", "golden", "fullsize32_v2_ctc.npz")
    gold = dict(np.load(path))
    ck = synth.make_checkpoint("v2_ctc", seed=0)
    eng = _make_engine(ck["cfg"], ck["state_dict"])
    wav, wlen = workloads.config2_batch(32, 20.0, rank=0)
    enc, elen = eng.encode(*eng.frontend(wav, wlen))
    assert elen.cpu().tolist() == gold["enc_len"].tolist()
    ref = split_ragged(gold["ids"], gold["frames"], gold["counts"].tolist())
    targets = [ids for ids, _ in ref]
    h = eng.ctc_align(enc, elen, targets).host()
    assert not h["flag"]
    lp = eng.ctc_head(enc).double().cpu().numpy()
    margins = gold["min_margin"].tolist()
    exact, err = 0, 0.0
    for b, (ids, frames) in enumerate(ref):
        T = int(gold["enc_len"][b])
        assert int(h["status"][b]) == 1
        best = float(lp[b, :T].max(axis=1).sum())
        err = max(err, abs(float(h["score"][b]) - best) / max(1.0, abs(best)))
        assert abs(float(h["score"][b]) - best) <= _bar(best)
        first = h["tok_first"][b, : len(ids)].tolist()
        if margins[b] > 1e-3:
            assert first == frames, b
        exact += first == frames
        ll = _torch_loglik(lp[b], T, ids)
        assert abs(float(h["loglik"][b]) - ll) <= _bar(ll)
    assert sum(1 for m in margins if m > 1e-3) >= 16
    # the kernel alone (gam_op_ctc_align on the head's log-probs), device events
    lp_d = torch.from_numpy(lp.astype(np.float32)).cuda()
    um = max(len(t) for t in targets)
    tgt = torch.zeros((32, um), dtype=torch.int32)
    for i, t in enumerate(targets):
        tgt[i, : len(t)] = torch.tensor(t, dtype=torch.int32)
    tgt, tlen = tgt.cuda(), torch.tensor([len(t) for t in targets], dtype=torch.int32).cuda()
    for _ in range(2):
        eng.op_ctc_align(lp_d, elen, tgt, tlen)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    n = 10
    for _ in range(n):
        eng.op_ctc_align(lp_d, elen, tgt, tlen)
    e1.record()
    torch.cuda.synchronize()
    report("ctc_align_fullsize32", score_rel_err=err, utterances_exact=f"{exact}/32", min_margin=min(margins),
           op_align_ms=e0.elapsed_time(e1) / n, tokens=int(len(gold["ids"])))
    assert exact >= 24


def _wav_file(tmp_path, seconds, seed):
    import wave
    from gigaam_amd import synth
    wav, _ = synth.synth_audio(1, seconds, seed=seed)
    pcm = (wav[0].numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16)
    p = str(tmp_path / f"clip{seed}.wav")
    with wave.open(p, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(16000)
        wf.writeframes(pcm.tobytes())
    return p


def test_model_align_reproduces_transcribe_word_timestamps(tmp_path):
    import gigaam_amd
    from gigaam_amd import synth
    from gigaam_amd.types import AlignmentResult
    ck = synth.make_checkpoint("v2_ctc", seed=1, n_layers=2)
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    wpath = _wav_file(tmp_path, 12.0, 17)
    res = model.transcribe(wpath, word_timestamps=True)
    al = model.align(wpath, model.transcribe(wpath).text)
    assert isinstance(al, AlignmentResult) and al.feasible
    assert al.text == res.text
    assert al.words == res.words
    assert al.score <= 0.0 and al.log_likelihood >= al.score - 1e-3
    # too long for the clip: ValueError from align, feasible=False from align_batch
    with pytest.raises(ValueError):
        model.align(wpath, "а" * 400)
    wav, wlen = synth.synth_audio(2, 3.0, seed=5, lengths=[48000, 31000])
    out = model.align_batch(wav, wlen, ["а б в", "а" * 400])
    assert out[0].feasible and not out[1].feasible
    assert out[1].words == [] and out[1].score == -np.inf and out[1].log_likelihood == -np.inf
    with pytest.raises(ValueError):
        model.align(wpath, "abc")           # Latin letters: not in the vocabulary


def test_model_align_batch_with_sentencepiece_ids(tmp_path):
    import gigaam_amd
    from gigaam_amd import synth
    ck = synth.make_checkpoint("v3_e2e_ctc", seed=1, n_layers=2)
    ck["cfg"]["decoding"]["model_path"] = os.path.join(ROOT, "tests", "golden", "spm256.model")
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    wav, wlen = synth.synth_audio(2, 6.0, seed=23, lengths=[96000, 70000])
    want = model.transcribe_batch(wav, wlen, word_timestamps=True)
    with torch.inference_mode():
        enc, elen = model._encode(wav.to("cuda:0"), wlen.to("cuda:0"), wlen)
        dec = model.decoding.decode(model.head, enc, elen)
    ids = [d[1] for d in dec]
    got = model.align_batch(wav, wlen, ids)
    for g, w, i in zip(got, want, ids):
        assert g.feasible and g.token_ids == i
        assert g.words == w[1]


def test_model_align_needs_a_ctc_head(tmp_path):
    import gigaam_amd
    from gigaam_amd import synth
    ck = synth.make_checkpoint("v2_rnnt", seed=1, n_layers=1)
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    wav, wlen = synth.synth_audio(1, 2.0, seed=3)
    with pytest.raises(TypeError, match="forced alignment needs a CTC head"):
        model.align_batch(wav, wlen, ["а"])
    with pytest.raises(TypeError, match="forced alignment needs a CTC head"):
        model.align(_wav_file(tmp_path, 2.0, 3), "а")
