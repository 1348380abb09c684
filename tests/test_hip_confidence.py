"""GPU: token confidence (gam_ctc_confidence / gam_op_ctc_confidence / gam_rnnt_confidence / gam_op_rnnt_confidence,
gigaam_amd/csrc/gam_confidence.h) against the float64 reference of tests/confidence_ref.py.

Bar: |conf - ref| <= 1e-3 absolute -- the project's bar for anything derived from log-probs (common.TOL_LOGP), and a confidence is
at most 1.  Span lengths and statuses are compared exactly: the CTC reference reads the SAME fp32 log-probs the kernel read (the
op's input, or the device's own ``ctc_head`` output copied to the host), so an argmax cannot flip on a near tie and no case is left
out.  Every measured worst error goes through ``common.report`` before it is asserted."""
import os

import numpy as np
import pytest
import torch

from beam_common import encp as _encp, run_rnnt_op, small_rnnt_model, wav_file as _wav_file
from common import ROOT, TOL_LOGP, load_case, report, split_ragged

import confidence_ref as C
import rnnt_align_ref as A
import rnnt_beam_ref as R

pytestmark = pytest.mark.gpu

MODES = ["f16x3", "f32"]
MEASURES = ["prob", "entropy"]
AGGS = ["mean", "min", "prod"]
CTC_CASES = ["v1_ctc_l2", "v2_ctc_l2", "v2_ctc_l2_b1", "v2_ctc_l2_short", "v3_ctc_l2", "v3_e2e_ctc_l2"]
RNNT_CASES = ["v1_rnnt_l2", "v2_rnnt_l2", "v3_rnnt_l2", "v3_e2e_rnnt_l2", "v2_rnnt_l2_dense", "v2_rnnt_l2_lstm2", "v3_e2e_rnnt_l2_dense"]
POISON = 0x7fffff00     # in the padding of ids / frames: never read


def _make_engine(cfg, state_dict, mode="f16x3", head=True):
    from gigaam_amd.engine import HipEngine, build_config
    eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg.get("head") if head else None), state_dict, torch.device("cuda:0"))
    eng.set_gemm_mode(mode)
    return eng


_OP_ENGINE = []


def _op_engine():
    if not _OP_ENGINE:
        from gigaam_amd import synth
        _OP_ENGINE.append(_make_engine(synth.model_cfg("v2_ctc"), {}, head=False))
    return _OP_ENGINE[0]


def _log_probs(rng, B, T, V, kind):
    """As tests/test_hip_ctc_align.py: "peaked", "flat", or "dyadic" (unnormalised values in {0, -0.5, -1, -2}: exact argmax ties)."""
    if kind == "dyadic":
        return rng.choice(np.array([0.0, -0.5, -1.0, -2.0], dtype=np.float32), size=(B, T, V))
    x = rng.standard_normal((B, T, V)).astype(np.float32) * (0.3 if kind == "flat" else 1.0)
    if kind == "peaked":
        top = rng.integers(0, V, (B, T))
        np.put_along_axis(x, top[..., None], 9.0, axis=2)
        x[:, 1::2] = x[:, 0::2][:, : x[:, 1::2].shape[1]]          # runs of two frames: spans longer than one
    return torch.log_softmax(torch.from_numpy(x), dim=-1).numpy()


def _padded(rows, cap=None, pad=POISON):
    cap = max([len(r) for r in rows] + [0]) if cap is None else cap
    t = torch.full((len(rows), cap), pad, dtype=torch.int32)
    for i, r in enumerate(rows):
        if len(r):
            t[i, :len(r)] = torch.tensor(r, dtype=torch.int32)
    return t


def _tokens(ids, frames, cap=None):
    return _padded(ids, cap), _padded(frames, cap), torch.tensor([len(r) for r in ids], dtype=torch.int32)


def _check_ctc(h, lp, enc_len, ids, frames, measure, agg, what):
    """Every utterance of a host result against the reference on the fp32 array ``lp``: status and spans exactly, conf within the
    bar, padding -1 / 0, everything in [0, 1].  Returns the worst error."""
    worst = 0.0
    for b in range(len(ids)):
        conf, span, ok = C.ctc_confidence(lp[b], int(enc_len[b]), ids[b], frames[b], measure, agg)
        n = len(ids[b])
        assert int(h["status"][b]) == ok, (what, b)
        assert h["span"][b, :n].tolist() == span, (what, b, h["span"][b, :n].tolist(), span)
        assert (h["conf"][b, n:] == -1.0).all() and (h["span"][b, n:] == 0).all(), (what, b)
        got = h["conf"][b, :n].astype(np.float64)
        if ok:
            assert ((got >= 0.0) & (got <= 1.0)).all(), (what, b)
        if n:
            worst = max(worst, float(np.abs(got - np.asarray(conf)).max()))
    return worst


@pytest.mark.parametrize("V", [34, 257, 1025])
@pytest.mark.parametrize("kind", ["peaked", "flat", "dyadic"])
def test_op_ctc_confidence_matches_float64_reference(kind, V):
    eng = _op_engine()
    rng = np.random.default_rng(V * 3 + len(kind))
    B, Tp = 8, 61
    enc_len = [61, 40, 1, 0, 17, 61, 2, 33]
    lp = _log_probs(rng, B, Tp, V, kind)
    greedy = [C.ctc_greedy(lp[b], enc_len[b]) for b in range(B)]
    rand_ids, rand_frames = [], []
    for b in range(B):           # random tokens at random frames: entry frames whose argmax is another class, spans that meet the next entry
        n = int(rng.integers(0, enc_len[b] + 1)) if enc_len[b] else 0
        fr = sorted(rng.choice(enc_len[b], size=n, replace=False).tolist()) if n else []
        am = [C.argmax_low(lp[b, f]) for f in fr]
        rand_frames.append(fr)
        # half of them the argmax of a LATER frame or of their own (so that spans grow), half anything
        rand_ids.append([int(a) if (a < V - 1 and rng.random() < 0.5) else int(rng.integers(0, V - 1)) for a in am])
    errs = {}
    other = 0
    for which, (ids, frames) in (("greedy", ([g[0] for g in greedy], [g[1] for g in greedy])), ("random", (rand_ids, rand_frames))):
        for measure in MEASURES:
            for agg in AGGS:
                out = eng.op_ctc_confidence(torch.from_numpy(lp), torch.tensor(enc_len, dtype=torch.int32), *_tokens(ids, frames),
                                            measure=measure, aggregation=agg)
                h = out.host()
                assert not h["flag"]
                e = _check_ctc(h, lp, enc_len, ids, frames, measure, agg, (kind, V, which, measure, agg))
                errs[f"{measure}"] = max(errs.get(measure, 0.0), e)
        if which == "random":
            other = sum(C.argmax_low(lp[b, f]) != i for b in range(B) for i, f in zip(ids[b], frames[b]))
    report(f"ctc_confidence_op_{kind}_{V}", **errs)
    assert other >= 5, other
    for k, e in errs.items():
        assert e <= TOL_LOGP, (kind, V, k, e)


def test_op_ctc_confidence_invalid_rows_and_limits():
    from gigaam_amd._lib import GigaAMHipError
    eng = _op_engine()
    rng = np.random.default_rng(7)
    V, Tp = 34, 20
    lp = _log_probs(rng, 8, Tp, V, "flat")
    enc_len = [20, 20, 20, 20, 20, 0, 0, 20]
    ids = [[1, 2, 3], [4, 33, 5], [6, -1], [1, 2], [1, 2], [], [3], [7, 8, 9]]
    frames = [[0, 5, 9], [1, 2, 3], [0, 1], [4, 4], [3, 20], [], [0], [2, 3, 4]]
    want = [1, 0, 0, 0, 0, 1, 0, 1]
    i_t, f_t, cnt = _tokens(ids, frames, 6)
    h = eng.op_ctc_confidence(torch.from_numpy(lp), torch.tensor(enc_len, dtype=torch.int32), i_t, f_t, cnt).host()
    assert h["status"].tolist() == want
    _check_ctc(h, lp, enc_len, ids, frames, "prob", "mean", "invalid")
    for b, ok in enumerate(want):
        if not ok:
            assert (h["conf"][b] == -1.0).all() and (h["span"][b] == 0).all()
    cnt2 = cnt.clone()
    cnt2[0], cnt2[7] = 7, -1                      # counts outside [0, cap]
    h2 = eng.op_ctc_confidence(torch.from_numpy(lp), torch.tensor(enc_len, dtype=torch.int32), i_t, f_t, cnt2).host()
    assert h2["status"].tolist() == [0, 0, 0, 0, 0, 1, 0, 0] and (h2["conf"][0] == -1.0).all() and (h2["conf"][7] == -1.0).all()
    # the same on another stream, bit for bit
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        h3 = eng.op_ctc_confidence(torch.from_numpy(lp), torch.tensor(enc_len, dtype=torch.int32), i_t, f_t, cnt).host()
    torch.cuda.synchronize()
    for k in ("conf", "span", "status"):
        assert h[k].tobytes() == h3[k].tobytes(), k
    # limits and codes are host errors
    d = torch.zeros((1, 4, 34), device="cuda:0")
    one = torch.tensor([4], dtype=torch.int32, device="cuda:0")
    o = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    p = o.data_ptr()
    lib = eng.lib
    assert lib.gam_op_ctc_confidence(eng._h, d.data_ptr(), one.data_ptr(), 1, 8193, 34, p, p, p, 4, 0, 0, p, p, p, None) != 0
    assert b"T'=8193" in lib.gam_last_error(eng._h)
    assert lib.gam_op_ctc_confidence(eng._h, d.data_ptr(), one.data_ptr(), 1, 4, 1026, p, p, p, 4, 0, 0, p, p, p, None) != 0
    assert b"V=1026" in lib.gam_last_error(eng._h)
    assert lib.gam_op_ctc_confidence(eng._h, d.data_ptr(), one.data_ptr(), 1, 4, 34, p, p, p, 4, 2, 0, p, p, p, None) != 0
    assert b"unknown measure 2" in lib.gam_last_error(eng._h)
    assert lib.gam_op_ctc_confidence(eng._h, d.data_ptr(), one.data_ptr(), 1, 4, 34, p, p, p, 4, 0, 3, p, p, p, None) != 0
    assert b"unknown aggregation 3" in lib.gam_last_error(eng._h)
    with pytest.raises(ValueError, match="unknown confidence measure"):
        eng.op_ctc_confidence(d, one, [[1]], [[0]], measure="margin")
    # the op needs no head; the encoded-level entry points of either family refuse this handle with a message
    enc = torch.zeros((1, eng.cfg.d_model, 4), device="cuda:0")
    with pytest.raises(GigaAMHipError, match="CTC head"):
        eng.ctc_confidence(enc, one, [[1]], [[0]])
    with pytest.raises(GigaAMHipError, match="RNN-T head"):
        eng.rnnt_confidence(enc, one, [[1]], [[0]])


# ------------------------------------------------------------------ RNN-T, op level
def _check_rnnt(h, head, encp64, enc_len, ids, frames, measure, what):
    worst = 0.0
    for b in range(len(ids)):
        conf, ok = C.rnnt_confidence(head, encp64[b], int(enc_len[b]), ids[b], frames[b], measure)
        n = len(ids[b])
        assert int(h["status"][b]) == ok, (what, b)
        assert (h["conf"][b, n:] == -1.0).all(), (what, b)
        got = h["conf"][b, :n].astype(np.float64)
        if not ok:
            assert (got == -1.0).all(), (what, b)
        elif n:
            assert ((got >= 0.0) & (got <= 1.0)).all(), (what, b)
            worst = max(worst, float(np.abs(got - np.asarray(conf)).max()))
    return worst


def _random_path(rng, T, n):
    """n token frames of a transducer path: non-decreasing, several tokens on one frame."""
    return sorted(rng.integers(0, T, n).tolist()) if T else []


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["v2_rnnt_l2", "v3_e2e_rnnt_l2"])
def test_op_rnnt_confidence_matches_float64_host_joint(name, mode):
    """The golden greedy decodes, a width-8 beam's decodes and random valid paths with several tokens on one frame, on the encoder
    projection of the golden encoder output (float64 on the host, fp32 on the device)."""
    ck, _, _, gold = load_case(name)
    cfg = ck["cfg"]
    eng = _make_engine(cfg, ck["state_dict"], mode)
    L = cfg["head"]["decoder"]["pred_rnn_layers"]
    S = cfg["decoding"].get("max_symbols_per_step", 10)
    head = R.head_from_state_dict(ck["state_dict"], L)
    V = len(head["out_b"])
    B = len(gold["enc_len"])
    enc_len = gold["enc_len"].tolist()
    encp64 = [R.encoder_projection(head, gold["encoded"][b]) for b in range(B)]
    encp = np.stack(encp64).astype(np.float32)
    encp64 = [e.astype(np.float64) for e in encp]          # the reference reads what the device reads
    elen = torch.tensor(enc_len, dtype=torch.int32)
    rows = split_ragged(gold["ids"], gold["frames"], gold["counts"].tolist())
    beam = run_rnnt_op(eng, encp, enc_len, 8, S)
    rng = np.random.default_rng(len(name))
    rand = []
    for b in range(B):
        n = int(rng.integers(3, 40))
        rand.append((rng.integers(0, V - 1, n).tolist(), _random_path(rng, min(enc_len[b], 12), n)))
    assert any(len(set(f)) < len(f) for _, f in rand)
    errs = {}
    for which, rws in (("greedy", rows), ("beam", beam["rows"]), ("random", rand)):
        ids, frames = [r[0] for r in rws], [r[1] for r in rws]
        for measure in MEASURES:
            out = eng.op_rnnt_confidence(torch.from_numpy(encp), elen, *_tokens(ids, frames), measure=measure)
            assert out.span is None
            h = out.host()
            assert not h["flag"] and h["status"].tolist() == [1] * B, (which, h["status"].tolist())
            e = _check_rnnt(h, head, encp64, enc_len, ids, frames, measure, (name, mode, which, measure))
            errs[measure] = max(errs.get(measure, 0.0), e)
    # the same decode as the decoder's own object, whose buffer is T' * max_symbols wide.  The pp GEMM then runs on B x (cap + 1)
    # rows, and its tile plan -- hence the order of its sums -- depends on the row count: the two widths agree to rounding, not bit
    # for bit, so the wide call is held to the same reference and bar (its gap to the narrow call is recorded)
    dec = eng.op_rnnt_beam(torch.from_numpy(encp), elen, 8, S)
    bids, bfr = [r[0] for r in beam["rows"]], [r[1] for r in beam["rows"]]
    for measure in MEASURES:
        wide = eng.op_rnnt_confidence(torch.from_numpy(encp), elen, dec, measure=measure)
        assert wide.cap == min(dec.ids.shape[1], 1024)
        h = wide.host()
        assert h["status"].tolist() == [1] * B
        errs[measure] = max(errs[measure], _check_rnnt(h, head, encp64, enc_len, bids, bfr, measure, (name, mode, "decoded", measure)))
        narrow = eng.op_rnnt_confidence(torch.from_numpy(encp), elen, *_tokens(bids, bfr), measure=measure).host()
        for b, ids in enumerate(bids):
            if ids:
                errs["wide_vs_narrow"] = max(errs.get("wide_vs_narrow", 0.0),
                                             float(np.abs(h["conf"][b, :len(ids)].astype(np.float64) - narrow["conf"][b, :len(ids)]).max()))
    report(f"rnnt_confidence_op_{name}_{mode}", **errs)
    for k, e in errs.items():
        assert e <= TOL_LOGP, (name, mode, k, e)


def test_op_rnnt_confidence_invalid_rows_limits_and_workspace():
    from gigaam_amd._lib import GigaAMHipError
    ck, _, _, gold = load_case("v2_rnnt_l2")
    eng = _make_engine(ck["cfg"], ck["state_dict"])
    head = R.head_from_state_dict(ck["state_dict"], 1)
    rng = np.random.default_rng(3)
    JH = eng.cfg.joint_hidden
    encp = _encp(rng, 7, 10, JH, 1.0)
    enc_len = [10, 10, 10, 10, 0, 0, 10]
    ids = [[1, 2, 3, 4], [4, 33, 5], [6, -1], [1, 2], [], [3], [7] * 20]
    frames = [[0, 0, 0, 9], [1, 2, 3], [0, 1], [4, 3], [], [0], [5] * 20]
    want = [1, 0, 0, 0, 1, 0, 1]
    i_t, f_t, cnt = _tokens(ids, frames)
    elen = torch.tensor(enc_len, dtype=torch.int32)
    h = eng.op_rnnt_confidence(torch.from_numpy(encp), elen, i_t, f_t, cnt).host()
    assert h["status"].tolist() == want
    e = _check_rnnt(h, head, encp.astype(np.float64), enc_len, ids, frames, "prob", "invalid")
    assert e <= TOL_LOGP, e
    cnt2 = cnt.clone()
    cnt2[0] = 21
    assert eng.op_rnnt_confidence(torch.from_numpy(encp), elen, i_t, f_t, cnt2).host()["status"].tolist() == [0, 0, 0, 0, 1, 0, 1]
    # the alignment's workspace limit slices the lattice, which this pass does not build: the results do not change
    try:
        eng.set_rnnt_align_workspace(4096)
        h2 = eng.op_rnnt_confidence(torch.from_numpy(encp), elen, i_t, f_t, cnt).host()
    finally:
        eng.set_rnnt_align_workspace(0)
    assert h2["conf"].tobytes() == h["conf"].tobytes() and h2["status"].tolist() == want
    # limits are host errors
    d = torch.zeros((1, 10, JH), device="cuda:0")
    one = torch.tensor([10], dtype=torch.int32, device="cuda:0")
    o = torch.zeros(4096, dtype=torch.int32, device="cuda:0")
    p = o.data_ptr()
    lib = eng.lib
    assert lib.gam_op_rnnt_confidence(eng._h, d.data_ptr(), one.data_ptr(), 1, 10, p, p, p, 1025, 0, p, p, None) != 0
    assert b"cap=1025" in lib.gam_last_error(eng._h)
    assert lib.gam_op_rnnt_confidence(eng._h, d.data_ptr(), one.data_ptr(), 1, 8193, p, p, p, 4, 0, p, p, None) != 0
    assert b"T'=8193" in lib.gam_last_error(eng._h)
    with pytest.raises(GigaAMHipError, match="encp must be"):
        eng.op_rnnt_confidence(torch.zeros((1, 10, 64)), one, [[1]], [[0]])
    # the wrong family: an error string, no fault
    with pytest.raises(GigaAMHipError, match="model has no CTC head"):
        eng.ctc_confidence(torch.from_numpy(gold["encoded"]), torch.from_numpy(gold["enc_len"]), [[1]] * len(gold["enc_len"]),
                           [[0]] * len(gold["enc_len"]))
    ckc, _, _, goldc = load_case("v2_ctc_l2")
    engc = _make_engine(ckc["cfg"], ckc["state_dict"])
    n = len(goldc["enc_len"])
    with pytest.raises(GigaAMHipError, match="model has no RNN-T head"):
        engc.rnnt_confidence(torch.from_numpy(goldc["encoded"]), torch.from_numpy(goldc["enc_len"]), [[1]] * n, [[0]] * n)


# ------------------------------------------------------------------ through the model
def _same_transcript(res, want):
    for r, (text, words) in zip(res, want):
        assert r.feasible and r.text == text and str(r) == text
        assert [(w.text, w.start, w.end) for w in r.words] == [(w.text, w.start, w.end) for w in words]
        assert len(r.token_ids) == len(r.token_frames) == len(r.token_confidence)
        assert all(0.0 <= c <= 1.0 for c in r.token_confidence) and all(0.0 <= w.confidence <= 1.0 for w in r.words)
        assert (r.confidence is None) == (not r.token_ids)


def _words_follow_tokens(model, r, agg):
    tok = model.decoding.tokenizer
    want = C.word_confidences(tok, r.token_ids, r.token_confidence, agg)
    assert [w.confidence for w in r.words] == pytest.approx(want, abs=1e-12)
    u = C.aggregate(r.token_confidence, agg)
    assert r.confidence == (None if u is None else pytest.approx(u, abs=1e-12))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CTC_CASES)
def test_model_confidence_on_golden_ctc_cases(name, mode):
    import gigaam_amd
    ck, wav, wlen, gold = load_case(name)
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    model.set_arithmetic(mode)
    want = model.transcribe_batch(wav, wlen, word_timestamps=True)
    decoded = model.decoding.decode(model.head, *model._encode(wav.to("cuda:0"), wlen.to("cuda:0"), wlen))
    encoded, enc_len = model._encode(wav.to("cuda:0"), wlen.to("cuda:0"), wlen)
    lp = model.head.engine.ctc_head(encoded).cpu().numpy()       # the device's own log-probs: what the confidence pass reads
    T = enc_len.cpu().tolist()
    errs = {}
    for measure in MEASURES:
        for agg in AGGS:
            res = model.confidence_batch(wav, wlen, measure=measure, aggregation=agg)
            _same_transcript(res, want)
            for b, r in enumerate(res):
                assert (r.token_ids, r.token_frames) == (decoded[b][1], decoded[b][2])
                conf, span, ok = C.ctc_confidence(lp[b], T[b], r.token_ids, r.token_frames, measure, agg)
                assert ok == 1
                if conf:
                    errs[measure] = max(errs.get(measure, 0.0), float(np.abs(np.asarray(r.token_confidence) - np.asarray(conf)).max()))
                _words_follow_tokens(model, r, agg)
    # a known transcript: the decode's own ids, aligned -- the frames are align_batch's
    texts = [d[1] for d in decoded]
    al = model.align_batch(wav, wlen, texts)
    res = model.confidence_batch(wav, wlen, texts, measure="prob", aggregation="min")
    for b, (r, a) in enumerate(zip(res, al)):
        assert r.feasible == a.feasible and r.token_ids == a.token_ids and r.token_frames == a.token_frames and r.text == a.text
        assert [(w.text, w.start, w.end) for w in r.words] == [(w.text, w.start, w.end) for w in a.words]
        conf, _, ok = C.ctc_confidence(lp[b], T[b], r.token_ids, r.token_frames, "prob", "min")
        assert ok == 1
        if conf:
            errs["aligned"] = max(errs.get("aligned", 0.0), float(np.abs(np.asarray(r.token_confidence) - np.asarray(conf)).max()))
    report(f"ctc_confidence_model_{name}_{mode}", **errs)
    for k, e in errs.items():
        assert e <= TOL_LOGP, (name, mode, k, e)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", RNNT_CASES)
def test_model_confidence_on_golden_rnnt_cases(name, mode):
    import gigaam_amd
    ck, wav, wlen, gold = load_case(name)
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    model.set_arithmetic(mode)
    L = ck["cfg"]["head"]["decoder"]["pred_rnn_layers"]
    head = R.head_from_state_dict(ck["state_dict"], L)
    want = model.transcribe_batch(wav, wlen, word_timestamps=True)
    encoded, enc_len = model._encode(wav.to("cuda:0"), wlen.to("cuda:0"), wlen)
    enc_h, T = encoded.double().cpu().numpy(), enc_len.cpu().tolist()
    encp64 = [R.encoder_projection(head, enc_h[b]) for b in range(len(T))]
    errs = {}
    res_by = {}
    for measure in MEASURES:
        res = res_by[measure] = model.confidence_batch(wav, wlen, measure=measure, aggregation="prod")
        _same_transcript(res, want)
        for b, r in enumerate(res):
            conf, ok = C.rnnt_confidence(head, encp64[b], T[b], r.token_ids, r.token_frames, measure)
            assert ok == 1
            if conf:
                errs[measure] = max(errs.get(measure, 0.0), float(np.abs(np.asarray(r.token_confidence) - np.asarray(conf)).max()))
            _words_follow_tokens(model, r, "prod")
    # the emission part of the greedy path cannot beat the Viterbi path of the same ids once the blank terms (<= 0) are added back
    texts = [r.token_ids for r in res_by["prob"]]
    al = model.rnnt_align_batch(wav, wlen, texts)
    gap = 0.0
    for r, a in zip(res_by["prob"], al):
        if r.token_ids and min(r.token_confidence) > 0.0:
            s = float(np.log(np.asarray(r.token_confidence, dtype=np.float64)).sum())
            gap = max(gap, a.score - s)
            assert s >= a.score - 1e-3 * max(1.0, abs(a.score)), (name, mode, s, a.score)
    errs["score_minus_sum_ln"] = gap
    # a known transcript, aligned: the frames are rnnt_align_batch's
    res = model.confidence_batch(wav, wlen, texts, measure="prob", aggregation="mean")
    for b, (r, a) in enumerate(zip(res, al)):
        assert r.feasible == a.feasible and r.token_ids == a.token_ids and r.token_frames == a.token_frames and r.text == a.text
        assert [(w.text, w.start, w.end) for w in r.words] == [(w.text, w.start, w.end) for w in a.words]
        conf, ok = C.rnnt_confidence(head, encp64[b], T[b], r.token_ids, r.token_frames, "prob")
        assert ok == 1
        if conf:
            errs["aligned"] = max(errs.get("aligned", 0.0), float(np.abs(np.asarray(r.token_confidence) - np.asarray(conf)).max()))
    report(f"rnnt_confidence_model_{name}_{mode}", **errs)
    for k in ("prob", "entropy", "aligned"):
        assert errs.get(k, 0.0) <= TOL_LOGP, (name, mode, k, errs[k])


def test_model_confidence_single_clip_beam_and_errors(tmp_path):
    import gigaam_amd
    from gigaam_amd import synth
    ctc = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=0, n_layers=2), "cuda:0")
    path = _wav_file(tmp_path, 6, 5)
    want = ctc.transcribe(path, word_timestamps=True)
    r = ctc.confidence(path)
    assert r.text == want.text and [(w.text, w.start, w.end) for w in r.words] == [(w.text, w.start, w.end) for w in want.words]
    wb = ctc.transcribe(path, word_timestamps=True, beam_size=4)
    rb = ctc.confidence(path, beam_size=4, measure="entropy", aggregation="min")
    assert rb.text == wb.text and [(w.text, w.start, w.end) for w in rb.words] == [(w.text, w.start, w.end) for w in wb.words]
    if want.text:
        known = ctc.confidence(path, want.text)
        assert known.text == want.text and known.token_frames == ctc.align(path, want.text).token_frames
    with pytest.raises(ValueError, match="cannot be aligned"):
        ctc.confidence(path, [1, 1] * 400)
    infeasible = ctc.confidence_batch(*synth.synth_audio(1, 1.0, seed=2), [[1, 1] * 400])[0]
    assert not infeasible.feasible and infeasible.words == [] and infeasible.token_confidence == [] and infeasible.confidence is None
    rnnt, _ = small_rnnt_model()
    wr = rnnt.transcribe(path, word_timestamps=True)
    rr = rnnt.confidence(path)
    assert rr.text == wr.text and [(w.text, w.start, w.end) for w in rr.words] == [(w.text, w.start, w.end) for w in wr.words]
    rnnt.set_decoding(beam_size=4)
    try:
        wr4 = rnnt.transcribe(path, word_timestamps=True)
        rr4 = rnnt.confidence(path, measure="entropy")
        assert rr4.text == wr4.text and [(w.text, w.start, w.end) for w in rr4.words] == [(w.text, w.start, w.end) for w in wr4.words]
        with pytest.raises(TypeError, match="beam search needs a CTC head"):
            rnnt.confidence(path, beam_size=4)
    finally:
        rnnt.set_decoding()
