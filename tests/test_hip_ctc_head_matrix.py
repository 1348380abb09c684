"""GPU: the kernels every CTC transcription ends in -- the token transpose, the head GEMM, gam_log_softmax_kernel and the batched
gam_ctc_greedy_kernel (gam_decode.h) -- and gam_emo_head_kernel, on the crafted inputs of tests/ctc_head_cases.py against its numpy /
float64 reference.  One engine per head, cached.

Exactness: tests/test_ctc_head_cases_host.py asserts on the CPU that every frame of every label-built case has a float64 top-1 /
top-2 margin above 2e-3 (twice TOL_LOGP), and that every listed tie is an exact tie in float32, so no frame is excused: ids, frames
and counts are compared exactly.  The last test of the module fails if an argmax form, a T' or the second round of the emotion
head's class loops was never run."""
import numpy as np
import pytest
import torch

from common import TOL_LOGP, report

import ctc_head_cases as K
from ctc_greedy_long_ref import collapse_ref

pytestmark = pytest.mark.gpu

TOL_EMO = 1e-5        # the bar of test_emotion_model_probs
TOL_LSE = 1e-5        # |logsumexp| of a log-prob row
TOL_SUM = 1e-6        # |sum - 1| of a probability row

_ENGINES = {}
_RAN = {"greedy": set(), "T": set(), "emo_nc": set(), "emo_T": set(), "logp": set()}     # what the coverage guard reads


def _make_engine(cfg, sd):
    from gigaam_amd.engine import HipEngine, build_config
    return HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), sd, torch.device("cuda:0"))


def _engine(head):
    if head not in _ENGINES:
        _ENGINES[head] = _make_engine(*K.head_state(head))
    return _ENGINES[head]


def _emo_engine(nc):
    if ("emo", nc) not in _ENGINES:
        _ENGINES[("emo", nc)] = _make_engine(*K.emo_state(nc))
    return _ENGINES[("emo", nc)]


def _greedy(head, encoded, enc_len):
    """ctc_greedy -> (ids [B, T'], frames [B, T'], counts [B]) as numpy.  The engine passes the lengths on as they are."""
    enc = torch.from_numpy(encoded).to("cuda:0")
    dec = _engine(head).ctc_greedy(enc, torch.tensor(enc_len, dtype=torch.int32))
    torch.cuda.synchronize()
    assert dec.ids.shape == dec.frames.shape == (encoded.shape[0], encoded.shape[2])
    _RAN["greedy"].add(K.head_v(head))
    _RAN["T"].add(encoded.shape[2])
    return [x.cpu().numpy() for x in dec[:3]]


def _assert_decoded(tag, got, want):
    ids, frames, counts = got
    assert counts.tolist() == [len(w[0]) for w in want], (tag, counts.tolist(), [len(w[0]) for w in want])
    for b, (wi, wf) in enumerate(want):
        assert ids[b, :len(wi)].tolist() == wi, (tag, b)
        assert frames[b, :len(wf)].tolist() == wf, (tag, b)


def _greedy_long(eng, lp):
    """op_ctc_greedy_long of one utterance's log-probs (device tensor [T, V]) -> (ids, frames)."""
    from gigaam_amd.engine import HipEngine
    rows, flag = HipEngine.collect(eng.op_ctc_greedy_long(lp))
    assert not flag and len(rows) == 1
    return rows[0]


@pytest.mark.parametrize("T", K.T_GRID)
@pytest.mark.parametrize("head", K.HEADS)
def test_length_grid_and_cross_check(head, T):
    """ctc_greedy is exactly the reference's; and three decodes agree: ctc_greedy, the collapsed first-maximum argmax of the device's
    own ctc_head output cut at enc_len, and op_ctc_greedy_long on that output per utterance.  (The tie heads take part: the tied
    logits of a frame are equal bit for bit, and the log-softmax maps equal inputs of one row to equal outputs.)"""
    eng = _engine(head)
    V = K.head_v(head)
    for which in K.GRID_BATCHES:
        case = K.grid_case(head, T, which)
        _, _, want = K.expected(case)
        got = _greedy(head, case["encoded"], case["enc_len"])
        _assert_decoded((head, case["name"]), got, want)
        lp = eng.ctc_head(torch.from_numpy(case["encoded"]).to("cuda:0"))
        assert lp.shape == (4, T, V)
        am = lp.cpu().numpy().argmax(axis=2)
        for b, n in enumerate(case["enc_len"]):
            n = K.clamp_len(n, T)
            assert collapse_ref(am[b, :n], V - 1) == want[b], (head, case["name"], b, "argmax of ctc_head")
            assert _greedy_long(eng, lp[b, :n]) == want[b], (head, case["name"], b, "op_ctc_greedy_long")


@pytest.mark.parametrize("head", K.HEADS)
def test_pass_borders_and_extremes(head):
    """Runs and repeats over the borders of the 512-frame compaction passes; all blank, one label, and a full result buffer."""
    for case in (K.border_case(head), K.extreme_case(head)):
        _, _, want = K.expected(case)
        got = _greedy(head, case["encoded"], case["enc_len"])
        _assert_decoded((head, case["name"]), got, want)


@pytest.mark.parametrize("V", K.TAP_V)
def test_exact_ties_take_the_first_maximum(V):
    head = f"tap{V}"
    case = K.tie_case(head)
    want = K.decode_ref(case["want"], case["enc_len"], V - 1)
    ids, frames, counts = got = _greedy(head, case["encoded"], case["enc_len"])
    for b in range(2):           # name the row that went wrong before the whole decode is compared
        n = int(counts[b])
        for f, i in zip(frames[b, :n].tolist(), ids[b, :n].tolist()):
            assert 0 <= f < case["want"].shape[1] and i == case["want"][b, f], (V, b, f, case["names"][b][f], i)
    _assert_decoded((head, "ties"), got, want)


@pytest.mark.parametrize("head", ["tie", "tie_hi"])
def test_duplicated_weight_rows_tie_bit_for_bit(head):
    """What the tie heads rest on: the logits of a pair are equal on the device (the log-probs are, elementwise of the logits)."""
    case = K.border_case(head)
    lp = _engine(head).ctc_head(torch.from_numpy(case["encoded"][:2]).to("cuda:0")).cpu().numpy()
    for lo, hi in K.TIE_PAIRS[head]:
        assert np.array_equal(lp[:, :, lo], lp[:, :, hi]), (head, lo, hi)


def test_length_limit():
    """The largest T' the launcher accepts (a 60 KiB dynamic-LDS launch, 30 passes) decodes; one frame more is refused."""
    from gigaam_amd._lib import GigaAMHipError
    assert K.T_LIMIT == 15344
    case = K.limit_case()
    _, _, want = K.expected(case)
    _assert_decoded("limit", _greedy("tap34", case["encoded"], case["enc_len"]), want)
    longer = np.concatenate([case["encoded"], case["encoded"][:, :, :1]], axis=2)
    assert longer.shape == (1, K.D_MODEL, K.T_LIMIT + 1)
    with pytest.raises(GigaAMHipError, match="too long"):
        _engine("tap34").ctc_greedy(torch.from_numpy(longer), torch.tensor([K.T_LIMIT + 1], dtype=torch.int32))
    _assert_decoded("limit, again", _greedy("tap34", case["encoded"], case["enc_len"]), want)      # the engine is still good


@pytest.mark.parametrize("head", K.HEADS)
def test_ctc_head_log_probs(head):
    eng = _engine(head)
    V = K.head_v(head)
    for shape in K.LOGP_SHAPES:
        enc, kind_of = K.logp_case(head, shape)
        lp = eng.ctc_head(torch.from_numpy(enc)).cpu().numpy().astype(np.float64)
        assert lp.shape == (shape[0], shape[1], V) and np.isfinite(lp).all()
        lg = K.logits64(head, enc)
        if K.is_tap(head):       # the tap is exact: the device's log-probs differ from its logits by one constant per row
            d = lg - lp
            assert np.abs(d - d[:, :, :1]).max() < TOL_LOGP
        err = np.abs(lp - K.log_softmax64(lg)).max(axis=2)
        lse = np.abs(K.logsumexp64(lp))
        for kind in K.logp_kinds(head):
            m = kind_of == kind
            e, s = float(err[m].max()), float(lse[m].max())
            print(f"ctc_head {head} {shape} {kind}: max log-prob error {e:.3e}, max |logsumexp| {s:.3e}")
            report("ctc_head_matrix", what="ctc_head", head=head, B=shape[0], T=shape[1], kind=kind, logp_err=e, lse_err=s)
            assert e < TOL_LOGP, (head, shape, kind, e)
            assert s < TOL_LSE, (head, shape, kind, s)
        _RAN["logp"].add(head)


@pytest.mark.parametrize("nc", K.EMO_NC)
def test_emo_probs(nc):
    eng = _emo_engine(nc)
    for T in K.EMO_T:
        for with_lens in (True, False):
            enc, lens = K.emo_case(nc, T, with_lens)
            got = eng.emo_probs(torch.from_numpy(enc), None if lens is None else torch.tensor(lens, dtype=torch.int32))
            got = got.cpu().numpy().astype(np.float64)
            want = K.emo_ref(nc, enc, lens)
            assert got.shape == want.shape == (enc.shape[0], nc)
            e, s = float(np.abs(got - want).max()), float(np.abs(got.sum(axis=1) - 1.0).max())
            print(f"emo_probs NC={nc} T'={T} lengths={'yes' if with_lens else 'none'}: max error {e:.3e}, max |sum - 1| {s:.3e}")
            report("ctc_head_matrix", what="emo_probs", NC=nc, T=T, lengths=bool(with_lens), prob_err=e, sum_err=s)
            assert e < TOL_EMO, (nc, T, with_lens, e)
            assert s < TOL_SUM, (nc, T, with_lens, s)
        _RAN["emo_nc"].add(nc)
        _RAN["emo_T"].add(T)


def _assert_sane(tag, ids, frames, V, n_max):
    assert len(ids) == len(frames) <= n_max, tag
    assert all(0 <= i < V - 1 for i in ids), (tag, [i for i in ids if not 0 <= i < V - 1][:4])
    assert all(0 <= f < n_max for f in frames) and all(a < b for a, b in zip(frames, frames[1:])), tag


@pytest.mark.parametrize("V", [34, 257])
def test_non_finite_rows(V):
    """All-NaN frames and frames with a single NaN through the two CTC greedy decoders, and through them only.  Every emitted id lies
    in [0, V - 1), frames ascend strictly, counts <= len; a frame with no comparable value decodes as class 0 in both argmax forms
    (what torch.argmax gives for it).  Through the head, ONE NaN in a frame of ``encoded`` makes every logit of the frame NaN."""
    head = f"tap{V}"
    eng = _engine(head)
    x, all_nan, one_nan = K.nonfinite_logits(V)
    T = x.shape[0]
    clean = np.where(np.isnan(x), np.float32(-9.0), x)
    lab = clean.argmax(axis=1)                       # the single NaN sits on the class that would have won: another class wins
    # ctc_greedy: utterance 0 has the NaN rows as they are; utterance 1 has one NaN per frame in a channel the tap does not read
    rng = np.random.default_rng(V)
    enc = (3.0 * rng.standard_normal((2, K.D_MODEL, T))).astype(np.float32)
    enc[0, :V, :] = x.T
    enc[1, :V, :] = clean.T
    enc[1, 700, all_nan | one_nan] = np.nan
    want0 = np.where(all_nan, 0, lab)
    want1 = np.where(all_nan | one_nan, 0, lab)
    for n in (T, K.NT + 1):
        ids, frames, counts = _greedy(head, enc, [n, n])
        for b in range(2):
            _assert_sane(("ctc_greedy", V, b), ids[b, :counts[b]].tolist(), frames[b, :counts[b]].tolist(), V, n)
        assert (ids[1, :counts[1]].tolist(), frames[1, :counts[1]].tolist()) == collapse_ref(want1[:n], V - 1)
        got0 = dict(zip(frames[0, :counts[0]].tolist(), ids[0, :counts[0]].tolist()))
        w_ids, w_frames = collapse_ref(want0[:n], V - 1)      # utterance 0 but its single-NaN frames and the frames behind them
        loose = one_nan[:n] | np.concatenate([[False], one_nan[:n - 1]])
        for f, i in zip(w_frames, w_ids):
            if not loose[f]:
                assert got0.get(f) == i, (V, f, i, got0.get(f))
    # op_ctc_greedy_long reads its rows as they are: all-NaN rows decode as class 0; a single NaN leaves a row with a maximum
    only_all = np.where(one_nan[:, None], clean, x)
    assert _greedy_long(eng, torch.from_numpy(only_all)) == collapse_ref(want0, V - 1)
    ids, frames = _greedy_long(eng, torch.from_numpy(x))
    _assert_sane(("op_ctc_greedy_long", V), ids, frames, V, T)


def test_every_form_and_size_was_run():
    """Runs last.  Both argmax forms at both ends of their V range, every T' of the grid, the pass-border and limit sizes, every
    head's log-probs, the emotion head's class loops more than once round: a changed case list that loses one of these fails here."""
    ran = _RAN["greedy"]
    assert ran, "the matrix did not run before this test"
    assert {2, 64} <= {v for v in ran if K.thread_form(v)}, sorted(ran)
    wave = {v for v in ran if not K.thread_form(v)}
    assert any(v <= 64 and v % 2 == 1 for v in wave) and any(64 < v <= K.D_MODEL for v in wave) and any(v > 1024 for v in wave), sorted(ran)
    assert set(K.T_GRID) | {K.T_BORDER, K.T_LIMIT} <= _RAN["T"], sorted(_RAN["T"])
    assert _RAN["logp"] == set(K.HEADS)
    assert any(nc > 64 for nc in _RAN["emo_nc"]) and any(nc > 128 for nc in _RAN["emo_nc"]) and 1 in _RAN["emo_nc"], _RAN["emo_nc"]
    assert _RAN["emo_T"] == set(K.EMO_T)
