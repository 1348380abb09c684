"""GPU: CTC forced alignment with wildcard tokens at op level (gam_op_ctc_align_star / gam_op_ctc_star_row, the STAR variants of
gigaam_amd/csrc/gam_align.h) against the float64 reference of tests/ctc_align_star_ref.py, by the checking scheme of
test_hip_ctc_align.py: status, score and log-likelihood, the returned labels are a CTC path of the target, rescoring them gives
the score, and tok_first / tok_last are that path's runs."""
import math

import numpy as np
import pytest
import torch

from common import report

import ctc_align_star_ref as RS
import test_hip_ctc_align as A

pytestmark = pytest.mark.gpu

LN2 = math.log(2)


def _run_star(eng, lp, enc_len, targets, star, pad=None):
    """gam_op_ctc_align_star on numpy inputs -> host dict.  ``pad``: value written into targets past target_len."""
    B = lp.shape[0]
    um = max([len(t) for t in targets] + [0])
    tgt = torch.full((B, um), 0 if pad is None else pad, dtype=torch.int32)
    for i, t in enumerate(targets):
        tgt[i, : len(t)] = torch.tensor(t, dtype=torch.int32)
    tl = torch.tensor([len(t) for t in targets], dtype=torch.int32)
    star = star if isinstance(star, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(star))
    return eng.op_ctc_align(torch.from_numpy(np.ascontiguousarray(lp)), torch.tensor(enc_len, dtype=torch.int32), tgt, tl, star=star).host()


def _check(h, b, lp, star, T, y, errs, exact_path=False):
    """Utterance b of a result against the float64 reference (lp [T', V], star [T'])."""
    V = lp.shape[1]
    U = len(y)
    score, states = RS.viterbi(lp, star, y, T)
    ok = states is not None
    assert int(h["status"][b]) == int(ok), (b, T, U)
    if not ok:
        assert h["score"][b] == -np.inf and h["loglik"][b] == -np.inf
        assert (h["frame_labels"][b] == -1).all()
        assert (h["tok_first"][b] == -1).all() and (h["tok_last"][b] == -1).all()
        return
    ll = RS.forward_loglik(lp, star, y, T)
    e_s, e_l = abs(float(h["score"][b]) - score), abs(float(h["loglik"][b]) - ll)
    errs["score"] = max(errs.get("score", 0.0), e_s / max(1.0, abs(score)))
    errs["loglik"] = max(errs.get("loglik", 0.0), e_l / max(1.0, abs(ll)))
    assert e_s <= A._bar(score), (b, float(h["score"][b]), score)
    assert e_l <= A._bar(ll), (b, float(h["loglik"][b]), ll)
    labels = h["frame_labels"][b]
    assert (labels[T:] == -1).all()
    got = RS.path_states(labels[:T].tolist(), y, V)
    assert got is not None, (b, "not a CTC path of the target")
    first, last = RS.token_runs(got, U)
    assert h["tok_first"][b, :U].tolist() == first and h["tok_last"][b, :U].tolist() == last
    assert (h["tok_first"][b, U:] == -1).all() and (h["tok_last"][b, U:] == -1).all()
    for u, v in enumerate(y):                                  # wildcard frames come out as label V
        if v == V and T > 0:
            assert (labels[first[u]: last[u] + 1] == V).all()
    e_r = abs(RS.rescore(lp, star, labels[:T]) - score)
    errs["rescore"] = max(errs.get("rescore", 0.0), e_r / max(1.0, abs(score)))
    assert e_r <= A._bar(score), (b, "returned path is not optimal", e_r)
    if exact_path:
        assert got == states, (b, "tie rule")


def _main_plan(rng, V, Tp):
    """(targets, enc_len) of the main matrix: where a wildcard can stand, and the feasibility edge."""
    W = V
    t = lambda U, r=0: A._target(rng, U, V, r)
    a = int(rng.integers(0, V - 1))
    targets = [
        [W] + t(10, 2),                          # wildcard first
        t(10, 2) + [W],                          # wildcard last
        [W] + t(14, 3) + [W],                    # both ends
        t(6) + [W] + t(7, 1),                    # one in the middle
        t(4) + [W] + t(5, 1) + [W] + t(3),       # two, tokens between them
        t(3) + [a, W, a] + t(3),                 # between two equal tokens
        [W],                                     # alone
        t(2) + [W, W] + t(2),                    # two adjacent wildcards: a repeat
        [W] + t(12, 3) + [W, W] + t(5) + [W],    # T exactly minimal
        [W] + t(12, 3) + [W, W] + t(5) + [W],    # T one short of minimal
        [],                                      # U = 0 with T = 0
    ]
    need = lambda y: len(y) + sum(y[i] == y[i - 1] for i in range(1, len(y)))
    enc_len = [Tp, Tp - 3, Tp, Tp // 2, Tp, 40, Tp, 30, need(targets[8]), need(targets[9]) - 1, 0]
    return targets, enc_len


@pytest.fixture(scope="module")
def main_cases():
    """Per (V, kind): seeded log-probs, the targets of _main_plan and the device's own star row -- computed once, never written."""
    eng = A._op_engine()
    out = {}
    for V in (34, 257):
        for kind in ("peaked", "flat"):
            rng = np.random.default_rng(V * 5 + (1 if kind == "flat" else 0))
            Tp = 160
            targets, enc_len = _main_plan(rng, V, Tp)
            lp = A._log_probs(rng, len(targets), Tp, V, kind)
            star = eng.ctc_star_row(torch.from_numpy(lp), torch.tensor(enc_len, dtype=torch.int32), LN2).cpu().numpy()
            out[(V, kind)] = (lp, targets, enc_len, star)
    return out


@pytest.mark.parametrize("kind", ["peaked", "flat"])
@pytest.mark.parametrize("V", [34, 257])
def test_op_align_star_matches_float64_reference(main_cases, V, kind):
    eng = A._op_engine()
    lp, targets, enc_len, star = main_cases[(V, kind)]
    h = _run_star(eng, lp, enc_len, targets, star, pad=-12345)
    errs = {}
    for b, y in enumerate(targets):
        _check(h, b, lp[b], star[b], enc_len[b], y, errs)
    assert h["status"].tolist() == [1] * 9 + [0, 1]
    assert h["score"][10] == 0.0 and h["loglik"][10] == 0.0
    report(f"ctc_align_star_op_V{V}_{kind}", **errs)


@pytest.mark.parametrize("kind", ["peaked", "flat"])
@pytest.mark.parametrize("V", [34, 257])
def test_op_align_star_with_a_row_of_zeros(main_cases, V, kind):
    """star = 0, torchaudio's convention: the wildcard beats every label on every frame."""
    eng = A._op_engine()
    lp, targets, enc_len, _ = main_cases[(V, kind)]
    star = np.zeros(lp.shape[:2], dtype=np.float32)
    h = _run_star(eng, lp, enc_len, targets, star)
    errs = {}
    for b, y in enumerate(targets):
        _check(h, b, lp[b], star[b], enc_len[b], y, errs)
    report(f"ctc_align_star_op_zero_row_V{V}_{kind}", **errs)


def test_op_align_star_exact_ties_follow_the_tie_rule():
    """Dyadic log-probs and a dyadic star row are exact in fp32 and fp64 alike: the path must be the reference's."""
    eng = A._op_engine()
    rng = np.random.default_rng(33)
    for V, Tp in ((4, 40), (34, 120)):
        W = V
        t = lambda U, r=0: A._target(rng, U, V, r)
        targets = [[W] + t(3, 1), t(4, 1) + [W] + t(4, 1), [W, W], [W] + t(7, 2) + [W, W] + t(6) + [W], t(2) + [W], [W], []]
        enc_len = [12, Tp, 3, 40, Tp, Tp // 2, Tp]
        lp = A._log_probs(rng, len(targets), Tp, V, "dyadic")
        star = rng.choice(np.array([0.0, -0.5, -1.0, -2.0], dtype=np.float32), size=(len(targets), Tp))
        h = _run_star(eng, lp, enc_len, targets, star)
        errs = {}
        for b, y in enumerate(targets):
            _check(h, b, lp[b], star[b], enc_len[b], y, errs, exact_path=True)


def _sprinkle(rng, y, V, n):
    y = list(y)
    for u in rng.choice(len(y), size=n, replace=False):
        y[u] = V
    return y


@pytest.mark.parametrize("U,Tp,T,what", [(600, 1100, 900, "spt2_global_bp"), (1024, 1100, 1100, "spt3_global_bp"),
                                         (500, 1100, 700, "spt1_global_bp"), (600, 300, 300, "spt2_lds_bp")])
def test_op_align_star_kernel_variants(U, Tp, T, what):
    """The states-per-thread and backpointer variants of the STAR kernel (S = 2 Umax + 1 picks SPT, T' x S the backpointers' home),
    wildcards sprinkled in.  U = 600 in 300 frames is infeasible as it stands: there the second utterance (U = 250) is the one that
    aligns."""
    eng = A._op_engine()
    rng = np.random.default_rng(U + Tp)
    V = 1025
    big = _sprinkle(rng, A._target(rng, U, V, 5), V, 40)
    small = _sprinkle(rng, A._target(rng, 250, V, 5), V, 15)
    targets, enc_len = [big, small], [T, min(T, 280)]
    lp = A._log_probs(rng, 2, Tp, V, "flat")
    star = eng.ctc_star_row(torch.from_numpy(lp), torch.tensor(enc_len, dtype=torch.int32), LN2).cpu().numpy()
    h = _run_star(eng, lp, enc_len, targets, star, pad=V + 77)
    errs = {}
    for b, y in enumerate(targets):
        _check(h, b, lp[b], star[b], enc_len[b], y, errs)
    assert h["status"].tolist() == [int(RS.feasible(T, big, V)), 1] and (T < U or h["status"][0] == 1)
    report(f"ctc_align_star_op_{what}", **errs)


def test_op_align_star_without_wildcards_equals_op_align_bit_for_bit():
    eng = A._op_engine()
    rng = np.random.default_rng(9)
    V, Tp = 257, 300
    targets = [A._target(rng, U, V, 3) for U in (20, 100, 140, 0)] + [[3, V - 1, 4], list(range(40))]
    enc_len = [Tp, 250, Tp, 17, Tp, 39]
    lp = A._log_probs(rng, len(targets), Tp, V, "flat")
    star = eng.ctc_star_row(torch.from_numpy(lp), torch.tensor(enc_len, dtype=torch.int32), LN2)
    a = A._run_op(eng, lp, enc_len, targets)
    b = _run_star(eng, lp, enc_len, targets, star)
    assert a["status"].tolist() == [1, 1, 1, 1, 0, 0]
    for k in ("frame_labels", "tok_first", "tok_last", "status"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("score", "loglik"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_star_row_is_rowmax_minus_penalty_exactly():
    eng = A._op_engine()
    rng = np.random.default_rng(4)
    for V, Tp, enc_len in ((34, 70, [70, 0, 33]), (257, 129, [1, 129, 64]), (1025, 50, [50, 49, 7])):
        lp = torch.from_numpy(A._log_probs(rng, 3, Tp, V, "flat"))
        for penalty in (LN2, 0.0, 0.05):
            got = eng.ctc_star_row(lp, torch.tensor(enc_len, dtype=torch.int32), penalty).cpu()
            want = lp.max(-1).values - torch.tensor(penalty, dtype=torch.float32)
            valid = torch.arange(Tp)[None, :] < torch.tensor(enc_len)[:, None]
            assert got.dtype == torch.float32 and torch.equal(got[valid], want[valid])
            assert (got[~valid] == 0).all()
        # one long utterance [T, V]: every row is valid
        got = eng.ctc_star_row(lp[0], None, LN2).cpu()
        assert torch.equal(got, lp[0].max(-1).values - torch.tensor(LN2, dtype=torch.float32))


def test_star_row_rejects_a_bad_penalty():
    from gigaam_amd._lib import GigaAMHipError
    eng = A._op_engine()
    lp = torch.zeros((1, 10, 5))
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(GigaAMHipError, match="penalty"):
            eng.ctc_star_row(lp, torch.tensor([10], dtype=torch.int32), bad)


def test_wildcard_id_stays_a_bad_id_without_star():
    eng = A._op_engine()
    rng = np.random.default_rng(6)
    V, Tp = 34, 60
    lp = A._log_probs(rng, 2, Tp, V, "peaked")
    h = A._run_op(eng, lp, [Tp, Tp], [[3, V, 4], [3, 5, 4]])
    assert h["status"].tolist() == [0, 1]
    assert h["score"][0] == -np.inf and (h["frame_labels"][0] == -1).all()
    # and with a star row: blank and ids past V are still bad ids
    star = np.zeros((2, Tp), dtype=np.float32)
    h = _run_star(eng, lp, [Tp, Tp], [[3, V - 1, 4], [3, V + 1, 4]], star)
    assert h["status"].tolist() == [0, 0]
