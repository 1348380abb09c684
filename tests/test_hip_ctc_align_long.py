"""GPU: CTC forced alignment of one long utterance (gam_op_ctc_align_long, gigaam_amd/csrc/gam_align_long.h) against the float64
reference of tests/ctc_align_ref.py: planted paths steered across the block and tile edges, equality with the one-workgroup kernel
inside its limits, exact ties, the edge cases, determinism and the limits."""
import contextlib

import numpy as np
import pytest
import torch

from common import report

import ctc_align_ref as R
from test_hip_ctc_align import _bar, _check_utterance, _log_probs, _op_engine, _run_op, _target

pytestmark = pytest.mark.gpu

SB_DEFAULT, TT_DEFAULT = 1024, 256      # gam_align_long.h: GAM_AL_SB_DEFAULT, GAM_AL_TT_DEFAULT

# The long op's |error| against float64 may be MARGIN times the one-workgroup kernel's on the same input (the largest over the
# utterances of a case, score and loglik each), plus MARGIN_FLOOR.  Both kernels make the same per-step fp32 roundings of
# O(one frame's log-prob) numbers; the long op adds one more of that size per block edge and frame (the fp64 -> fp32 conversion
# of the neighbour's state) but returns float64 where the one-workgroup kernel rounds its result to fp32.  Measured on MI355X
# (DESIGN.md section 4.17): the long op's error is 0.02 .. 0.45 of the other's on the four cases, so the margin is 1 -- no larger.
MARGIN = 1.0
MARGIN_FLOOR = 2e-6                     # a few fp32 ulps of the O(10) running values: where the old kernel's error is ~0


@contextlib.contextmanager
def _tiling(eng, sb, tt):
    eng.tune_ctc_align_long(sb, tt)
    try:
        yield
    finally:
        eng.tune_ctc_align_long(0, 0)


def _run_long(eng, lp, y):
    """gam_op_ctc_align_long on numpy log-probs [T, V] -> a host dict in the batch layout _check_utterance reads (B = 1)."""
    h = eng.op_ctc_align_long(torch.from_numpy(np.ascontiguousarray(lp, dtype=np.float32)), y).host()
    return {"frame_labels": h["frame_labels"][None, :], "tok_first": h["tok_first"][None, :], "tok_last": h["tok_last"][None, :],
            "status": np.array([h["status"]]), "score": np.array([h["score"]]), "loglik": np.array([h["loglik"]]), "flag": h["flag"]}


# ---- planted paths
def _max_advance(s, frames):
    """The most states a path can climb in ``frames`` moves from state s (targets without adjacent repeats: +2 from every token)."""
    return 0 if frames <= 0 else (2 * frames if s & 1 else 2 * frames - 1)


def _walk(rng, t_a, s_a, t_b, s_b):
    """A random CTC state path from (t_a, s_a) to (t_b, s_b), both ends included: stay, +1, or +2 from a token state."""
    assert 0 <= s_b - s_a <= _max_advance(s_a, t_b - t_a), (t_a, s_a, t_b, s_b)
    out, s = [s_a], s_a
    for t in range(t_a + 1, t_b + 1):
        moves = [m for m in ((0, 1, 2) if s & 1 else (0, 1)) if 0 <= s_b - (s + m) <= _max_advance(s + m, t_b - t)]
        s += int(rng.choice(moves))
        out.append(s)
    assert s == s_b
    return out


def _planted_path(rng, T, U, sb, tt):
    """A state path over S = 2U + 1 states in T frames, steered so that block edge i (state b = i * sb) is crossed
    i odd:  by +1 (b-1 -> b) at a frame that OPENS a time tile, followed by a stay on b (the block's first state);
    i even: by +2 (b-1 -> b+1, from the last token state of the block) at a frame that CLOSES a time tile."""
    S = 2 * U + 1
    anchors = [(0, int(rng.integers(0, 2)))]
    for i, b in enumerate(range(sb, S - 2, sb), start=1):
        tc = int(round(b / S * T))
        if i & 1:
            tc -= tc % tt                                   # first frame of a tile
            anchors += [(tc - 1, b - 1), (tc, b), (tc + 1, b)]
        else:
            tc += tt - 1 - tc % tt                          # last frame of a tile
            anchors += [(tc - 1, b - 1), (tc, b + 1)]
    anchors.append((T - 1, S - 1 - int(rng.integers(0, 2))))
    path = [anchors[0][1]]
    for (t_a, s_a), (t_b, s_b) in zip(anchors, anchors[1:]):
        path += _walk(rng, t_a, s_a, t_b, s_b)[1:]
    assert len(path) == T
    return path


def _crossings(path, sb, tt):
    """What the path does at the block edges of a tiling: the set of moves seen there, and whether an edge is crossed at the first /
    at the last frame of a time tile."""
    seen = {"moves": set(), "tile_first": False, "tile_last": False}
    for t in range(1, len(path)):
        p, s = path[t - 1], path[t]
        if s // sb != p // sb:
            seen["moves"].add(s - p)
            assert p % sb == sb - 1, "a crossing leaves from the block's last state"
            seen["tile_first"] |= t % tt == 0
            seen["tile_last"] |= t % tt == tt - 1
        elif s == p and s >= sb and s % sb == 0:
            seen["moves"].add(0)                            # a stay on a block's first state: it beat the neighbour's edge
    return seen


def _planted_case(T, U, V, sb, tt, seed):
    rng = np.random.default_rng(seed)
    y = [int(rng.integers(0, V - 1))]
    while len(y) < U:
        v = int(rng.integers(0, V - 1))
        if v != y[-1]:
            y.append(v)
    path = _planted_path(rng, T, U, sb, tt)
    labels = R.state_labels(path, y, V - 1)
    x = rng.standard_normal((T, V)).astype(np.float32)
    x[np.arange(T), labels] = 9.0
    lp = torch.log_softmax(torch.from_numpy(x), dim=-1).numpy()
    return y, path, labels, lp


_PLANTED = {}


def _planted(T, U, V, sb, tt):
    """The planted case of a shape and its float64 reference, built once and shared (read-only) by the tilings that run it."""
    key = (T, U, V)
    if key not in _PLANTED:
        y, path, labels, lp = _planted_case(T, U, V, sb, tt, seed=T + 3 * U + V)
        seen = _crossings(path, sb, tt)
        # the structure the test is about, asserted before the GPU runs
        assert seen["moves"] == {0, 1, 2}, seen
        assert seen["tile_first"] and seen["tile_last"], seen
        score, states = R.viterbi(lp, y)
        assert states == path, "the planted path is not the float64 reference's optimum"
        _PLANTED[key] = (y, path, labels, lp, score, R.forward_loglik(lp, y))
    return _PLANTED[key]


def _check_planted(eng, name, T, U, V, steer, forced):
    y, path, labels, lp, score, ll = _planted(T, U, V, *steer)
    with _tiling(eng, *(forced or (0, 0))):
        h = eng.op_ctc_align_long(torch.from_numpy(lp), y).host()
    first, last = R.token_runs(path, U)
    e_s, e_l = abs(h["score"] - score), abs(h["loglik"] - ll)
    report(name, score=score, loglik=ll, score_err=e_s, loglik_err=e_l)
    print(name, "score", score, "err", e_s, "loglik", ll, "err", e_l)
    assert h["status"] == 1
    assert h["frame_labels"].tolist() == labels
    assert h["tok_first"].tolist() == first and h["tok_last"].tolist() == last
    assert e_s <= _bar(score), (h["score"], score)
    assert e_l <= _bar(ll), (h["loglik"], ll)


@pytest.mark.parametrize("sb,tt", [(128, 16), (64, 1), (192, 400)])
def test_planted_path_across_block_and_tile_edges(sb, tt):
    """T = 400, U = 150 (S = 301), V = 34: 3 blocks x 25 tiles, and the two degenerate tilings (one frame per tile; one tile) on the
    same path.  The path is steered for the 128 x 16 tiling."""
    _check_planted(_op_engine(), f"ctc_align_long_planted_T400_sb{sb}_tt{tt}", 400, 150, 34, (128, 16), (sb, tt))


@pytest.mark.parametrize("V", [34, 257])
def test_planted_path_beyond_the_one_workgroup_limits(V):
    """T = 9000 frames, U = 1500 tokens with the DEFAULT tiling (3 blocks x 36 tiles): beyond both limits of gam_op_ctc_align."""
    _check_planted(_op_engine(), f"ctc_align_long_planted_T9000_V{V}", 9000, 1500, V, (SB_DEFAULT, TT_DEFAULT), None)


# ---- inside the limits of the one-workgroup kernel: every check of its own test, and no larger an error
def _plan_case(V, Tp, kind):
    """The plan of test_op_align_matches_float64_reference -- (U, repeats, T), None = exactly minimal T -- as (lp, enc_len, targets)."""
    rng = np.random.default_rng(V * 7 + Tp + (1 if kind == "flat" else 0))
    plan = [(0, 0, Tp), (1, 0, Tp // 3), (12, 4, Tp), (40, 10, None), (Tp // 4, 3, Tp - 7), (Tp // 2, 0, Tp),
            (0, 0, 0), (30, 5, Tp // 2)]
    targets = [_target(rng, U, V, r) for U, r, _ in plan]
    enc_len = [T if T is not None else len(y) + sum(y[i] == y[i - 1] for i in range(1, len(y))) for (_, _, T), y in zip(plan, targets)]
    return _log_probs(rng, len(plan), Tp, V, kind), enc_len, targets


@pytest.mark.parametrize("V,Tp", [(34, 160), (257, 400)])
@pytest.mark.parametrize("kind", ["peaked", "flat"])
def test_long_op_matches_float64_reference_and_the_one_workgroup_kernel(V, Tp, kind):
    eng = _op_engine()
    lp, enc_len, targets = _plan_case(V, Tp, kind)
    old = _run_op(eng, lp, enc_len, targets)
    errs, worst = {}, {"long_score": 0.0, "long_loglik": 0.0, "old_score": 0.0, "old_loglik": 0.0}
    with _tiling(eng, 64, 16):
        for b, y in enumerate(targets):
            T = enc_len[b]
            h = _run_long(eng, lp[b][:T], y)
            _check_utterance(h, 0, lp[b][:T], T, y, errs)
            score, states = R.viterbi(lp[b], y, T)
            if states is None or T == 0:
                continue
            ll = R.forward_loglik(lp[b], y, T)
            for who, res, i in (("long", h, 0), ("old", old, b)):
                worst[f"{who}_score"] = max(worst[f"{who}_score"], abs(float(res["score"][i]) - score))
                worst[f"{who}_loglik"] = max(worst[f"{who}_loglik"], abs(float(res["loglik"][i]) - ll))
    report(f"ctc_align_long_vs_one_workgroup_V{V}_T{Tp}_{kind}", margin=MARGIN, floor=MARGIN_FLOOR, **worst, **errs)
    print(f"V{V} T{Tp} {kind}", worst)
    for k in ("score", "loglik"):
        assert worst[f"long_{k}"] <= MARGIN * worst[f"old_{k}"] + MARGIN_FLOOR, (k, worst)


@pytest.mark.parametrize("kind", ["peaked", "flat"])
def test_single_tile_long_op_is_the_one_workgroup_kernel(kind):
    """One block and one tile (sb = 192 >= the largest S = 161, tt = 400 >= T): no edge conversion happens, and the two kernels run
    the same frame step (gam_trellis.h) on the same numbers.  So paths and statuses are equal, the Viterbi score rounded to fp32 is
    the one-workgroup kernel's bit for bit, and loglik differs only by the final two-term log-sum-exp (float there, double here) on
    running values of O(10): within MARGIN_FLOOR plus one rounding of the total to fp32."""
    eng = _op_engine()
    lp, enc_len, targets = _plan_case(34, 160, kind)
    old = _run_op(eng, lp, enc_len, targets)
    worst = 0.0
    with _tiling(eng, 192, 400):
        for b, y in enumerate(targets):
            T, U = enc_len[b], len(y)
            h = _run_long(eng, lp[b][:T], y)
            assert int(h["status"][0]) == int(old["status"][b]), b
            assert np.array_equal(h["frame_labels"][0][:T], old["frame_labels"][b][:T]), b
            assert np.array_equal(h["tok_first"][0][:U], old["tok_first"][b][:U]), b
            assert np.array_equal(h["tok_last"][0][:U], old["tok_last"][b][:U]), b
            if int(old["status"][b]) != 1 or T == 0:
                continue
            assert np.float32(h["score"][0]).tobytes() == np.float32(old["score"][b]).tobytes(), (b, h["score"][0], old["score"][b])
            ll = np.float32(old["loglik"][b])
            d = abs(float(np.float32(h["loglik"][0])) - float(ll))
            worst = max(worst, d)
            assert d <= MARGIN_FLOOR + float(np.spacing(np.float32(abs(ll)))), (b, h["loglik"][0], ll)
    print(f"single tile {kind}: largest loglik difference {worst:.3g}")


def test_long_op_exact_ties_follow_the_tie_rule():
    """Dyadic log-probs: every sum is exact in fp32 and in fp64, through the edge conversion too, so the state path must be the
    reference's.  sb = 64, tt = 8: up to 4 blocks."""
    eng = _op_engine()
    rng = np.random.default_rng(21)
    with _tiling(eng, 64, 8):
        for V, Tp in ((4, 120), (34, 120)):
            plan = [(3, 1, 12), (40, 8, Tp), (0, 0, Tp // 2), (70, 20, Tp), (100, 0, Tp), (32, 0, 33)]
            targets = [_target(rng, U, V, r) for U, r, _ in plan]
            lp = _log_probs(rng, len(plan), Tp, V, "dyadic")
            errs = {}
            for b, ((_, _, T), y) in enumerate(zip(plan, targets)):
                _check_utterance(_run_long(eng, lp[b][:T], y), 0, lp[b][:T], T, y, errs, exact_path=True)


def test_long_op_edge_cases():
    eng = _op_engine()
    rng = np.random.default_rng(5)
    V, Tp = 34, 200
    lp = _log_probs(rng, 1, Tp, V, "peaked")[0]
    straddle = _target(rng, 80, V)
    straddle[32] = straddle[31]            # states 63 and 65: the forbidden skip lies across the edge of the blocks of 64
    straddle[64] = straddle[63]            # states 127 and 129
    reps = sum(straddle[i] == straddle[i - 1] for i in range(1, 80))
    cases = [
        ([], Tp, 1),                                   # U = 0: the all-blank path
        ([], 0, 1),                                    # T = 0 with U = 0 scores 0
        (straddle, 80 + reps, 1),                      # exactly minimal T
        (straddle, 80 + reps - 1, 0),                  # one frame short
        (straddle, Tp, 1),                             # repeated tokens straddling the block edges
        ([3, V - 1, 4], Tp, 0),                        # the blank id inside a target
        ([3, -3, 4], Tp, 0),                           # negative id
        (list(range(30)), 29, 0),                      # more tokens than frames
    ]
    with _tiling(eng, 64, 8):
        errs = {}
        for y, T, status in cases:
            h = _run_long(eng, lp[:T], y)
            assert int(h["status"][0]) == status, (len(y), T)
            _check_utterance(h, 0, lp[:T], T, y, errs)
        h = _run_long(eng, lp[:0], [])
        assert h["score"][0] == 0.0 and h["loglik"][0] == 0.0
    # and on the default tiling (one block, one tile)
    for y, T, status in cases:
        h = _run_long(eng, lp[:T], y)
        assert int(h["status"][0]) == status
        _check_utterance(h, 0, lp[:T], T, y, errs)


def test_long_op_is_bit_identical_on_another_stream_and_on_a_reused_handle():
    eng = _op_engine()
    rng = np.random.default_rng(9)
    V, T = 257, 300
    y = _target(rng, 140, V, 3)
    lp = torch.from_numpy(_log_probs(rng, 1, T, V, "flat")[0])
    with _tiling(eng, 64, 16):
        a = eng.op_ctc_align_long(lp, y).host()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            b = eng.op_ctc_align_long(lp, y).host()
        torch.cuda.synchronize()
        eng.op_ctc_align_long(lp[:100], y[:20]).host()      # another shape in between: the workspace is reused
        c = eng.op_ctc_align_long(lp, y).host()
    assert a["status"] == 1
    for other in (b, c):
        for k in ("frame_labels", "tok_first", "tok_last"):
            assert np.array_equal(a[k], other[k]), k
        for k in ("score", "loglik"):
            assert np.float64(a[k]).tobytes() == np.float64(other[k]).tobytes(), k


def test_long_op_limits():
    from gigaam_amd._lib import GigaAMHipError
    eng = _op_engine()
    rng = np.random.default_rng(3)
    V, T = 34, 120
    y = _target(rng, 40, V)
    lp = _log_probs(rng, 1, T, V, "peaked")[0]
    want = _run_long(eng, lp, y)
    eng.set_ctc_align_workspace(4096)
    try:
        with pytest.raises(GigaAMHipError, match="gam_set_ctc_align_workspace") as e:
            eng.op_ctc_align_long(torch.from_numpy(lp), y)
        assert "4096" in str(e.value)
    finally:
        eng.set_ctc_align_workspace(0)
    got = _run_long(eng, lp, y)                              # the handle stays usable
    assert np.array_equal(got["frame_labels"], want["frame_labels"]) and got["score"][0] == want["score"][0]
    for sb, tt in ((100, 0), (32, 0), (3136, 0), (-64, 0), (64, -1)):
        with pytest.raises(GigaAMHipError):
            eng.tune_ctc_align_long(sb, tt)
    eng.tune_ctc_align_long(3072, 1)
    eng.tune_ctc_align_long(0, 0)
    with pytest.raises(GigaAMHipError):
        eng.set_ctc_align_workspace(-1)
