"""GPU: CTC forced alignment of one long utterance with wildcard tokens (gam_op_ctc_align_long_star, the STAR variants of
gigaam_amd/csrc/gam_align_long.h) against the float64 reference of tests/ctc_align_star_ref.py: wildcards at the block edges of the
tiling and at the end of the target, the infeasible call, exact paths against the reference and the one-workgroup STAR kernel, and
bit equality with gam_op_ctc_align_long on a target without wildcards."""
import math

import numpy as np
import pytest
import torch

from common import report

import ctc_align_star_ref as RS
from test_hip_ctc_align import _log_probs, _op_engine, _target
from test_hip_ctc_align_long import _tiling
from test_hip_ctc_align_star import _check, _run_star

pytestmark = pytest.mark.gpu

LN2 = math.log(2)
T, U, V = 300, 200, 34
TILINGS = [(64, 7), (128, 16), (0, 0)]                 # (0, 0): planned


def _run_long_star(eng, lp, y, star):
    """gam_op_ctc_align_long_star on numpy log-probs [T, V] -> a host dict in the batch layout _check reads (B = 1)."""
    h = eng.op_ctc_align_long(torch.from_numpy(np.ascontiguousarray(lp, dtype=np.float32)), y,
                              star=torch.from_numpy(np.ascontiguousarray(star, dtype=np.float32))).host()
    return {"frame_labels": h["frame_labels"][None, :], "tok_first": h["tok_first"][None, :], "tok_last": h["tok_last"][None, :],
            "status": np.array([h["status"]]), "score": np.array([h["score"]]), "loglik": np.array([h["loglik"]]), "flag": h["flag"]}


def _targets(rng):
    """Wildcards where the tiling matters (sb = 64: block j holds states 64 j .. 64 j + 63, token u is state 2u + 1):
    A: u = 31 (state 63, a block's LAST state -- the one published as the block's edge), u = 100, and the very last token (the end
       rule reads S - 1, a wildcard, and S - 2);
    B: u = 32 (state 65, a block's FIRST token: fed by the neighbour's published edge through s - 1 and s - 2), and u = 0."""
    base = _target(rng, U, V, 6)
    a, b = list(base), list(base)
    for u in (31, 100, U - 1):
        a[u] = V
    for u in (0, 32):
        b[u] = V
    return {"A": a, "B": b}


@pytest.fixture(scope="module")
def cases():
    """Per kind: log-probs [T, V], the device's star row, the two targets and their float64 results -- built once, never written."""
    eng = _op_engine()
    out = {}
    for kind in ("peaked", "flat", "dyadic"):
        rng = np.random.default_rng(77 + len(kind))
        lp = _log_probs(rng, 1, T, V, kind)[0]
        if kind == "dyadic":
            star = rng.choice(np.array([0.0, -0.5, -1.0, -2.0], dtype=np.float32), size=T)
        else:
            star = eng.ctc_star_row(torch.from_numpy(lp), None, LN2).cpu().numpy()
        out[kind] = (lp, star, _targets(rng))
    return out


@pytest.mark.parametrize("sb,tt", TILINGS)
@pytest.mark.parametrize("kind", ["peaked", "flat"])
def test_long_star_matches_float64_reference(cases, kind, sb, tt):
    eng = _op_engine()
    lp, star, targets = cases[kind]
    errs = {}
    with _tiling(eng, sb, tt):
        for name, y in targets.items():
            h = _run_long_star(eng, lp, y, star)
            assert h["score"].dtype == np.float64
            _check(h, 0, lp, star, T, y, errs)
            assert int(h["status"][0]) == 1, name
    report(f"ctc_align_long_star_{kind}_sb{sb}_tt{tt}", **errs)


@pytest.mark.parametrize("sb,tt", TILINGS)
def test_long_star_exact_path_equals_reference_and_one_workgroup_kernel(cases, sb, tt):
    """Dyadic log-probs and star row: exact in fp32 and fp64, so the path is the reference's, and the one-workgroup STAR kernel's."""
    eng = _op_engine()
    lp, star, targets = cases["dyadic"]
    with _tiling(eng, sb, tt):
        for name, y in targets.items():
            h = _run_long_star(eng, lp, y, star)
            _check(h, 0, lp, star, T, y, {}, exact_path=True)
            short = _run_star(eng, lp[None], [T], [y], star[None])
            for k in ("frame_labels", "tok_first", "tok_last"):
                assert np.array_equal(h[k][0], short[k][0]), (name, k)
            assert int(short["status"][0]) == 1 and float(h["score"][0]) == float(short["score"][0])


@pytest.mark.parametrize("sb,tt", TILINGS)
def test_long_star_infeasible_call(cases, sb, tt):
    eng = _op_engine()
    lp, star, targets = cases["flat"]
    y = targets["A"]
    need = len(y) + sum(y[i] == y[i - 1] for i in range(1, len(y)))
    with _tiling(eng, sb, tt):
        for Tn in (need - 1, 150):                              # one frame short; fewer frames than tokens
            h = _run_long_star(eng, lp[:Tn], y, star[:Tn])
            _check(h, 0, lp[:Tn], star[:Tn], Tn, y, {})
            assert int(h["status"][0]) == 0
        h = _run_long_star(eng, lp[:need], y, star[:need])      # exactly minimal
        _check(h, 0, lp[:need], star[:need], need, y, {})
        assert int(h["status"][0]) == 1
        for bad in ([3, V - 1, 4], [3, V + 1, 4]):              # blank and ids past the wildcard stay bad ids
            assert int(_run_long_star(eng, lp, bad, star)["status"][0]) == 0
    # without a star row the wildcard id is a bad id, as before
    assert eng.op_ctc_align_long(torch.from_numpy(lp), [3, V, 4]).host()["status"] == 0


@pytest.mark.parametrize("sb,tt", TILINGS)
def test_long_star_without_wildcards_equals_long_op_bit_for_bit(cases, sb, tt):
    eng = _op_engine()
    lp, star, _ = cases["flat"]
    y = _target(np.random.default_rng(5), U, V, 6)
    with _tiling(eng, sb, tt):
        a = eng.op_ctc_align_long(torch.from_numpy(lp), y).host()
        b = eng.op_ctc_align_long(torch.from_numpy(lp), y, star=torch.from_numpy(star)).host()
    assert a["status"] == 1 and b["status"] == 1
    for k in ("frame_labels", "tok_first", "tok_last"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("score", "loglik"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k


def test_long_star_empty_call():
    eng = _op_engine()
    h = eng.op_ctc_align_long(torch.zeros((0, V)), [], star=torch.zeros((0,))).host()
    assert h["status"] == 1 and h["score"] == 0.0 and h["loglik"] == 0.0
    h = eng.op_ctc_align_long(torch.zeros((0, V)), [V], star=torch.zeros((0,))).host()
    assert h["status"] == 0 and h["score"] == -np.inf
