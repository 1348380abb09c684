"""GPU: RNN-T confidence (gam_confidence.h gam_rnnt_conf_nodes_kernel behind the teacher-forced predictor and its pp GEMM), the joint
and the predictor entry points (gam_rnnt_joint, gam_rnnt_predict) on heads other than pred_hidden = joint_hidden = 320, against
float64 (tests/confidence_ref.py, tests/rnnt_beam_ref.py) -- the heads of tests/rnnt_cluster_cases.py, the inputs of
tests/rnnt_head_cases.py.  V = 34, 130, 257, 1025 give 3, 9, 17 and 65 class tiles, each with a partly filled last group of
GAM_CF_NV = 4; joint_hidden sets the k-loop and the LDS row pitch; pred_hidden = 48, 16 and 496 make the K of the pp GEMM no multiple
of the exact-fp32 kernel's 32-wide k-tile (its last tile is then zero-filled).  The alignment on the same heads is in
tests/test_hip_rnnt_align.py test_op_align_matches_float64_reference."""
import numpy as np
import pytest
import torch

import beam_common as BC
import confidence_ref as CF
import rnnt_beam_ref as R
import rnnt_head_cases as H
from common import TOL_LOGP, report

pytestmark = pytest.mark.gpu

MEASURES = ["prob", "entropy"]
POISON = 0x7fffff00     # in the padding of ids / frames: never read
TOL_STATE = 1e-4        # g, h, c of one predictor step: the bar of tests/test_hip_hardening.py test_rnnt_per_step_entry_points

_ENGINES = {}


def _engine(name, L):
    if (name, L) not in _ENGINES:
        from gigaam_amd.engine import HipEngine, build_config
        cfg, sd = H.conf_head(name, L)[:2]
        _ENGINES[(name, L)] = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), sd, torch.device("cuda:0"))
    return _ENGINES[(name, L)]


def _padded(rows):
    cap = max([len(r) for r in rows] + [0])
    t = torch.full((len(rows), cap), POISON, dtype=torch.int32)
    for i, r in enumerate(rows):
        if len(r):
            t[i, :len(r)] = torch.tensor(r, dtype=torch.int32)
    return t


def _tokens(rows):
    return _padded([r[0] for r in rows]), _padded([r[1] for r in rows]), torch.tensor([len(r[0]) for r in rows], dtype=torch.int32)


def _check(h, hd, encp64, lengths, rows, measure, want_status, what):
    """Status exactly, padding and invalid rows -1, every confidence of a valid row in [0, 1]; returns the largest error."""
    worst = 0.0
    assert h["status"].tolist() == want_status, (what, h["status"].tolist())
    for b, (ids, frames) in enumerate(rows):
        conf, ok = CF.rnnt_confidence(hd, encp64[b], lengths[b], ids, frames, measure)
        n = len(ids)
        assert ok == want_status[b], (what, b)
        assert (h["conf"][b, n:] == -1.0).all(), (what, b)
        got = h["conf"][b, :n].astype(np.float64)
        if not ok:
            assert (got == -1.0).all(), (what, b)
        elif n:
            assert ((got >= 0.0) & (got <= 1.0)).all(), (what, b)
            worst = max(worst, float(np.abs(got - np.asarray(conf)).max()))
    return worst


@pytest.mark.parametrize("name,L", H.CONF_SETS)
def test_confidence_matches_float64_reference(name, L):
    """The float64 greedy decode, a width-8 beam's rows and random valid paths with several tokens on one frame (0, 1, 16, 17 and 33
    tokens: none, one, a full 16-token workgroup, one more, two and one more), both measures; then the random rows with an
    out-of-range id in one and decreasing frames in another: status 0, conf -1, the other rows as before."""
    eng = _engine(name, L)
    _, _, hd, encp, lengths = H.conf_head(name, L)
    encp64 = [e.astype(np.float64) for e in encp]          # the reference reads what the device reads
    elen = torch.tensor(lengths, dtype=torch.int32)
    paths = H.conf_paths(name, L)
    eng.set_hotwords([])
    beam = BC.run_rnnt_op(eng, encp, lengths, 8, 3)["rows"]
    assert sum(len(r[0]) for r in beam) > 16
    errs = {}
    for which, rows in (("greedy", paths["greedy"]), ("beam", beam), ("random", paths["random"])):
        for measure in MEASURES:
            h = eng.op_rnnt_confidence(torch.from_numpy(encp), elen, *_tokens(rows), measure=measure).host()
            assert not h["flag"]
            e = _check(h, hd, encp64, lengths, rows, measure, [1] * len(lengths), (name, L, which, measure))
            errs[f"{which}_{measure}"] = e
    valid = {m: eng.op_rnnt_confidence(torch.from_numpy(encp), elen, *_tokens(paths["random"]), measure=m).host() for m in MEASURES}
    for measure in MEASURES:
        h = eng.op_rnnt_confidence(torch.from_numpy(encp), elen, *_tokens(paths["invalid"]), measure=measure).host()
        e = _check(h, hd, encp64, lengths, paths["invalid"], measure, H.INVALID_STATUS, (name, L, "invalid", measure))
        errs[f"invalid_{measure}"] = e
        for b, st in enumerate(H.INVALID_STATUS):
            if st:
                assert h["conf"][b].tobytes() == valid[measure]["conf"][b].tobytes(), (name, L, measure, b)      # untouched
    print(f"rnnt confidence head {name} L={L}: largest errors {errs} (bar {TOL_LOGP})")
    report(f"rnnt_head_confidence_{name}_L{L}", **errs)
    for k, e in errs.items():
        assert e <= TOL_LOGP, (name, L, k, e)


@pytest.mark.parametrize("name", H.JOINT_HEADS)
def test_joint_and_predict_match_float64_reference(name):
    """eng.rnnt_predict over four steps (the zero input, then three labels; B = 2) against R.Predictor's g, h and c, and
    eng.rnnt_joint on the [2, 5, 4] grid of those predictor outputs against R.joint_lp."""
    eng = _engine(name, 1)
    hd = H.conf_head(name, 1)[2]
    enc, labels = H.joint_inputs(name)
    pred = R.Predictor(hd)
    worst = 0.0
    gs = []
    g, st = eng.rnnt_predict(None, None, 2)
    for u in range(4):
        if u:
            g, st = eng.rnnt_predict(torch.tensor([labels[0][u - 1], labels[1][u - 1]], dtype=torch.int32), st)
        gs.append(g)
        for b in range(2):
            states = pred._get(tuple(labels[b][:u]))[1]
            worst = max(worst, float(np.abs(g[b].double().cpu().numpy() - states[-1][0]).max()))
            for l, (h_ref, c_ref) in enumerate(states):
                worst = max(worst, float(np.abs(st[0][l, b].double().cpu().numpy() - h_ref).max()),
                            float(np.abs(st[1][l, b].double().cpu().numpy() - c_ref).max()))
    lp = eng.rnnt_joint(torch.from_numpy(enc), torch.stack(gs, dim=1)).double().cpu().numpy()
    V = H.sizes(name)[0]
    assert lp.shape == (2, 5, 4, V)
    jw = 0.0
    for b in range(2):
        encp = enc[b].astype(np.float64) @ hd["enc_w"].T + hd["enc_b"]
        for t in range(5):
            for u in range(4):
                jw = max(jw, float(np.abs(lp[b, t, u] - R.joint_lp(hd, encp[t], pred(tuple(labels[b][:u])))).max()))
    print(f"rnnt per-step entry points head {name}: predictor error {worst:.3e} (bar {TOL_STATE}), joint error {jw:.3e} (bar {TOL_LOGP})")
    report(f"rnnt_head_joint_predict_{name}", predictor_err=worst, joint_err=jw)
    assert worst <= TOL_STATE and jw <= TOL_LOGP, (name, worst, jw)
