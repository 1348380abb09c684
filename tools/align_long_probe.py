"""Long-utterance CTC alignment at recording size: gam_op_ctc_align_long on a planted-path input of one hour of encoder frames
against a char-level transcript (T = 90 000, U = 50 000, V = 34 by default).  Checks that the returned path is a CTC path of the
target and that it rescores to the returned score (both O(T)), and prints the sweep / backtrack / outputs times from the
library's per-class event timing, plus the wall time of the whole call.  A tool, not a test: no threshold.

    python tools/align_long_probe.py [--frames T] [--tokens U] [--classes V] [--sb SB --tt TT] [--repeat N]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ctc_align_ref as R  # noqa: E402


def planted(rng, T, U, V):
    """Targets without adjacent repeats, a monotone state path that spreads the 2U + 1 states over the T frames (stay / +1 / +2 from a
    token state), and peaked log-probs (logit 9 on the path's label, N(0, 1) elsewhere)."""
    y = rng.integers(0, V - 1, U)
    same = np.flatnonzero(y[1:] == y[:-1]) + 1
    while same.size:                                        # re-draw until no adjacent repeats are left
        y[same] = rng.integers(0, V - 1, same.size)
        same = np.flatnonzero(y[1:] == y[:-1]) + 1
    S = 2 * U + 1
    path, s = np.empty(T, dtype=np.int64), int(rng.integers(0, 2))
    for t in range(T):
        path[t] = s
        left, need = T - 1 - t, S - 1 - s                   # frames left after this one, states still to climb (ending in S - 1)
        if left == 0:
            break
        # the most a path climbs in f more moves from state q: 2f from a token state, 2f - 1 from a blank
        moves = [m for m in ((0, 1, 2) if s & 1 else (0, 1))
                 if 0 <= need - m <= (0 if left == 1 else 2 * (left - 1) - (0 if (s + m) & 1 else 1))]
        # lean on the move that keeps the path on the diagonal
        want = need / left
        p = np.array([np.exp(-abs(m - want)) for m in moves])
        s += int(rng.choice(moves, p=p / p.sum()))
    assert path[-1] == S - 1, (path[-1], S - 1)
    labels = np.where(path & 1, y[np.maximum(path - 1, 0) >> 1], V - 1)
    x = rng.standard_normal((T, V)).astype(np.float32)
    x[np.arange(T), labels] = 9.0
    return y.tolist(), labels, torch.log_softmax(torch.from_numpy(x), dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=90000)
    ap.add_argument("--tokens", type=int, default=50000)
    ap.add_argument("--classes", type=int, default=34)
    ap.add_argument("--sb", type=int, default=0)
    ap.add_argument("--tt", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    from gigaam_amd import synth
    from gigaam_amd.engine import HipEngine, build_config
    cfg = synth.model_cfg("v2_ctc")
    eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], None), {}, torch.device("cuda:0"))
    T, U, V = args.frames, args.tokens, args.classes
    y, labels, lp = planted(np.random.default_rng(0), T, U, V)
    lp_d, y_d = lp.cuda(), torch.tensor(y, dtype=torch.int32).cuda()
    eng.tune_ctc_align_long(args.sb, args.tt)
    out = eng.op_ctc_align_long(lp_d, y_d).host()          # sizes the workspace; the result is checked below
    assert out["status"] == 1
    states = R.path_states(out["frame_labels"].tolist(), y, V - 1)
    assert states is not None, "the returned labels are not a CTC path of the target"
    rescore = float(lp.double()[torch.arange(T), torch.from_numpy(out["frame_labels"].astype(np.int64))].sum())
    planted_score = float(lp.double()[torch.arange(T), torch.from_numpy(labels)].sum())
    first, last = R.token_runs(states, U)
    assert out["tok_first"].tolist() == first and out["tok_last"].tolist() == last
    bar = 1e-3 * max(1.0, abs(rescore))
    assert abs(rescore - out["score"]) <= bar, (rescore, out["score"])
    assert abs(planted_score - out["score"]) <= bar, (planted_score, out["score"])
    assert out["loglik"] >= out["score"] - bar
    best = None
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        eng.profile_enable(1)
        t0 = time.perf_counter()
        eng.op_ctc_align_long(lp_d, y_d)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        prof = eng.profile_read()
        eng.profile_enable(0)
        run = {"wall_ms": wall, "sweep_ms": prof["decode"]["ms"], "backtrack_ms": prof["align_bt"]["ms"], "outputs_ms": prof["align_out"]["ms"]}
        if best is None or run["wall_ms"] < best["wall_ms"]:
            best = run
    S = 2 * U + 1
    print(json.dumps({"probe": "align_long", "T": T, "U": U, "V": V, "sb": args.sb or "default", "tt": args.tt or "default",
                      "score": out["score"], "rescore": rescore, "planted_score": planted_score, "loglik": out["loglik"],
                      "path_equals_planted": bool((out["frame_labels"] == labels).all()),
                      "backpointer_bytes": T * ((S + 63) // 64) * 16, "repeat": args.repeat,
                      **{k: round(v, 3) for k, v in best.items()}}))
    eng.tune_ctc_align_long(0, 0)


if __name__ == "__main__":
    main()
