"""Float64 reference of transducer forced alignment (gigaam_amd/csrc/gam_rnnt_align.h holds the contract), built on the float64
predictor and joint of tests/rnnt_beam_ref.py.  Used by the CPU and the GPU tests.

The standard transducer lattice, the one the RNN-T loss sums over: nodes (t, u), 0 <= t < T, 0 <= u <= U, blank = V - 1.
  lb[t, u] = log P(blank | frame t, y[:u])        -> (t + 1, u)
  le[t, u] = log P(y[u] | frame t, y[:u]), u < U  -> (t, u + 1)
  log_likelihood = alpha[T-1, U] + lb[T-1, U] with the log-sum-exp recursion; score = the same with max (Viterbi);
  tok_frame[u] = the frame at which y[u] is emitted on the best path.
max_symbols_per_step does not bound the lattice.  Tie rule: the blank predecessor (t-1, u) wins over the emission predecessor
(t, u-1).  T = 0: feasible only with U = 0 (both scores 0)."""
import itertools
from typing import List, Optional, Sequence, Tuple

import numpy as np

import rnnt_beam_ref as R

NEG = -np.inf


def lattice(head, encp, y: Sequence[int], T: Optional[int] = None) -> np.ndarray:
    """[T, U + 1, 2] float64: (lb, le) of every node; le at u = U is -inf.  encp [>= T, JH] (W_enc f + b_enc)."""
    encp = np.asarray(encp, dtype=np.float64)
    T = encp.shape[0] if T is None else T
    y = tuple(int(v) for v in y)
    U = len(y)
    pred = R.Predictor(head)
    pps = np.stack([pred(y[:u]) for u in range(U + 1)])
    lat = np.full((T, U + 1, 2), NEG)
    for t in range(T):      # (R.joint_lp's arithmetic, a frame's U + 1 rows at a time)
        z = np.maximum(encp[t][None, :] + pps, 0.0) @ head["out_w"].T + head["out_b"]
        m = z.max(axis=1, keepdims=True)
        lp = z - (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))
        lat[t, :, 0] = lp[:, -1]
        if U:
            lat[t, :U, 1] = lp[np.arange(U), list(y)]
    return lat


def lattice_from_joint(joint, y: Sequence[int], T: int) -> np.ndarray:
    """The same from ``joint(t, prefix) -> lp`` (rnnt_beam_ref's convention)."""
    y = tuple(int(v) for v in y)
    U = len(y)
    lat = np.full((T, U + 1, 2), NEG)
    for t in range(T):
        for u in range(U + 1):
            lp = joint(t, y[:u])
            lat[t, u, 0] = lp[-1]
            if u < U:
                lat[t, u, 1] = lp[y[u]]
    return lat


def _sweep(lat: np.ndarray, U: int, combine):
    """alpha [T, U + 1] by anti-diagonals d = t + u (every node of one depends on the one before only); ``combine`` is np.maximum
    or np.logaddexp."""
    T = lat.shape[0]
    a = np.full((T, U + 1), NEG)
    a[0, 0] = 0.0
    with np.errstate(invalid="ignore"):
        for d in range(1, T + U):
            u = np.arange(max(0, d - T + 1), min(U, d) + 1)
            t = d - u
            pb = np.where(t > 0, a[t - 1, u] + lat[t - 1, u, 0], NEG)
            pe = np.where(u > 0, a[t, u - 1] + lat[t, u - 1, 1], NEG)
            both = (pb == NEG) & (pe == NEG)
            a[t, u] = np.where(both, NEG, combine(np.where(both, 0.0, pb), np.where(both, 0.0, pe)))
    return a


def forward_loglik(lat: np.ndarray, U: Optional[int] = None) -> float:
    """log p(y | x) = alpha[T-1, U] + lb[T-1, U] (= -rnnt_loss).  T = 0: 0 if U = 0 else -inf."""
    U = lat.shape[1] - 1 if U is None else U
    if lat.shape[0] == 0:
        return 0.0 if U == 0 else NEG
    a = _sweep(lat, U, np.logaddexp)
    return float(a[-1, U] + lat[-1, U, 0])


def capped_loglik(lat: np.ndarray, S: int, U: Optional[int] = None) -> float:
    """log P_S(y | x) of the DECODERS' model (rnnt_beam_ref.exact_loglik on a lattice): at most S symbols per frame, and after S
    symbols the frame advances without a joint, i.e. with probability 1.  Where that free advance is used P_S can EXCEED the
    transducer likelihood, which pays lb there; where no alignment of weight reaches S symbols in a frame the two agree."""
    U = lat.shape[1] - 1 if U is None else U
    T = lat.shape[0]
    enter = np.full(U + 1, NEG)
    enter[0] = 0.0
    for t in range(T):
        arr = np.full((U + 1, S + 1), NEG)
        arr[:, 0] = enter
        for u in range(U):
            arr[u + 1, 1:] = np.logaddexp(arr[u + 1, 1:], arr[u, :S] + lat[t, u, 1])
        enter = np.logaddexp(np.logaddexp.reduce(arr[:, :S] + lat[t, :U + 1, :1], axis=1), arr[:, S])
    return float(enter[U])


def viterbi(lat: np.ndarray, U: Optional[int] = None) -> Tuple[float, List[int], bool]:
    """(score, tok_frame [U], feasible): the best path under the tie rule (blank predecessor on a tie)."""
    U = lat.shape[1] - 1 if U is None else U
    T = lat.shape[0]
    if T == 0:
        return (0.0, [], True) if U == 0 else (NEG, [], False)
    a = _sweep(lat, U, np.maximum)
    score = float(a[-1, U] + lat[-1, U, 0])
    if not score > NEG:
        return NEG, [], False
    t, u, fr = T - 1, U, [0] * U
    while u > 0:
        pb = a[t - 1, u] + lat[t - 1, u, 0] if t > 0 else NEG
        pe = a[t, u - 1] + lat[t, u - 1, 1]
        if pe > pb:
            fr[u - 1] = t
            u -= 1
        else:
            t -= 1
    return score, fr, True


def valid_path(tok_frame: Sequence[int], T: int) -> bool:
    """Token frames of a lattice path: non-decreasing and inside [0, T)."""
    fr = [int(f) for f in tok_frame]
    return all(0 <= f < T for f in fr) and all(a <= b for a, b in zip(fr, fr[1:]))


def rescore(lat: np.ndarray, tok_frame: Sequence[int]) -> float:
    """The log-prob of the path that emits y[u] at frame tok_frame[u] (and blank once per frame)."""
    T = lat.shape[0]
    fr = [int(f) for f in tok_frame]
    assert valid_path(fr, T), (fr, T)
    s, u = 0.0, 0
    for t in range(T):
        while u < len(fr) and fr[u] == t:
            s += lat[t, u, 1]
            u += 1
        s += lat[t, u, 0]
    assert u == len(fr)
    return float(s)


def brute_force(lat: np.ndarray, U: Optional[int] = None) -> Tuple[float, float, List[List[int]]]:
    """Every path of a tiny lattice: (best score, log-sum-exp of all, the token-frame lists of every path that attains the best)."""
    U = lat.shape[1] - 1 if U is None else U
    T = lat.shape[0]
    best, paths, tot = NEG, [], NEG
    for fr in itertools.combinations_with_replacement(range(T), U):
        s = rescore(lat[:, :U + 1], fr)
        tot = float(np.logaddexp(tot, s)) if max(tot, s) > NEG else NEG
        if s > best:
            best, paths = s, [list(fr)]
        elif s == best:
            paths.append(list(fr))
    return best, tot, paths


def tie_rule_path(paths: List[List[int]]) -> List[int]:
    """Of several best paths the tie rule keeps: walking back from (T-1, U), the blank predecessor wins, i.e. every token is
    emitted as EARLY as the set of best paths allows, decided from the last token to the first."""
    U = len(paths[0])
    cand = paths
    for u in range(U - 1, -1, -1):
        m = min(p[u] for p in cand)
        cand = [p for p in cand if p[u] == m]
    return cand[0]
