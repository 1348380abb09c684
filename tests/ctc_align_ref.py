"""Float64 reference of CTC forced alignment (gigaam_amd/csrc/gam_align.h): Viterbi with the library's tie rule, the forward
log-likelihood, and a validator / rescorer for a returned path.  numpy only; used by the CPU and the GPU tests.

Tie rule: among equal predecessors the path keeps state s over s-1 over s-2; at the end it prefers S-1 (the last token) over S-2
(the trailing blank).  Read backwards from the last frame, the returned path is therefore the lexicographically largest state
sequence among the optimal ones."""
from typing import List, Optional, Sequence, Tuple

import numpy as np

NEG = -np.inf


def feasible(T: int, y: Sequence[int], V: int) -> bool:
    """A CTC path for ``y`` exists in T frames, and every id is a non-blank class (blank = V - 1)."""
    if any(int(v) < 0 or int(v) > V - 2 for v in y):
        return False
    reps = sum(1 for i in range(1, len(y)) if y[i] == y[i - 1])
    return T >= len(y) + reps


def _shift(x: np.ndarray, k: int) -> np.ndarray:
    """x[s - k] at s (-inf before the start)."""
    return np.concatenate([np.full(k, NEG), x])[: len(x)]


def _lattice(y: Sequence[int], blank: int):
    S = 2 * len(y) + 1
    lab = np.full(S, blank, dtype=np.int64)
    lab[1::2] = np.asarray(y, dtype=np.int64)
    skip = np.zeros(S, dtype=bool)
    for s in range(3, S, 2):
        skip[s] = lab[s] != lab[s - 2]
    return S, lab, skip


def viterbi(lp: np.ndarray, y: Sequence[int], T: Optional[int] = None):
    """lp [>= T, V] log-probs -> (score, states [T]) of the best path for target ``y`` (blank = V - 1), or (-inf, None) if
    there is none.  T = 0 with an empty target scores 0 with an empty path."""
    lp = np.asarray(lp, dtype=np.float64)
    V = lp.shape[1]
    T = lp.shape[0] if T is None else T
    if not feasible(T, y, V):
        return NEG, None
    if T == 0:
        return 0.0, []
    S, lab, skip = _lattice(y, V - 1)
    prev = np.full(S, NEG)
    prev[0] = 0.0                    # a virtual start at t = -1 that only state 0 holds
    bps = np.zeros((T, S), dtype=np.int8)
    for t in range(T):
        d0 = prev
        d1 = _shift(prev, 1)
        d2 = np.where(skip, _shift(prev, 2), NEG)
        best = d0.copy()
        bp = np.zeros(S, dtype=np.int8)
        m = d1 > best
        best[m], bp[m] = d1[m], 1
        m = d2 > best
        best[m], bp[m] = d2[m], 2
        prev = best + lp[t, lab]
        bps[t] = bp
    s = S - 1
    if S >= 2 and prev[S - 2] > prev[S - 1]:
        s = S - 2
    score = prev[s]
    if not np.isfinite(score):
        return NEG, None
    states = [0] * T
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(bps[t, s])
    return float(score), states


def forward_loglik(lp: np.ndarray, y: Sequence[int], T: Optional[int] = None) -> float:
    """log p(y | lp) summed over every CTC path (= -ctc_loss), float64."""
    lp = np.asarray(lp, dtype=np.float64)
    V = lp.shape[1]
    T = lp.shape[0] if T is None else T
    if not feasible(T, y, V):
        return NEG
    if T == 0:
        return 0.0
    S, lab, skip = _lattice(y, V - 1)
    prev = np.full(S, NEG)
    prev[0] = 0.0
    for t in range(T):
        a1 = _shift(prev, 1)
        a2 = np.where(skip, _shift(prev, 2), NEG)
        prev = np.logaddexp(np.logaddexp(prev, a1), a2) + lp[t, lab]
    return float(np.logaddexp(prev[S - 1], prev[S - 2]) if S >= 2 else prev[S - 1])


def state_labels(states: Sequence[int], y: Sequence[int], blank: int) -> List[int]:
    return [int(y[(s - 1) // 2]) if s % 2 else blank for s in states]


def token_runs(states: Sequence[int], U: int) -> Tuple[List[int], List[int]]:
    """First / last frame of each token's run on a state path."""
    first, last = [-1] * U, [-1] * U
    for t, s in enumerate(states):
        if s % 2:
            u = (s - 1) // 2
            if first[u] < 0:
                first[u] = t
            last[u] = t
    return first, last


def path_states(labels: Sequence[int], y: Sequence[int], blank: int) -> Optional[List[int]]:
    """The state sequence of a per-frame label path, or None if the labels are not a CTC path for ``y``."""
    states, u, prev = [], 0, blank      # u = tokens emitted so far
    for lab in labels:
        lab = int(lab)
        if lab == blank:
            states.append(2 * u)
        elif u > 0 and lab == prev and states and states[-1] == 2 * u - 1:
            states.append(2 * u - 1)    # the current token's run goes on
        elif u < len(y) and lab == y[u]:
            u += 1
            states.append(2 * u - 1)
        else:
            return None
        prev = lab
    return states if u == len(y) else None


def rescore(lp: np.ndarray, labels: Sequence[int]) -> float:
    lp = np.asarray(lp, dtype=np.float64)
    return float(sum(lp[t, int(l)] for t, l in enumerate(labels)))
