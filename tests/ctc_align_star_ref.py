"""Float64 reference of CTC forced alignment with wildcard tokens (gigaam_amd/csrc/gam_trellis.h, the STAR variants).

A wildcard is target id V, one past blank (V - 1): an ordinary CTC token whose emission at frame t is ``star[t]``.  So the whole
reference is tests/ctc_align_ref.py on an AUGMENTED matrix with one more column: ``[lp[:, :V-1], star, lp[:, V-1]]`` maps the
wildcard to id V - 1 and blank to id V, both where ctc_align_ref expects them (blank = the last column); ordinary ids keep theirs.
numpy only; used by the CPU and the GPU tests."""
from typing import List, Optional, Sequence, Tuple

import numpy as np

import ctc_align_ref as R

NEG = R.NEG


def feasible(T: int, y: Sequence[int], V: int) -> bool:
    """The star rule: ids in [0, V-2] or V (the wildcard; blank V - 1 stays a bad id), and T >= U + repeats with wildcards counted
    in U and two adjacent wildcards counted as a repeat."""
    if any(int(v) < 0 or int(v) > V or int(v) == V - 1 for v in y):
        return False
    reps = sum(1 for i in range(1, len(y)) if y[i] == y[i - 1])
    return T >= len(y) + reps


def augment(lp: np.ndarray, star: np.ndarray) -> np.ndarray:
    """lp [T, V], star [T] -> float64 [T, V + 1]: labels | wildcard | blank."""
    lp = np.asarray(lp, dtype=np.float64)
    star = np.asarray(star, dtype=np.float64)[: lp.shape[0]]
    return np.concatenate([lp[:, :-1], star[:, None], lp[:, -1:]], axis=1)


def map_target(y: Sequence[int], V: int) -> List[int]:
    """Target ids of the caller (wildcard = V) -> ids of the augmented matrix (wildcard = V - 1)."""
    return [V - 1 if int(v) == V else int(v) for v in y]


def map_labels(labels: Sequence[int], V: int) -> List[int]:
    """Per-frame labels of the kernel (blank = V - 1, wildcard = V) -> labels of the augmented matrix (wildcard V - 1, blank V)."""
    return [V if int(l) == V - 1 else (V - 1 if int(l) == V else int(l)) for l in labels]


def viterbi(lp: np.ndarray, star: np.ndarray, y: Sequence[int], T: Optional[int] = None):
    """(score, states [T]) of the best path, or (-inf, None): ctc_align_ref.viterbi on the augmented matrix."""
    V = np.asarray(lp).shape[1]
    T = np.asarray(lp).shape[0] if T is None else T
    if not feasible(T, y, V):
        return NEG, None
    return R.viterbi(augment(lp, star), map_target(y, V), T)


def forward_loglik(lp: np.ndarray, star: np.ndarray, y: Sequence[int], T: Optional[int] = None) -> float:
    V = np.asarray(lp).shape[1]
    T = np.asarray(lp).shape[0] if T is None else T
    if not feasible(T, y, V):
        return NEG
    return R.forward_loglik(augment(lp, star), map_target(y, V), T)


def path_states(labels: Sequence[int], y: Sequence[int], V: int) -> Optional[List[int]]:
    """The state sequence of the kernel's per-frame labels, or None if they are not a CTC path of ``y``."""
    return R.path_states(map_labels(labels, V), map_target(y, V), V)


def token_runs(states: Sequence[int], U: int) -> Tuple[List[int], List[int]]:
    return R.token_runs(states, U)


def state_labels(states: Sequence[int], y: Sequence[int], V: int) -> List[int]:
    """Per-frame labels in the kernel's ids (blank V - 1, wildcard V) of a state path."""
    return [int(y[(s - 1) // 2]) if s % 2 else V - 1 for s in states]


def rescore(lp: np.ndarray, star: np.ndarray, labels: Sequence[int]) -> float:
    """The log-prob of the kernel's per-frame labels."""
    V = np.asarray(lp).shape[1]
    return R.rescore(augment(lp, star), map_labels(labels, V))


def star_row(lp: np.ndarray, penalty: float) -> np.ndarray:
    """max_v lp[t, v] - penalty in float32 arithmetic, as the row kernel computes it."""
    return (np.asarray(lp, dtype=np.float32).max(axis=-1) - np.float32(penalty)).astype(np.float32)
