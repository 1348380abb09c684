"""Float64 reference of token, word and utterance confidence (gigaam_amd/csrc/gam_confidence.h holds the contract).  Used by the
CPU and the GPU tests.

Per utterance: T = enc_len, the decoded ``ids[0..U)`` at ``frames[0..U)``, blank = V - 1.
  step distribution  CTC: p_f = exp(lp[f, :]) over all V classes of frame f.  RNN-T, token u: the joint's softmax at node
                     (frames[u], ids[:u]) -- the distribution the token was emitted from.
  measure            "prob": p(decoded token); "entropy": 1 - H(p) / ln V, H = -sum p ln p (p = 0 adds 0).  Clamped into [0, 1].
  CTC span           frames[u], then every next frame < frames[u + 1] (< T for the last token) whose argmax over all V classes
                     (ties to the lower id, on the fp32 values as stored) is ids[u].  frames[u] always belongs.
  aggregation        "mean" / "min" / "prod": over a CTC token's span, over the tokens of a word, over all tokens (the utterance;
                     None for an empty transcript).
  validity           an id outside [0, V - 2], a frame outside [0, T), CTC frames not strictly increasing, RNN-T frames
                     decreasing, more tokens than ``cap``: status 0, every confidence -1, every span 0."""
from typing import List, Optional, Sequence, Tuple

import numpy as np

MEASURES = {"prob": 0, "entropy": 1}
AGGREGATIONS = {"mean": 0, "min": 1, "prod": 2}


def aggregate(values: Sequence[float], how: str) -> Optional[float]:
    if how not in AGGREGATIONS:
        raise ValueError(how)
    v = [float(x) for x in values]
    if not v:
        return None
    if how == "mean":
        return sum(v) / len(v)
    if how == "min":
        return min(v)
    return float(np.prod(np.asarray(v, dtype=np.float64)))


def measure_logp(lp_row: np.ndarray, token: int, measure: str) -> float:
    """The measure of one step from its log-probs (any float array: promoted to float64)."""
    lp = np.asarray(lp_row, dtype=np.float64)
    if measure == "prob":
        c = float(np.exp(lp[token]))
    elif measure == "entropy":
        p = np.exp(lp)
        with np.errstate(invalid="ignore"):
            h = -float(np.where(p > 0.0, p * lp, 0.0).sum())
        c = 1.0 - h / np.log(len(lp))
    else:
        raise ValueError(measure)
    return min(max(c, 0.0), 1.0)


def argmax_low(row: np.ndarray) -> int:
    """First maximum of the values as stored (np.argmax returns the lowest index of a tie)."""
    return int(np.argmax(row))


def valid(ids: Sequence[int], frames: Sequence[int], T: int, V: int, strict: bool, cap: Optional[int] = None) -> bool:
    ids, frames = [int(i) for i in ids], [int(f) for f in frames]
    if len(ids) != len(frames) or (cap is not None and len(ids) > cap):
        return False
    if any(i < 0 or i > V - 2 for i in ids) or any(f < 0 or f >= T for f in frames):
        return False
    return all((a < b) if strict else (a <= b) for a, b in zip(frames, frames[1:]))


def ctc_confidence(lp: np.ndarray, T: int, ids: Sequence[int], frames: Sequence[int], measure: str = "prob", agg: str = "mean",
                   cap: Optional[int] = None) -> Tuple[List[float], List[int], int]:
    """lp [>= T, V] log-probs of ONE utterance (argmaxes on the array as given: pass the fp32 array) -> (conf [U], span [U], status)."""
    if measure not in MEASURES:
        raise ValueError(measure)
    if agg not in AGGREGATIONS:
        raise ValueError(agg)
    lp = np.asarray(lp)
    V = lp.shape[-1]
    U = len(ids)
    if not valid(ids, frames, T, V, True, cap):
        return [-1.0] * U, [0] * U, 0
    conf, span = [], []
    for u in range(U):
        tok, f0 = int(ids[u]), int(frames[u])
        lim = int(frames[u + 1]) if u + 1 < U else T
        vals = [measure_logp(lp[f0], tok, measure)]
        f = f0 + 1
        while f < lim and argmax_low(lp[f]) == tok:
            vals.append(measure_logp(lp[f], tok, measure))
            f += 1
        conf.append(aggregate(vals, agg))
        span.append(len(vals))
    return conf, span, 1


def ctc_greedy(lp: np.ndarray, T: int) -> Tuple[List[int], List[int]]:
    """The greedy decode of lp [>= T, V]: (ids, first frames of their runs)."""
    lp = np.asarray(lp)
    blank = lp.shape[-1] - 1
    ids, frames, prev = [], [], blank
    for t in range(T):
        k = argmax_low(lp[t])
        if k != blank and k != prev:
            ids.append(k)
            frames.append(t)
        prev = k
    return ids, frames


def rnnt_node_logp(head, pred, encp_t: np.ndarray, prefix: Sequence[int]) -> np.ndarray:
    """log_softmax of the joint at (frame, prefix): the weight-level joint of tests/rnnt_align_ref.lattice, one node at a time.
    ``pred``: an rnnt_beam_ref.Predictor of ``head`` (caches the prefixes)."""
    z = np.maximum(np.asarray(encp_t, dtype=np.float64) + pred(tuple(int(v) for v in prefix)), 0.0) @ head["out_w"].T + head["out_b"]
    m = z.max()
    return z - (m + np.log(np.exp(z - m).sum()))


def rnnt_confidence(head, encp: np.ndarray, T: int, ids: Sequence[int], frames: Sequence[int], measure: str = "prob",
                    cap: Optional[int] = None) -> Tuple[List[float], int]:
    """encp [>= T, JH] (W_enc f + b_enc) of ONE utterance -> (conf [U], status)."""
    import rnnt_beam_ref as R
    if measure not in MEASURES:
        raise ValueError(measure)
    V = len(head["out_b"])
    U = len(ids)
    if not valid(ids, frames, T, V, False, cap):
        return [-1.0] * U, 0
    pred = R.Predictor(head)
    y = [int(i) for i in ids]
    return [measure_logp(rnnt_node_logp(head, pred, encp[int(frames[u])], y[:u]), y[u], measure) for u in range(U)], 1


def word_groups(tokenizer, ids: Sequence[int]) -> List[List[int]]:
    """Token positions of every word ``timestamps_utils.frames_to_words`` returns, by the class rules of gam_search.h / lm.py: a
    piece that starts with the SentencePiece marker starts a new word and belongs to it; the " " token of a char-wise vocabulary
    separates words and belongs to none; a group whose text is empty is no word."""
    groups: List[List[int]] = []
    cur: List[int] = []
    text: List[str] = []

    def flush():
        if "".join(text).strip():
            groups.append(list(cur))
        cur.clear()
        text.clear()

    for i, tok in enumerate(ids):
        piece = tokenizer.id_to_str(int(tok))
        if piece.startswith("▁"):
            flush()
            piece = piece[1:]
        elif piece == " ":
            flush()
            continue
        cur.append(i)
        text.append(piece)
    flush()
    return groups


def word_confidences(tokenizer, ids: Sequence[int], conf: Sequence[float], agg: str) -> List[float]:
    return [aggregate([conf[i] for i in g], agg) for g in word_groups(tokenizer, ids)]
