"""Float64 reference of the long CTC confidence pass (gam_op_ctc_confidence_long; the contract is in
gigaam_amd/csrc/gam_confidence.h).  ONE utterance of T frames: ``confidence_ref.ctc_confidence`` as it is (it has no length limit)
for a list without wildcards, plus the wildcard rule.

Wildcard rule (``wildcard=True``): id V, one past blank, is a valid entry.  Its frame takes part in the strictly-increasing check
and bounds the previous token's span like any token's; it is itself not scored: conf -1, span 0.  With ``wildcard=False`` id V is
invalid as any id outside [0, V - 2].  A list is valid only if EVERY entry is; an invalid list has status 0, every conf -1, every
span 0."""
from typing import List, Optional, Sequence, Tuple

import numpy as np

import confidence_ref as C


def ctc_confidence_long(lp: np.ndarray, ids: Sequence[int], frames: Sequence[int], measure: str = "prob", agg: str = "mean",
                        wildcard: bool = False, cap: Optional[int] = None) -> Tuple[List[float], List[int], int]:
    """lp [T, V] log-probs (argmaxes on the array as given: pass the fp32 array) -> (conf [U], span [U], status)."""
    lp = np.asarray(lp)
    T, V = lp.shape
    ids, frames = [int(i) for i in ids], [int(f) for f in frames]
    U = len(ids)
    if not wildcard or V not in ids:
        return C.ctc_confidence(lp, T, ids, frames, measure, agg, cap)
    if measure not in C.MEASURES:
        raise ValueError(measure)
    if agg not in C.AGGREGATIONS:
        raise ValueError(agg)
    # validity with the wildcards as ordinary entries of a legal id
    if not C.valid([0 if i == V else i for i in ids], frames, T, V, True, cap):
        return [-1.0] * U, [0] * U, 0
    conf, span = [], []
    for u in range(U):
        if ids[u] == V:
            conf.append(-1.0)
            span.append(0)
            continue
        lim = frames[u + 1] if u + 1 < U else T      # (the next entry bounds the span, wildcard or not)
        vals = [C.measure_logp(lp[frames[u]], ids[u], measure)]
        f = frames[u] + 1
        while f < lim and C.argmax_low(lp[f]) == ids[u]:
            vals.append(C.measure_logp(lp[f], ids[u], measure))
            f += 1
        conf.append(C.aggregate(vals, agg))
        span.append(len(vals))
    return conf, span, 1
