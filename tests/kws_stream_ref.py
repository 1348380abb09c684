"""Float64 reference of the RESUMABLE keyword search (gam_ctc_kws_stream_kernel, gigaam_amd/csrc/gam_kws.h): tests/kws_ref.py's
``dense`` + ``pick`` restated with the state passed in and out, so that a stream can be fed in pieces.  The step is kws_ref's own
(``_step``); what is new is only what is carried: the lattice, the open candidate, the hit count and the next frame."""
import numpy as np

import kws_ref as R

NEG = -np.inf


def begin(U, t_base=0):
    """The state of a stream before its first frame: every lattice state -inf / -1, no candidate, no hit."""
    return {"dt": np.full((1, U), NEG), "db": np.full((1, U), NEG), "st": np.full((1, U), -1, dtype=np.int64),
            "sb": np.full((1, U), -1, dtype=np.int64), "cand": None, "n": 0, "next": int(t_base), "ended": False}


def push(state, lp, y, min_score, hits, max_hits, end=False):
    """Rows ``lp`` [n, V] are stream frames state["next"] ..: returns (state', E [n], S [n]); hits that close are appended to ``hits``
    as (start, end, score) while the list is shorter than ``max_hits``; state'["n"] counts every one.  ``end``: emit the open candidate
    behind the last row.  ``state`` is not changed."""
    assert not state["ended"]
    lp = np.asarray(lp, dtype=np.float64).reshape(-1, np.shape(lp)[-1])
    n, U = lp.shape[0], len(y)
    dt, st, db, sb = state["dt"], state["st"], state["db"], state["sb"]
    cand, count, t0 = state["cand"], state["n"], state["next"]
    E, S = np.full(n, NEG), np.full(n, -1, dtype=np.int64)
    one = np.ones(1, dtype=bool)

    def emit(c):
        nonlocal count
        if count < max_hits:
            hits.append((c[1], c[2], c[0]))
        count += 1

    if n:
        ct, cb, allow = R._emissions(lp, y)
    for r in range(n):
        t = t0 + r
        dt, st, db, sb = R._step(dt, st, db, sb, ct[r], cb[r], allow, one, t)
        E[r], S[r] = dt[0, U - 1], st[0, U - 1]
        if not (E[r] >= min_score):
            continue
        if cand is None:
            cand = (E[r], int(S[r]), t)
        elif S[r] <= cand[2]:
            if E[r] >= cand[0]:
                cand = (E[r], int(S[r]), t)
        else:
            emit(cand)
            cand = (E[r], int(S[r]), t)
    if end and cand is not None:
        emit(cand)
        cand = None
    return ({"dt": dt, "db": db, "st": st, "sb": sb, "cand": cand, "n": count, "next": t0 + n, "ended": bool(end)}, E, S)


def run(lp, y, min_score, max_hits, cuts, t_base=0):
    """The stream ``lp`` [T, V] fed in the pieces that ``cuts`` (sorted frame indices, repeats allowed: pieces of 0 frames) make, END as
    a call of its own -> (E [T], S [T], hits, count of all hits).  E / S / hit frames are stream frames (``t_base`` onwards)."""
    T = np.shape(lp)[0]
    edges = [0] + [int(c) for c in cuts] + [T]
    state, hits, Es, Ss = begin(len(y), t_base), [], [], []
    for a, b in zip(edges[:-1], edges[1:]):
        state, E, S = push(state, lp[a:b], y, min_score, hits, max_hits)
        Es.append(E)
        Ss.append(S)
    state, _, _ = push(state, lp[:0], y, min_score, hits, max_hits, end=True)
    return np.concatenate(Es), np.concatenate(Ss), hits, state["n"]
