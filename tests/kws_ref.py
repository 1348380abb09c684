"""Float64 reference of the keyword search (gigaam_amd/csrc/gam_kws.h restates the contract): the per-frame scores and starts of a
keyword in one utterance, the streaming hit rule, and the best score of an occurrence with a GIVEN start and end.

Log-probs lp [T, V] are read as they are, blank = V - 1; a keyword is 1..64 ids in [0, V - 2].  Emissions are log-likelihood ratios
against the greedy path, c_t(v) = lp[t, v] - max_w lp[t, w].  States: tok_i (i < U) and blk_i (i < U - 1); every state carries a
value and the start frame of its best path.  Predecessors come from frame t - 1 and a later candidate replaces the best so far only
if it is STRICTLY greater:
    tok_i, i > 0: stay tok_i, then blk_{i-1}, then tok_{i-1} (only if y_i != y_{i-1})
    tok_0:        stay tok_0, then a fresh start (value 0, start frame t)
    blk_i:        stay blk_i, then tok_i
-inf stays -inf with start -1."""
import numpy as np

NEG = -np.inf


def _step(dt, st, db, sb, ct, cb, allow, fresh, t):
    """One frame for a stack of lattices: dt / st / db / sb [R, U]; ct [U] the tokens' emissions, cb the blank's; allow [U] whether
    tok_{i-1} -> tok_i exists (column 0: the fresh start); fresh [R] whether row r may start at this frame."""
    R, U = dt.shape
    pb = np.concatenate([np.full((R, 1), NEG), db[:, :-1]], axis=1)
    psb = np.concatenate([np.full((R, 1), -1, dtype=np.int64), sb[:, :-1]], axis=1)
    pt = np.concatenate([np.where(fresh, 0.0, NEG)[:, None], dt[:, :-1]], axis=1)
    pst = np.concatenate([np.where(fresh, t, -1)[:, None], st[:, :-1]], axis=1)
    best, bs = dt.copy(), st.copy()
    m = pb > best
    best[m], bs[m] = pb[m], psb[m]
    m = allow[None, :] & (pt > best)
    best[m], bs[m] = pt[m], pst[m]
    bb, bbs = db.copy(), sb.copy()
    m = dt > bb
    bb[m], bbs[m] = dt[m], st[m]
    ndt = best + ct[None, :]
    ndb = bb + cb
    ndb[:, U - 1] = NEG                 # (there is no blank behind the last token)
    return ndt, np.where(ndt > NEG, bs, -1), ndb, np.where(ndb > NEG, bbs, -1)


def _emissions(lp, y):
    lp = np.asarray(lp, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    V = lp.shape[1]
    assert 1 <= len(y) <= 64 and y.min() >= 0 and y.max() <= V - 2
    c = lp - lp.max(axis=1, keepdims=True)
    allow = np.ones(len(y), dtype=bool)
    allow[1:] = y[1:] != y[:-1]
    return c[:, y], c[:, V - 1], allow


def dense(lp, y):
    """(E [T] float64, S [T] int64): the best score of an occurrence of y that ends at frame t (-inf: none) and its start frame."""
    ct, cb, allow = _emissions(lp, y)
    T, U = ct.shape
    dt, db = np.full((1, U), NEG), np.full((1, U), NEG)
    st, sb = np.full((1, U), -1, dtype=np.int64), np.full((1, U), -1, dtype=np.int64)
    E, S = np.full(T, NEG), np.full(T, -1, dtype=np.int64)
    one = np.ones(1, dtype=bool)
    for t in range(T):
        dt, st, db, sb = _step(dt, st, db, sb, ct[t], cb[t], allow, one, t)
        E[t], S[t] = dt[0, U - 1], st[0, U - 1]
    return E, S


def pick(E, S, min_score, max_hits):
    """The streaming hit rule on per-frame scores / starts -> ([(start, end, score)] the first max_hits hits, the count of all)."""
    hits, cand = [], None
    for t in range(len(E)):
        if not (E[t] >= min_score):
            continue
        if cand is None:
            cand = (E[t], int(S[t]), t)
        elif S[t] <= cand[2]:
            if E[t] >= cand[0]:
                cand = (E[t], int(S[t]), t)
        else:
            hits.append(cand)
            cand = (E[t], int(S[t]), t)
    if cand is not None:
        hits.append(cand)
    return [(s, e, sc) for sc, s, e in hits[:max_hits]], len(hits)


def span_scores(lp, y, starts, ends):
    """For each (s, e): the best score of a path that enters tok_0 fresh at EXACTLY frame s and is in tok_{U-1} at frame e (-inf
    when there is none, e.g. s < 0 or e - s + 1 too short).  One lattice per distinct start, stepped together."""
    ct, cb, allow = _emissions(lp, y)
    T, U = ct.shape
    starts, ends = np.asarray(starts, dtype=np.int64), np.asarray(ends, dtype=np.int64)
    out = np.full(len(starts), NEG)
    ok = (starts >= 0) & (ends >= starts) & (ends < T)
    if not ok.any():
        return out
    us = np.unique(starts[ok])
    last = np.array([ends[ok & (starts == s)].max() for s in us])
    row_of = {int(s): r for r, s in enumerate(us)}
    by_end = {}
    for i in np.nonzero(ok)[0]:
        by_end.setdefault(int(ends[i]), []).append(i)
    R = len(us)
    dt, db = np.full((R, U), NEG), np.full((R, U), NEG)
    st, sb = np.full((R, U), -1, dtype=np.int64), np.full((R, U), -1, dtype=np.int64)
    for t in range(int(us.min()), int(last.max()) + 1):
        act = np.nonzero((us <= t) & (t <= last))[0]
        if len(act) == 0:
            continue
        dt[act], st[act], db[act], sb[act] = _step(dt[act], st[act], db[act], sb[act], ct[t], cb[t], allow, us[act] == t, t)
        for i in by_end.get(t, ()):
            out[i] = dt[row_of[int(starts[i])], U - 1]
    return out


def span_score(lp, y, s, e):
    return float(span_scores(lp, y, [s], [e])[0])
