"""Float64 reference of CTC prefix beam search with hotword boosting (gigaam_amd/csrc/gam_beam.h; the hotword rules: gam_search.h).  numpy only; used by the CPU
and the GPU tests.  Prefixes are real tuples here (the kernel identifies them by length and a 64-bit hash).

Per frame t, every beam entry y (last token l, p_b / p_nb: log-probs of the paths ending in blank / non-blank) contributes
  stay    y.p_b     (+)= (p_b (+) p_nb) + lp[t, blank]
  repeat  y.p_nb    (+)= p_nb + lp[t, l]                     (y non-empty; whether or not l is a candidate)
  extend  (y+c).p_nb (+)= (c == l ? p_b : p_b (+) p_nb) + lp[t, c]   for c in the top-K non-blank ids of lp[t] (ties: lower id)
with (+) = log-add-exp and K = min(W, V - 1).  Candidates naming the same prefix merge (an extension may equal another entry).  The
new beam is the top W by rank = (p_b (+) p_nb) + bonus, ties by the origin key (source entry's position, -1 for stay / repeat else c)
ascending; a merged prefix takes its smallest key.  Candidates of rank -inf are dropped.
Token frames: an extension's token enters at t; a merged prefix keeps the entry's frames unless the extension's term outweighs the
entry's own stay + repeat mass, when its last token re-enters at t -- so each frame is the first of the token's run on the best path.

Hotwords: a trie of token-id phrases, one boost beta per matched token.  Only an extension by c moves the state (node, acc): to the
child of node for c (acc += beta; at a phrase end acc is committed and reset; the walk stays on the node if it has children, else
returns to the root), else the pending acc is rolled back and the walk restarts from the root's child for c.  No failure links.
bonus = committed + acc.  The final pick drops the pending acc: best (p_b (+) p_nb) + committed, ties to the lower beam position.
With ``lm`` (a ctc_lm_ref.LMSpec, where the word rules are) every prefix carries an LM state; its term joins the rank and the final pick."""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

NEG = -np.inf


class Trie:
    """Hotword phrases (token-id sequences) as a trie: node 0 is the root."""

    def __init__(self, phrases: Sequence[Sequence[int]] = ()):
        self.kids: List[Dict[int, int]] = [{}]
        self.end: List[bool] = [False]
        for p in phrases:
            n = 0
            for c in p:
                c = int(c)
                if c not in self.kids[n]:
                    self.kids.append({})
                    self.end.append(False)
                    self.kids[n][c] = len(self.kids) - 1
                n = self.kids[n][c]
            if len(p):
                self.end[n] = True

    def step(self, state: Tuple[int, float, float], c: int, beta: float) -> Tuple[int, float, float]:
        """(node, acc, committed) after an extension by c."""
        node, acc, cb = state
        child = self.kids[node].get(c)
        if child is None and node != 0:
            acc, node = 0.0, 0                      # roll back the partial match, restart from the root
            child = self.kids[0].get(c)
        if child is None:
            return 0, 0.0, cb
        acc += beta
        if self.end[child]:
            cb, acc = cb + acc, 0.0
        return (child if self.kids[child] else 0), acc, cb

    def bonus(self, y: Sequence[int], beta: float) -> float:
        """The committed bonus of a complete label sequence (the pending part dropped)."""
        st = (0, 0.0, 0.0)
        for c in y:
            st = self.step(st, int(c), beta)
        return st[2]


def _lse(a: float, b: float) -> float:
    return float(np.logaddexp(a, b))


def topk_ids(row: np.ndarray, k: int) -> List[int]:
    """The top-k non-blank ids of one log-prob row (blank = last), ties to the lower id."""
    v = np.asarray(row[:-1], dtype=np.float64)
    order = np.lexsort((np.arange(len(v)), -v))
    return [int(i) for i in order[:k]]


def beam_search(lp: np.ndarray, W: Optional[int], T: Optional[int] = None, hotwords: Sequence[Sequence[int]] = (),
                beta: float = 2.0, lm=None) -> Dict[str, object]:
    """lp [>= T, V] log-probs (blank = V - 1), beam width W (None: unbounded, every non-blank id a candidate), ``lm`` a
    ctc_lm_ref.LMSpec or None (its term is then an exact + 0.0).  Returns ids, frames (the frame each token's extension entered the
    beam), score (log p + committed bonus + LM term), logp, lm (the LM term), margins (per frame: rank of the W-th kept minus rank of
    the (W+1)-th candidate, inf when nothing was cut, or the smaller gap between the two terms of a kept merge) and final_margin (best
    minus second best final value, inf with one entry)."""
    lp = np.asarray(lp, dtype=np.float64)
    V = lp.shape[1]
    T = lp.shape[0] if T is None else T
    blank = V - 1
    K = V - 1 if W is None else min(W, V - 1)
    trie = Trie(hotwords)
    lm0 = lm.start() if lm is not None else ((), (), 0.0)
    beam = [((), 0.0, NEG, (0, 0.0, 0.0), (), lm0)]
    margins: List[float] = []
    for t in range(T):
        row = lp[t]
        cand_ids = topk_ids(row, K)
        cands: Dict[tuple, list] = {}

        def add(y, pb, pnb, key, hw, frames, stay, ls):
            e = cands.setdefault(y, [NEG, NEG, key, hw, None, None, NEG, NEG, ls])
            e[0], e[1] = _lse(e[0], pb), _lse(e[1], pnb)
            e[2] = min(e[2], key)
            assert e[3] == hw and e[8] == ls, "hotword and LM state must depend on the prefix only"
            e[4 if stay else 5] = frames
            e[6 if stay else 7] = _lse(pb, pnb)

        for i, (y, pb, pnb, hw, fr, ls) in enumerate(beam):
            tot = _lse(pb, pnb)
            add(y, tot + row[blank], (pnb + row[y[-1]]) if y else NEG, (i, -1), hw, fr, True, ls)
            for c in cand_ids:
                base = pb if (y and c == y[-1]) else tot
                add(y + (c,), NEG, base + row[c], (i, c), trie.step(hw, c, beta), fr + (t,), False,
                    lm.step(ls, c) if lm is not None else ls)
        ranked = []
        for y, (pb, pnb, key, hw, fs, fe, ms, me, ls) in cands.items():
            r = _lse(pb, pnb) + hw[2] + hw[1] + ls[2]
            fr = fe if me > ms else fs
            if r > NEG:
                ranked.append((-r, key, y, pb, pnb, hw, fr, abs(ms - me) if ms > NEG and me > NEG else np.inf, ls))
        ranked.sort(key=lambda e: (e[0], e[1]))
        if W is not None and len(ranked) > W:
            cut = float(ranked[W][0] - ranked[W - 1][0])
            ranked = ranked[:W]
        else:
            cut = np.inf
        margins.append(min([cut] + [e[7] for e in ranked]))
        beam = [(y, pb, pnb, hw, fr, ls) for _, _, y, pb, pnb, hw, fr, _, ls in ranked]
    if T == 0:
        return {"ids": [], "frames": [], "score": 0.0, "logp": 0.0, "lm": 0.0, "margins": [], "final_margin": np.inf}
    finals = []
    for i, (_, pb, pnb, hw, _, ls) in enumerate(beam):
        lmf = lm.final(ls) if lm is not None else 0.0
        finals.append((_lse(pb, pnb) + hw[2] + lmf, i, lmf))
    finals.sort(key=lambda e: (-e[0], e[1]))
    y, pb, pnb, hw, fr, _ = beam[finals[0][1]]
    logp = _lse(pb, pnb)
    return {"ids": list(y), "frames": list(fr), "score": logp + hw[2] + finals[0][2], "logp": logp, "lm": finals[0][2],
            "margins": margins, "final_margin": float(finals[0][0] - finals[1][0]) if len(finals) > 1 else np.inf}


def min_margin(res: Dict[str, object]) -> float:
    """The smallest decision margin of a run: every frame's cut and the final pick."""
    return float(min([res["final_margin"]] + list(res["margins"])))
