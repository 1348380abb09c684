"""Float64 reference of RNN-T beam search with hotwords AND a word n-gram LM (gigaam_amd/csrc/gam_rnnt_beam.h,
gam_rnnt_beam_kernel<true>).  numpy only; used by the CPU and the GPU tests.  Hypotheses, partial words and LM states are real
tuples here, the ARPA model the dict model of tests/ctc_lm_ref.py; the kernel identifies them by 64-bit hashes (gigaam_amd/lm.py).

The search is tests/rnnt_beam_ref.py's (same candidates, theta cut, merges, ties and frame rule) with one more per-hypothesis term,
under the word rules of tests/ctc_lm_ref.py (``LMSpec.step`` / ``LMSpec.final``):
  Each hypothesis carries an LM state (partial word, last order - 1 words, lm).  An extension a.y + v takes ``spec.step(state, v)``
  (a class-1/2 token completes a non-empty partial word: lm += alpha ln P(w | ctx) + beta); blank candidates and the forced advance
  keep the state.  Equal y means equal state, so the merge in B keeps it (asserted).  rank = score + committed + acc + lm, in the
  theta cut and in every top-W selection.
  Final pick: best score + committed + ``spec.final(state)`` (the last word, then alpha ln P(</s> | ctx)), ties to the lower beam
  position.  score = log p + committed + that LM term; logp = log p.  With lm=None the result is tests/rnnt_beam_ref.py's."""
from typing import Dict, List, Optional, Sequence

import numpy as np

from ctc_beam_ref import Trie
from rnnt_beam_ref import NEG, Predictor, joint_lp, topk_ids


def beam_search(head, encp, W: int, S: int, T: Optional[int] = None, hotwords: Sequence[Sequence[int]] = (),
                beta: float = 2.0, joint=None, lm=None) -> Dict[str, object]:
    """As rnnt_beam_ref.beam_search (same arguments and result keys), with the LM term of ``lm`` (a ctc_lm_ref.LMSpec) when given.
    Extra result keys: ``lm`` (the picked hypothesis's final LM term), ``states`` (the final beam's LM states) and ``merges`` (how
    many merges in B the search made, each with equal LM states)."""
    encp = np.asarray(encp, dtype=np.float64) if encp is not None else None
    T = encp.shape[0] if T is None else T
    pred = Predictor(head) if head is not None else None
    if joint is None:
        joint = lambda t, y: joint_lp(head, encp[t], pred(y))     # noqa: E731
    trie = Trie(hotwords)
    step = (lambda st, v: lm.step(st, v)) if lm is not None else (lambda st, v: st)     # noqa: E731
    lm0 = lm.start() if lm is not None else ((), (), 0.0)
    # a hypothesis: [y, score, hw state, frames, LM state]
    beam = [((), 0.0, (0, 0.0, 0.0), (), lm0)]
    margins: List[float] = []
    merges = 0

    def rank(sc, hw, ls):
        return sc + hw[2] + hw[1] + ls[2]

    for t in range(T):
        Bd: Dict[tuple, list] = {}      # y -> [score, best contributor score, key, hw, frames, merge gap, LM state]
        A = beam
        for s in range(S + 1):
            C = []
            for p, (y, sc, hw, fr, ls) in enumerate(A):
                if s < S:
                    lp = joint(t, y)
                    cands = [(sc + lp[-1], (s, p, 0))]
                    K = min(W, len(lp) - 1)
                    for v in topk_ids(lp, K):
                        hw2 = trie.step(hw, v, beta)
                        ls2 = step(ls, v)
                        sc2 = sc + lp[v]
                        C.append((rank(sc2, hw2, ls2), (s, p, v + 1), y + (v,), sc2, hw2, fr + (t,), ls2))
                else:
                    cands = [(sc, (s, p, 0))]
                for csc, key in cands:
                    if csc == NEG:
                        continue
                    e = Bd.get(y)
                    if e is None:
                        Bd[y] = [csc, csc, key, hw, fr, np.inf, ls]
                    else:
                        assert e[3] == hw and e[6] == ls, "hotword and LM state must depend on y only"
                        merges += 1
                        e[0] = float(np.logaddexp(e[0], csc))
                        e[5] = min(e[5], abs(csc - e[1]))
                        if csc > e[1]:
                            e[1], e[4] = csc, fr
            if not C:
                break
            ranks = sorted((rank(e[0], e[3], e[6]) for e in Bd.values()), reverse=True)
            theta = ranks[W - 1] if len(ranks) >= W else NEG
            if theta > NEG:
                margins.append(min(abs(c[0] - theta) for c in C))
            Cf = sorted([c for c in C if c[0] > theta], key=lambda c: (-c[0], c[1]))
            if len(Cf) > W:
                margins.append(Cf[W - 1][0] - Cf[W][0])
            A = [(c[2], c[3], c[4], c[5], c[6]) for c in Cf[:W]]
            if not A:
                break
        ranked = sorted(Bd.items(), key=lambda kv: (-rank(kv[1][0], kv[1][3], kv[1][6]), kv[1][2]))
        if len(ranked) > W:
            r = [rank(e[0], e[3], e[6]) for _, e in ranked]
            margins.append(r[W - 1] - r[W])
            ranked = ranked[:W]
        for _, e in ranked:
            if e[5] < np.inf:
                margins.append(e[5])
        beam = [(y, e[0], e[3], e[4], e[6]) for y, e in ranked]
    finals = []
    for i, (_, sc, hw, _, ls) in enumerate(beam):
        lmf = lm.final(ls) if lm is not None else 0.0
        finals.append((sc + hw[2] + lmf, i, lmf))
    finals.sort(key=lambda e: (-e[0], e[1]))
    y, sc, hw, fr, _ = beam[finals[0][1]]
    return {"ids": list(y), "frames": list(fr), "score": sc + hw[2] + finals[0][2], "logp": sc, "lm": finals[0][2],
            "beam": [(b[0], b[1]) for b in beam], "states": [b[4] for b in beam], "margins": margins, "merges": merges,
            "final_margin": float(finals[0][0] - finals[1][0]) if len(finals) > 1 else np.inf}
