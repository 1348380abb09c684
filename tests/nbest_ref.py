"""Float64 N-best references: the searches of tests/ctc_beam_ref.py and tests/rnnt_beam_ref.py restated so that they return EVERY entry
of the final beam, best first, instead of the best one (gam_ctc_beam_nbest / gam_rnnt_beam_nbest; the emission: gam_search.h).

An entry's value is what the 1-best pick ranks by -- log p + committed hotword bonus + LM term with the last word and </s> (the pending
hotword part dropped); order: value descending, ties to the lower beam position.  ``hyps`` [{ids, frames, score, logp}], ``margins``
(the per-frame decision margins of the 1-best references) and ``final_gaps`` (value r minus value r + 1).  tests/test_nbest_host.py
holds hyps[0] equal to the 1-best references, so the two cannot drift.

Qualification: the kernels rank in fp32, the references in fp64; an utterance is compared for N hypotheses when every per-frame margin
and every gap among the first min(N + 1, n) final values exceed the margin of the search's 1-best test module."""
import itertools
from typing import Dict, List, Optional, Sequence

import numpy as np

import ctc_align_ref as A
from ctc_beam_ref import NEG, Trie, _lse, topk_ids
from rnnt_beam_ref import Predictor, exact_loglik, joint_lp, topk_ids as rnnt_topk_ids

CTC_MARGIN = 2e-5       # tests/test_hip_ctc_beam.py MARGIN (op level)
RNNT_MARGIN = 1e-4      # tests/test_hip_rnnt_beam.py MARGIN (op level)


def _result(entries, margins) -> Dict[str, object]:
    """entries: [(value, position, ids, frames, score, logp)] of the final beam."""
    entries = sorted(entries, key=lambda e: (-e[0], e[1]))
    return {"hyps": [{"ids": list(e[2]), "frames": list(e[3]), "score": e[4], "logp": e[5]} for e in entries],
            "values": [e[0] for e in entries], "margins": list(margins),
            "final_gaps": [float(entries[i][0] - entries[i + 1][0]) for i in range(len(entries) - 1)]}


def ctc_nbest(lp: np.ndarray, W: int, T: Optional[int] = None, hotwords: Sequence[Sequence[int]] = (), beta: float = 2.0,
              lm=None) -> Dict[str, object]:
    """ctc_beam_ref.beam_search's search (same arithmetic, same order of operations) returning the whole final beam."""
    lp = np.asarray(lp, dtype=np.float64)
    V = lp.shape[1]
    T = lp.shape[0] if T is None else T
    blank = V - 1
    K = min(W, V - 1)
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
            assert e[3] == hw and e[8] == ls
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
        if len(ranked) > W:
            cut = float(ranked[W][0] - ranked[W - 1][0])
            ranked = ranked[:W]
        else:
            cut = np.inf
        margins.append(min([cut] + [e[7] for e in ranked]))
        beam = [(y, pb, pnb, hw, fr, ls) for _, _, y, pb, pnb, hw, fr, _, ls in ranked]
    if T == 0:
        return _result([(0.0, 0, (), (), 0.0, 0.0)], [])
    entries = []
    for i, (y, pb, pnb, hw, fr, ls) in enumerate(beam):
        lmf = lm.final(ls) if lm is not None else 0.0
        logp = _lse(pb, pnb)
        entries.append((logp + hw[2] + lmf, i, y, fr, logp + hw[2] + lmf, logp))
    return _result(entries, margins)


def rnnt_nbest(head, encp, W: int, S: int, T: Optional[int] = None, hotwords: Sequence[Sequence[int]] = (), beta: float = 2.0,
               joint=None, lm=None) -> Dict[str, object]:
    """rnnt_beam_ref.beam_search's search (same arithmetic, same order of operations) returning the whole final beam."""
    encp = np.asarray(encp, dtype=np.float64) if encp is not None else None
    T = encp.shape[0] if T is None else T
    pred = Predictor(head) if head is not None else None
    if joint is None:
        joint = lambda t, y: joint_lp(head, encp[t], pred(y))     # noqa: E731
    trie = Trie(hotwords)
    step = (lambda st, v: lm.step(st, v)) if lm is not None else (lambda st, v: st)     # noqa: E731
    lm0 = lm.start() if lm is not None else ((), (), 0.0)
    beam = [((), 0.0, (0, 0.0, 0.0), (), lm0)]
    margins: List[float] = []

    def rank(sc, hw, ls):
        return sc + hw[2] + hw[1] + ls[2]

    for t in range(T):
        Bd: Dict[tuple, list] = {}
        Al = beam
        for s in range(S + 1):
            C = []
            for p, (y, sc, hw, fr, ls) in enumerate(Al):
                if s < S:
                    lp = joint(t, y)
                    cands = [(sc + lp[-1], (s, p, 0))]
                    K = min(W, len(lp) - 1)
                    for v in rnnt_topk_ids(lp, K):
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
                        assert e[3] == hw and e[6] == ls
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
            Al = [(c[2], c[3], c[4], c[5], c[6]) for c in Cf[:W]]
            if not Al:
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
    entries = []
    for i, (y, sc, hw, fr, ls) in enumerate(beam):
        lmf = lm.final(ls) if lm is not None else 0.0
        entries.append((sc + hw[2] + lmf, i, y, fr, sc + hw[2] + lmf, sc))
    return _result(entries, margins)


def qualifies(res: Dict[str, object], n_best: int, margin: float) -> bool:
    """Every per-frame margin and every gap among the first min(n_best + 1, n) final values exceed ``margin``."""
    n = len(res["hyps"])
    gaps = res["final_gaps"][: max(min(n_best + 1, n) - 1, 0)]
    return bool(min(list(res["margins"]) + list(gaps) + [np.inf]) > margin)


def _brute(V: int, T: int, loglik, trie: Trie, beta: float) -> List[tuple]:
    """Every label sequence of at most T non-blank tokens with a finite value: [(value, y, log p)], value descending."""
    out = []
    for n in range(T + 1):
        for y in itertools.product(range(V - 1), repeat=n):
            ll = loglik(y)
            if ll > NEG:
                out.append((ll + trie.bonus(y, beta), list(y), ll))
    out.sort(key=lambda e: -e[0])
    return out


def ctc_brute(lp: np.ndarray, T: int, hotwords, beta: float) -> List[tuple]:
    """All prefixes by ctc_align_ref.forward_loglik + Trie.bonus."""
    return _brute(lp.shape[1], T, lambda y: A.forward_loglik(lp, list(y), T), Trie(hotwords), beta)


def rnnt_brute(head, encp: np.ndarray, T: int, hotwords, beta: float, S: int = 1) -> List[tuple]:
    """All hypotheses of at most T S tokens by rnnt_beam_ref.exact_loglik + Trie.bonus."""
    pred = Predictor(head)
    e64 = np.asarray(encp, dtype=np.float64)
    joint = lambda t, y: joint_lp(head, e64[t], pred(tuple(y)))     # noqa: E731
    V = head["out_w"].shape[0]
    return _brute(V, T * S, lambda y: exact_loglik(joint, y, T, S), Trie(hotwords), beta)
