"""Float64 reference of RNN-T beam search with hotword boosting (gigaam_amd/csrc/gam_rnnt_beam.h holds the contract).  Hypotheses
are real token tuples here (the kernel identifies them by length and a 64-bit hash); the predictor and the joint are the oracle's
lstm_step / rnnt_joint math in float64.  Used by the CPU and the GPU tests.

Per frame t: B = {}, A_0 = the beam.  For s = 0 .. S: every a in A_s (position p) gives, when s < S, lp = lp(t, a.y), its blank
candidate (a.y, a.score + lp[blank], key (s, p, 0)) merged into B, and for the top-K non-blank ids v of lp (ties to the lower id) the
extension (a.y + v, a.score + lp[v], key (s, p, v + 1)) into C_s; when s = S, the forced advance (a.y, a.score, key (S, p, 0)) into B.
theta = the W-th highest rank in B (-inf while |B| < W); A_{s+1} = top W of {c in C_s: rank > theta} (ties: smaller key); the frame
ends when it is empty.  The new beam is the top W of B.  Merging in B log-add-exps the scores; the entry keeps the frames of the
contributor with the higher score (ties: the earlier one) and the key of its first contributor.  rank = score + committed + acc.
Final: best score + committed, ties to the lower beam position.
With ``lm`` (a ctc_lm_ref.LMSpec, where the word rules are): an extension a.y + v takes ``lm.step(state, v)``; blank candidates and
the forced advance keep the state; equal y means equal state (asserted at every merge); rank and the final pick add the LM term
(final: ``lm.final(state)``, the last word and </s>).  score = log p + committed + that term; logp = log p.
``greedy_trace`` / ``greedy_ref``: the greedy decode over the same predictor and joint (the tests of gam_rnnt_greedy)."""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ctc_beam_ref import Trie

NEG = -np.inf


def head_from_state_dict(sd, n_layers: Optional[int] = None) -> Dict[str, object]:
    """The RNN-T head's weights as float64 numpy arrays (checkpoint key names)."""
    def g(k):
        v = sd[k]
        return np.asarray(v.detach().double().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64)
    if n_layers is None:
        n_layers = sum(1 for k in sd if k.startswith("head.decoder.lstm.weight_ih_l"))
    p = "head.decoder.lstm."
    return {
        "embed": g("head.decoder.embed.weight"),
        "lstm": [(g(f"{p}weight_ih_l{l}"), g(f"{p}weight_hh_l{l}"), g(f"{p}bias_ih_l{l}") + g(f"{p}bias_hh_l{l}")) for l in range(n_layers)],
        "enc_w": g("head.joint.enc.weight"), "enc_b": g("head.joint.enc.bias"),
        "pred_w": g("head.joint.pred.weight"), "pred_b": g("head.joint.pred.bias"),
        "out_w": g("head.joint.joint_net.1.weight"), "out_b": g("head.joint.joint_net.1.bias"),
    }


def encoder_projection(head, encoded) -> np.ndarray:
    """encoded [D, T'] (one utterance, channel-first) -> encp [T', JH] = W_enc f + b_enc."""
    f = np.asarray(encoded, dtype=np.float64).T
    return f @ head["enc_w"].T + head["enc_b"]


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


class Predictor:
    """pp(y) = W_pred g(y) + b_pred with the LSTM state after feeding y, cached per y (the empty y: predict(None, None))."""

    def __init__(self, head):
        self.head = head
        self.cache: Dict[tuple, Tuple[np.ndarray, list]] = {}

    def __call__(self, y: tuple) -> np.ndarray:
        return self._get(y)[0]

    def _get(self, y: tuple):
        if y in self.cache:
            return self.cache[y]
        hd = self.head
        H = hd["embed"].shape[1]
        if y:
            _, st = self._get(y[:-1])
            x = hd["embed"][y[-1]]
        else:
            st = [(np.zeros(H), np.zeros(H)) for _ in hd["lstm"]]
            x = np.zeros(H)
        new = []
        for (wi, wh, bias), (h, c) in zip(hd["lstm"], st):
            gates = wi @ x + wh @ h + bias
            i, f, gg, o = np.split(gates, 4)
            c2 = _sig(f) * c + _sig(i) * np.tanh(gg)
            h2 = _sig(o) * np.tanh(c2)
            new.append((h2, c2))
            x = h2
        pp = hd["pred_w"] @ x + hd["pred_b"]
        self.cache[y] = (pp, new)
        return self.cache[y]


def joint_lp(head, encp_t: np.ndarray, pp: np.ndarray) -> np.ndarray:
    z = np.maximum(encp_t + pp, 0.0) @ head["out_w"].T + head["out_b"]
    m = z.max()
    return z - (m + np.log(np.exp(z - m).sum()))


def topk_ids(lp: np.ndarray, k: int) -> List[int]:
    v = lp[:-1]
    order = np.lexsort((np.arange(len(v)), -v))
    return [int(i) for i in order[:k]]


def beam_search(head, encp, W: int, S: int, T: Optional[int] = None, hotwords: Sequence[Sequence[int]] = (),
                beta: float = 2.0, joint=None, lm=None) -> Dict[str, object]:
    """encp [>= T, JH] (float64: W_enc f + b_enc), beam width W, max symbols per frame S.  ``joint(t, y) -> lp`` replaces the
    network's joint when given (tests with hand-made log-probs).  ``lm``: a ctc_lm_ref.LMSpec or None (its term is then an exact
    + 0.0).  Returns ids, frames, score (log p + committed bonus + LM term), logp, lm (the picked hypothesis's final LM term), beam
    (the final [(y, score)]), states (the final beam's LM states), margins (every top-W cut, theta comparison and kept merge),
    merges (how many merges in B the search made, each with equal LM states) and final_margin."""
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


def min_margin(res: Dict[str, object]) -> float:
    """The smallest decision margin of a run: every cut, theta comparison, kept merge and the final pick."""
    return float(min([res["final_margin"]] + list(res["margins"])))


def greedy_trace(head, encoded, T: int, S: int) -> Dict[str, object]:
    """The float64 greedy decode of one utterance (reference decoding.py's loop: at most S symbols per frame, the first maximum
    wins) with everything it saw: ``ids``, ``frames``, ``margin`` (the smallest top-1 / top-2 margin over its joint steps, inf when
    there was none), ``lp`` [joint steps, V] (the log-probs of every joint evaluation, in decode order), ``per_frame`` [T] (tokens
    emitted at each frame)."""
    encp = encoder_projection(head, encoded)
    pred = Predictor(head)
    blank = head["out_w"].shape[0] - 1
    y, frames, margin, rows, per_frame = (), [], np.inf, [], [0] * T
    for t in range(T):
        for _ in range(S):
            lp = joint_lp(head, encp[t], pred(y))
            rows.append(lp)
            k = int(np.argmax(lp))
            top2 = np.partition(lp, -2)[-2:]
            margin = min(margin, float(top2[1] - top2[0]))
            if k == blank:
                break
            y += (k,)
            frames.append(t)
            per_frame[t] += 1
    lp = np.stack(rows) if rows else np.zeros((0, blank + 1))
    return {"ids": list(y), "frames": frames, "margin": margin, "lp": lp, "per_frame": per_frame}


def greedy_ref(head, encoded, T: int, S: int) -> Tuple[List[int], List[int], float]:
    """(ids, frames, smallest top-1 / top-2 margin) of ``greedy_trace``."""
    r = greedy_trace(head, encoded, T, S)
    return r["ids"], r["frames"], r["margin"]


def exact_loglik(joint, y: Sequence[int], T: int, S: int) -> float:
    """log P_S(y | x): every alignment of y over T frames with at most S symbols per frame; after S symbols the frame advances
    without a joint (probability 1).  ``joint(t, prefix) -> lp``.  DP over (t, u, symbols emitted in frame t)."""
    y = tuple(int(v) for v in y)
    U = len(y)
    a = {(0, 0, 0): 0.0}
    for t in range(T):
        nxt: Dict[tuple, float] = {}
        for k in range(S + 1):
            for u in range(U + 1):
                v = a.get((t, u, k))
                if v is None:
                    continue
                if k == S:
                    nxt[(t + 1, u, 0)] = float(np.logaddexp(nxt.get((t + 1, u, 0), NEG), v))
                    continue
                lp = joint(t, y[:u])
                nxt[(t + 1, u, 0)] = float(np.logaddexp(nxt.get((t + 1, u, 0), NEG), v + lp[-1]))
                if u < U:
                    a[(t, u + 1, k + 1)] = float(np.logaddexp(a.get((t, u + 1, k + 1), NEG), v + lp[y[u]]))
        a.update(nxt)
    return a.get((T, U, 0), NEG)
