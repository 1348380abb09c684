"""The float64 resumable twin of gam_rnnt_beam_stream_kernel (gigaam_amd/csrc/gam_rnnt_beam_stream.h): the frame step of
tests/rnnt_beam_ref.py's contract run from a carried beam, call by call, with the kernel's refusals.

``new_record()`` -> a record that was not begun; ``call(head, rec, encp_rows, t_base, flags, W, S, hotwords, beta, lm)`` -> status
(1 accepted, 0 refused: the record is then unchanged); with END the record holds ``result``: ids, frames (stream frames), score,
logp, lm, beam, margins, final_margin as ``rnnt_beam_ref.beam_search`` returns them.  ``gens`` stands for the handle's hotword / LM
generations: a call whose pair differs from BEGIN's is refused, as after ``set_hotwords`` / ``set_lm``.

The float64 values carry no renormalisation and no rebase: none of them changes a real-number value.  ``rebase=period`` emulates the
kernel's BOOKKEEPING beside them -- `off` after every frame, cb_off / lm_off at every stream frame t > 0 that is a multiple of the
period -- and records in ``peak`` the largest magnitude any term of a rank reaches as the kernel holds it: score - off,
committed - cb_off, acc, lm - lm_off, over every entry of B, every candidate and every kept beam.  ``rebase=None``: the offsets of
the committed bonus and the LM term stay 0, which is the batch kernel's bookkeeping.  Used by the CPU and the GPU tests; do not
change a returned result."""
import numpy as np

import rnnt_beam_ref as R
from ctc_beam_ref import Trie

BEGIN, END = 1, 2
REBASE = 256              # gam_rnnt_beam.h GAM_RB_STREAM_REBASE
NEG = -np.inf


def new_record():
    return {"phase": "new"}


def _dims(head):
    return (int(head["out_w"].shape[0]), int(head["embed"].shape[1]), int(head["out_w"].shape[1]), len(head["lstm"]))


def call(head, rec, encp_rows, t_base, flags, W, S, hotwords=(), beta=2.0, lm=None, max_frames=2 ** 31 - 1, gens=(0, 0), rebase=None):
    n = 0 if encp_rows is None else len(encp_rows)
    begin = bool(flags & BEGIN)
    if not begin:
        if (rec.get("phase") != "begun" or rec["next"] != t_base or rec["cfg"] != (W, S) + _dims(head) or rec["gens"] != tuple(gens)
                or rec["max_frames"] > max_frames):
            return 0
        t0, max_frames = rec["t0"], rec["max_frames"]
    else:
        t0 = t_base
    if t_base + n - t0 > max_frames or t_base + n >= 2 ** 31:
        return 0
    if begin:
        lm0 = lm.start() if lm is not None else ((), (), 0.0)
        rec.clear()
        rec.update(cfg=(W, S) + _dims(head), gens=tuple(gens), t0=t0, max_frames=max_frames, pred=R.Predictor(head),
                   beam=[((), 0.0, (0, 0.0, 0.0), (), lm0)], margins=[], merges=0, off=0.0, cb_off=0.0, lm_off=0.0, peak=0.0)
    trie = Trie(hotwords)
    pred = rec["pred"]
    step = (lambda st, v: lm.step(st, v)) if lm is not None else (lambda st, v: st)     # noqa: E731
    margins = rec["margins"]
    beam = rec["beam"]

    def rank(sc, hw, ls):
        return sc + hw[2] + hw[1] + ls[2]

    def see(sc, hw, ls):
        if np.isfinite(sc):
            rec["peak"] = max(rec["peak"], abs(sc - rec["off"]), abs(hw[2] - rec["cb_off"]), abs(hw[1]), abs(ls[2] - rec["lm_off"]))

    for i in range(n):
        if not beam:
            break
        t = t_base + i
        et = np.asarray(encp_rows[i], dtype=np.float64)
        Bd = {}
        A = beam
        for s in range(S + 1):
            C = []
            for p, (y, sc, hw, fr, ls) in enumerate(A):
                if s < S:
                    lp = R.joint_lp(head, et, pred(y))
                    cands = [(sc + lp[-1], (s, p, 0))]
                    K = min(W, len(lp) - 1)
                    for v in R.topk_ids(lp, K):
                        hw2 = trie.step(hw, v, beta)
                        ls2 = step(ls, v)
                        sc2 = sc + lp[v]
                        see(sc2, hw2, ls2)
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
                        rec["merges"] += 1
                        e[0] = float(np.logaddexp(e[0], csc))
                        e[5] = min(e[5], abs(csc - e[1]))
                        if csc > e[1]:
                            e[1], e[4] = csc, fr
                    see(Bd[y][0], hw, ls)
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
        if beam:      # the kernel's bookkeeping: M = the best rank without its LM term leaves the scores; the rebase
            _, sc, hw, _, ls = beam[0]
            rec["off"] += (sc - rec["off"]) + (hw[2] - rec["cb_off"]) + hw[1]
            if rebase and t > 0 and t % rebase == 0:
                rec["cb_off"], rec["lm_off"] = hw[2], ls[2]
            for _, sc, hw, _, ls in beam:
                see(sc, hw, ls)
    rec["beam"] = beam
    rec["next"] = t_base + n
    rec["phase"] = "ended" if flags & END else "begun"
    if flags & END:
        rec["result"] = _final(rec, lm)
    return 1


def _final(rec, lm):
    beam = rec["beam"]
    if rec["next"] == rec["t0"]:      # a stream without a frame
        return {"ids": [], "frames": [], "score": 0.0, "logp": 0.0, "lm": 0.0, "beam": [], "margins": [], "final_margin": np.inf}
    if not beam:
        return {"ids": [], "frames": [], "score": NEG, "logp": NEG, "lm": 0.0, "beam": [], "margins": list(rec["margins"]),
                "final_margin": np.inf}
    finals = []
    for i, (_, sc, hw, _, ls) in enumerate(beam):
        lmf = lm.final(ls) if lm is not None else 0.0
        finals.append((sc + hw[2] + lmf, i, lmf))
    finals.sort(key=lambda e: (-e[0], e[1]))
    y, sc, hw, fr, _ = beam[finals[0][1]]
    return {"ids": list(y), "frames": list(fr), "score": sc + hw[2] + finals[0][2], "logp": sc, "lm": finals[0][2],
            "beam": [(b[0], b[1]) for b in beam], "states": [b[4] for b in beam], "margins": list(rec["margins"]), "merges": rec["merges"],
            "final_margin": float(finals[0][0] - finals[1][0]) if len(finals) > 1 else np.inf}


def stream(head, encp, cuts, W, S, hotwords=(), beta=2.0, lm=None, t0=0, end_alone=False, rebase=None):
    """The stream ``encp`` [T, JH] cut at the row numbers ``cuts`` (repeated numbers: empty calls) -> (result, record)."""
    edges = [0] + list(cuts) + [len(encp)]
    rec = new_record()
    for j, (a, b) in enumerate(zip(edges, edges[1:])):
        last = j == len(edges) - 2
        st = call(head, rec, encp[a:b], t0 + a, (BEGIN if j == 0 else 0) | (END if last and not end_alone else 0), W, S, hotwords, beta, lm,
                  rebase=rebase)
        assert st == 1, (cuts, j)
    if end_alone:
        assert call(head, rec, None, t0 + len(encp), END, W, S, hotwords, beta, lm, rebase=rebase) == 1
    return rec["result"], rec


# ---- the long-stream input of the rebase tests: head D, T = 2 periods + 40, W = 4, S = 3, six hotwords from the plain decode
LONG_T = 2 * REBASE + 40
LONG_W, LONG_S = 4, 3
LONG_KIND = "blank"
# kind -> the first seed, from 0 up, whose input qualifies (tests/test_rnnt_beam_stream_host.py finds them again); the LM of the LM case
# takes the first LM seed that qualifies on the "blank" input, 0
LONG_SEEDS = {"blank": 0, "dense": 0}
LONG_LM_SEED = 0


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def long_input(seed, kind=LONG_KIND):
    """(float64 head, encp [LONG_T, JH] float32, phrases) of a seed: encp = 3 N(0, 1) from default_rng([seed, 77])."""
    import rnnt_head_cases as HC
    hd = HC.head("D", 1, kind)[2]
    V, _, JH = HC.sizes("D")
    encp = (np.random.default_rng([seed, 77]).standard_normal((LONG_T, JH)) * HC.ENCP_SCALE).astype(np.float32)
    plain = R.beam_search(hd, encp.astype(np.float64), LONG_W, LONG_S)["ids"]
    return hd, encp, HC.hotwords(np.random.default_rng([seed, V]), [plain], V, 6)


def long_qualifies(hd, encp, phrases, lm=None):
    """(qualifies, margin, bar, peak, result) of one long-stream input: the float64 reference's smallest decision margin against
    bar = max(HC.MARGIN, 8 x the fp32 ulp at the largest term magnitude the rebase-emulating twin reports) -- two ranks are compared,
    each a sum of four rounded terms."""
    import rnnt_head_cases as HC
    res, rec = stream(hd, encp.astype(np.float64), [], LONG_W, LONG_S, phrases, HC.BETA, lm, rebase=REBASE)
    margin = R.min_margin(res)
    bar = max(HC.MARGIN, 8.0 * ulp32(rec["peak"]))
    return margin > bar, margin, bar, rec["peak"], res


def first_seed(limit=32, kind=LONG_KIND):
    """The first seed, from 0 up, whose long-stream input qualifies (the project's seed rule)."""
    for seed in range(limit):
        hd, encp, phrases = long_input(seed, kind)
        q = long_qualifies(hd, encp, phrases)
        if q[0]:
            return seed, q
    raise AssertionError(f"no seed below {limit} qualifies")


def long_lm(seed, hd, encp, lm_seed):
    """(ARPA text, LMSpec) of order 3 (beam_common.arpa through nbest_inputs.small_lm) over the words of the plain decode."""
    import beam_common as BC
    import nbest_inputs as I
    import rnnt_head_cases as HC
    plain = R.beam_search(hd, encp.astype(np.float64), LONG_W, LONG_S)["ids"]
    return I.small_lm(np.random.default_rng([lm_seed, seed, 78]), BC.tokenizer(HC.sizes("D")[0]), [plain], 3)
