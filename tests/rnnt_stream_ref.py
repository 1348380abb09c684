"""Float64 twin of the resumable RNN-T greedy decode (gigaam_amd/csrc/gam_rnnt_stream.h holds the contract): one stream fed in
pieces, the state carried from call to call in a record that holds EXACTLY the fields of the kernel's -- begun and ended marks, the
next frame, the token count, the last label, max_symbols, V / H / JH / L and the committed (h, c) of every predictor layer.  The
candidate state, W_pred g and the symbols emitted on the current frame are no part of it: a call recomputes the first two from the
record, and ends only when its last frame has ended.  The predictor and the joint are tests/rnnt_beam_ref.py's float64 math.  Used by
the CPU test (every cut of every utterance equals ``R.greedy_trace``) and by the GPU tests (what a refused call must leave alone)."""
from typing import Dict, List, Optional

import numpy as np

import rnnt_beam_ref as R
import rnnt_cluster_cases as K

BEGIN, END = 1, 2
FIELDS = ("begun", "ended", "next", "count", "label", "max_symbols", "V", "H", "JH", "L", "hc")


def new_record() -> Dict[str, object]:
    """A record that was never begun (the zeros of a fresh buffer)."""
    return {"begun": False, "ended": False, "next": 0, "count": 0, "label": None, "max_symbols": 0, "V": 0, "H": 0, "JH": 0, "L": 0,
            "hc": []}


def _sizes(head):
    return head["out_w"].shape[0], head["embed"].shape[1], head["enc_w"].shape[0], len(head["lstm"])


def _predict(head, label: Optional[int], hc):
    """One predictor step from the committed state: (pp = W_pred g + b_pred, the candidate [(h', c')])."""
    H = head["embed"].shape[1]
    x = np.zeros(H) if label is None else head["embed"][label]
    new = []
    for (wi, wh, bias), (h, c) in zip(head["lstm"], hc):
        i, f, g, o = np.split(wi @ x + wh @ h + bias, 4)
        c2 = R._sig(f) * c + R._sig(i) * np.tanh(g)
        h2 = R._sig(o) * np.tanh(c2)
        new.append((h2, c2))
        x = h2
    return head["pred_w"] @ x + head["pred_b"], new


def call(head, rec: Dict[str, object], encp, t_base: int, flags: int, S: int, ids: List[int], frames: List[int], cap: int) -> int:
    """One call of the stream: rows ``encp`` [n, JH] (float64) are stream frames t_base ..; token k goes to ids[k] / frames[k] (lists
    of ``cap`` entries, written in place).  Returns the status: 1 accepted (``rec`` updated), 0 refused (nothing touched)."""
    V, H, JH, L = _sizes(head)
    n = 0 if encp is None else int(encp.shape[0])
    if flags & BEGIN:
        count, label, hc = 0, None, [(np.zeros(H), np.zeros(H)) for _ in range(L)]
    else:
        if not (rec["begun"] and not rec["ended"] and rec["next"] == t_base
                and (rec["max_symbols"], rec["V"], rec["H"], rec["JH"], rec["L"]) == (S, V, H, JH, L)):
            return 0
        count, label, hc = rec["count"], rec["label"], rec["hc"]
    if count + n * S > cap:
        return 0
    blank = V - 1
    cand = None          # (pp, candidate state) of the committed state: recomputed by every call, never carried
    for i in range(n):
        for _ in range(S):
            if cand is None:
                cand = _predict(head, label, hc)
            lp = R.joint_lp(head, encp[i], cand[0])
            k = int(np.argmax(lp))
            if k == blank:
                break
            ids[count], frames[count] = k, t_base + i
            count += 1
            label, hc, cand = k, cand[1], None
        # the frame has ended, by a blank or at max_symbols: no symbol count is left to carry
    rec.update(begun=True, ended=bool(flags & END), next=t_base + n, count=count, label=label, max_symbols=S, V=V, H=H, JH=JH, L=L,
               hc=hc)
    assert set(rec) == set(FIELDS)
    return 1


def decode_cut(head, encoded, T: int, S: int, cuts) -> Dict[str, object]:
    """Utterance ``encoded`` [D, >= T] as a stream cut at the frames ``cuts`` (ascending, within [0, T]): BEGIN on the first call, END
    on the last.  Returns ids, frames and ``counts`` (the token count after every call)."""
    encp = R.encoder_projection(head, encoded)[:T]
    edges = [0] + list(cuts) + [T]
    ids, frames, rec, counts = [0] * (T * S), [0] * (T * S), new_record(), []
    for j, (a, b) in enumerate(zip(edges, edges[1:])):
        flags = (BEGIN if j == 0 else 0) | (END if j == len(edges) - 2 else 0)
        assert call(head, rec, encp[a:b], a, flags, S, ids, frames, T * S) == 1
        counts.append(rec["count"])
    return {"ids": ids[:rec["count"]], "frames": frames[:rec["count"]], "counts": counts}


# ---- head C with two predictor layers on the cluster matrix's batch of head C (tests/rnnt_cluster_cases.py): the seed and the blank
# bias are head C's own
def l2_inputs():
    """(cfg, state dict, encoded [6, d_model, 60], lengths) of head C at L = 2."""
    from gigaam_amd import synth
    _, _, encoded, lengths = K.inputs("C")
    cfg = K.head_cfg("C")
    cfg["head"]["decoder"]["pred_rnn_layers"] = 2
    return cfg, synth.make_state_dict(cfg, seed=K.HEADS["C"][3], rnnt_blank_bias=K.HEADS["C"][4]), encoded, lengths


_L2 = {}


def l2_case():
    """(cfg, state dict, encoded, lengths, the float64 greedy traces of the six utterances); computed once, not to be changed."""
    if not _L2:
        cfg, sd, encoded, lengths = l2_inputs()
        head = R.head_from_state_dict(sd, 2)
        _L2["case"] = (cfg, sd, encoded, lengths, [R.greedy_trace(head, encoded[b], T, K.MAX_SYMBOLS) for b, T in enumerate(lengths)])
    return _L2["case"]
