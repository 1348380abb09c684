"""The seeded inputs tests/test_nbest_host.py (CPU) and tests/test_hip_nbest.py (GPU) share, so that the CPU file checks the references
on exactly what the GPU file runs.  numpy / torch on the CPU only."""
import itertools

import numpy as np

import beam_common as BC
import ctc_lm_ref as CL
import rnnt_beam_ref as RR

BETA = 1.5
LM_ALPHA, LM_BETA = 0.8, 0.6
_HEADS = {}


def rnnt_head(V, L=1, blank_bias=None):
    """(cfg, state dict, float64 head) of a synthetic RNN-T head with one encoder layer (as tests/test_hip_rnnt_beam.py builds it)."""
    key = (V, L, blank_bias)
    if key not in _HEADS:
        from gigaam_amd import synth
        cfg = synth.model_cfg("v3_e2e_rnnt" if V > 34 else "v2_rnnt", n_layers=1)
        cfg["head"]["decoder"]["num_classes"] = cfg["head"]["joint"]["num_classes"] = V
        cfg["head"]["decoder"]["pred_rnn_layers"] = L
        sd = synth.make_state_dict(cfg, seed=V + L, rnnt_blank_bias=blank_bias)
        _HEADS[key] = (cfg, sd, RR.head_from_state_dict(sd, L))
    return _HEADS[key]


def small_lm(rng, tok, id_lists, order=3):
    """(ARPA text, LMSpec) of a small LM (beam_common.arpa) over the words of ``id_lists`` and some random ones."""
    from gigaam_amd import lm as LM
    classes = [int(c) for c in LM.token_classes(tok)]
    V = len(classes)
    start = [c for c in range(V - 1) if classes[c] == 1]
    cont = [c for c in range(V - 1) if classes[c] == 0]
    cands = [w for ids in id_lists for w in CL.words_of(ids, classes)]
    for _ in range(30):
        k = int(rng.integers(0, 3))
        cands.append(tuple(([int(rng.choice(start))] if start else [int(rng.choice(cont))]) + [int(rng.choice(cont)) for _ in range(k)]))
    spell = {}
    for ids in cands:
        text = tok.decode(list(ids))
        w = text[1:] if text.startswith("▁") else text
        if w and w not in spell.values() and " " not in w and LM.word_spelling(tok, w, classes) == list(ids):
            spell[tuple(ids)] = w
    sents = [[spell[w] for w in CL.words_of(ids, classes) if w in spell] for ids in id_lists]
    text = BC.arpa(rng, sorted(spell.values()), order, [s for s in sents if s])
    return text, CL.LMSpec(CL.ArpaLM(text), classes, spell, LM_ALPHA, LM_BETA)


def _greedy_ids(lp, T):
    lab = np.argmax(lp[:T], axis=1).tolist()
    V = lp.shape[1]
    return [v for i, v in enumerate(lab) if v != V - 1 and (i == 0 or v != lab[i - 1])]


# ---- GPU test 1 (hypothesis 0 is the 1-best result): plain, 8 hotwords, a small LM
def ctc_hyp0_inputs(V):
    """{variant: (lp [6, 43, V], enc_len, phrases, (ARPA text, LMSpec) or None)}."""
    rng = np.random.default_rng(1000 + V)
    T, B = 40, 6
    enc_len = [T, T - 5, T, 1, T, T + 3]
    out = {}
    for variant in ("plain", "hotwords", "lm"):
        lp = BC.log_probs(rng, B, T + 3, V, "flat" if variant == "lm" else "peaked")
        phrases = BC.ctc_hotwords(rng, lp, 8) if variant == "hotwords" else []
        lm = small_lm(rng, BC.tokenizer(V), [_greedy_ids(lp[b], enc_len[b]) for b in range(B)]) if variant == "lm" else None
        out[variant] = (lp, enc_len, phrases, lm)
    return out


def rnnt_hyp0_inputs(V):
    """{variant: (encp [4, 10, JH], enc_len, phrases, (ARPA text, LMSpec) or None)} for the head rnnt_head(V)."""
    cfg, _, head = rnnt_head(V)
    JH = cfg["head"]["joint"]["joint_hidden"]
    rng = np.random.default_rng(2000 + V)
    T, B = 10, 4
    enc_len = [T, T - 3, 1, T]
    out = {}
    for variant in ("plain", "hotwords", "lm"):
        encp = BC.encp(rng, B, T, JH, 1.0)
        plain = [RR.beam_search(head, encp[b].astype(np.float64), 4, 3, enc_len[b])["ids"] for b in range(B)]
        phrases = []
        if variant == "hotwords":
            phrases = [p[i:i + 2] for p in plain for i in range(0, max(len(p) - 1, 0), 2)][:6]
            phrases += [[int(c) for c in rng.integers(0, V - 1, 2)] for _ in range(8 - len(phrases))]
        lm = small_lm(rng, BC.tokenizer(V), plain) if variant == "lm" else None
        out[variant] = (encp, enc_len, phrases, lm)
    return out


# ---- GPU test 2 (exact top-N when nothing is pruned): V = 3, T' <= 4
EXACT_HOTWORDS = ([], [[0, 1]], [[1], [0, 0, 1]])
EXACT_BETA = 1.25


def ctc_exact_inputs():
    """[(hotwords, lp [16, 4, 3], enc_len)]."""
    rng = np.random.default_rng(21)
    V, Tp, B = 3, 4, 16
    return [(hot, np.log(rng.dirichlet(np.ones(V) * 0.7, size=(B, Tp))).astype(np.float32), [1 + b % Tp for b in range(B)])
            for hot in EXACT_HOTWORDS]


def rnnt_exact_inputs():
    """[(hotwords, encp [16, 4, JH], enc_len)] for the head rnnt_head(3, 1, 0.0)."""
    cfg, _, _ = rnnt_head(3, 1, 0.0)
    JH = cfg["head"]["joint"]["joint_hidden"]
    rng = np.random.default_rng(21)
    B, Tp = 16, 4
    return [(hot, BC.encp(rng, B, Tp, JH, 0.5), [1 + b % Tp for b in range(B)]) for hot in EXACT_HOTWORDS]


# ---- GPU test 3 (against the float64 N-best reference, N = W): the seeds, shapes and generators of the 1-best tests
#      test_op_beam_matches_float64_reference
CTC_REF_SETS = [(V, kind) for V in (34, 257, 1025) for kind in ("peaked", "flat")]
RNNT_REF_SETS = [(34, "blank", 1), (34, "dense", 1), (257, "dense", 2)]


def ctc_ref_inputs(V, kind):
    """[(W, lp [6, T + 3, V], enc_len, phrases)]: W in {1, 4, 8, 32}, without and with 8 hotwords."""
    rng = np.random.default_rng(V * 3 + (1 if kind == "flat" else 0))
    T = 24 if kind == "flat" else 40
    B = 6
    out = []
    for W in (1, 4, 8, 32):
        for hot in (False, True):
            lp = BC.log_probs(rng, B, T + 3, V, kind)
            out.append((W, lp, [T, T - 5, T, 1, T, T + 3], BC.ctc_hotwords(rng, lp, 8) if hot else []))
    return out


def rnnt_ref_inputs(V, kind, L):
    """[(W, S, encp [4, T, JH], enc_len)] for the head rnnt_head(V, L, 14.0 if blank else None); no hotwords."""
    cfg, _, _ = rnnt_head(V, L, 14.0 if kind == "blank" else None)
    JH = cfg["head"]["joint"]["joint_hidden"]
    rng = np.random.default_rng(V * 7 + L + (1 if kind == "dense" else 0))
    B = 4
    out = []
    for W, S in itertools.product((1, 4, 8, 32), (1, 3, 10)):
        T = 10 if W >= 8 else 20
        out.append((W, S, BC.encp(rng, B, T, JH, 1.0), [T, T - 3, 1, T]))
    return out
