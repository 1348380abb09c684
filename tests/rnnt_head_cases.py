"""The inputs tests/test_rnnt_head_cases_host.py (CPU) and tests/test_hip_rnnt_head_matrix.py / test_hip_rnnt_head_conf_align.py
(GPU) share: RNN-T beam search (plain, LM, N-best, LM + N-best), confidence, joint and predictor on the six heads of
tests/rnnt_cluster_cases.py -- sizes other than pred_hidden = joint_hidden = 320, where gam_rnnt_beam.h's union region, wave-tile loops
and row-tile switch, gam_confidence.h's class-tile groups and the K of the pp / joint GEMMs take paths that 320 / 320 never runs.

One state dict per (head, L, kind): kind "blank" (blank bias 14, blank-dominant) or "dense" (the synthetic default, emission-heavy), as
tests/test_hip_rnnt_beam.py builds them.  The input seed of every set was picked on the CPU with the float64 references alone
(tests/rnnt_beam_ref.py, tests/nbest_ref.py): the first seed at which at least 90 % of the set's utterances have a decision margin
above MARGIN.

The float64 searches of the emission-heavy sets take up to 20 s a set on a head of 512 hidden units, so the GPU tests do not run
them: ``compute_*`` run the references, tests/golden/make_rnnt_head_refs.py stores what they return in
tests/golden/rnnt_head_refs.npz, ``*_cases`` read that file and add the seeded encp.  The host test runs ``compute_*`` again,
compares with the file and asserts the share of qualifying utterances on what it computed.  Do not change a returned object."""
import functools
import gzip
import json
import os

import numpy as np

import beam_common as BC
import nbest_inputs as I
import nbest_ref as N
import rnnt_beam_ref as R
import rnnt_cluster_cases as K

MARGIN = 1e-4             # tests/test_hip_rnnt_beam.py MARGIN (op level); N.RNNT_MARGIN is the same figure
BLANK_BIAS = 14.0         # kind "blank"
BETA = 1.5                # hotword boost
T, B = 10, 4
# encp = ENCP_SCALE x standard normal (beam_common.encp).  The encoder projection of these synthetic heads has an rms of 4.6 on the
# cluster matrix's batches; at scale 1 every search on them -- both kinds -- ends in the empty transcript, so that only pp(()) and the
# blank column would decide the compared values.  At 3 the "dense" sets emit more tokens than they have frames and the "blank" sets a
# few (the host test asserts both), so the predictor's label steps, the hidden rows and the slot pool decide ids and scores.
ENCP_SCALE = 3.0
ENC_LEN = [T, T - 3, 1, T]
KINDS = ("blank", "dense")
HEAD_L = [(name, 1) for name in sorted(K.HEADS)] + [("A", 2), ("C", 2), ("E", 2)]
WS = [(1, 3), (4, 1), (8, 3), (16, 3), (17, 2), (32, 10)]
WS_EDGE = (32, 16)        # A at L = 2: the largest accepted configuration (161296 of the 163840 bytes of LDS)
# with the LM: (W, S, LM order); S = 3 at W = 32 because A at L = 2 with the LM's carve does not fit beyond it
LM_WS = [(1, 3, 2), (4, 1, 3), (8, 3, 4), (16, 3, 5), (17, 2, 3), (32, 3, 2)]
LM_SETS = [("C", 1), ("E", 1), ("A", 2)]          # kind "dense"
NBEST_SETS = [("C", 1), ("E", 1), ("F", 1)]       # kind "dense", n_best = W, without and with the LM
LDS_LIMIT = 160 * 1024
REFS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rnnt_head_refs.npz")
PARTS = {"beam": 1, "lm": 2, "nbest": 3, "nbest_lm": 4}

# (part, head, L, kind) -> input seed; a set not listed takes 0.  Picked by the rule in the module docstring.
SEEDS = {
    ("beam", "A", 2, "dense"): 18, ("beam", "C", 2, "blank"): 1, ("beam", "D", 1, "dense"): 1, ("beam", "E", 2, "dense"): 9,
    ("beam", "F", 1, "dense"): 5, ("lm", "C", 1, "dense"): 1, ("nbest", "E", 1, "dense"): 8, ("nbest", "F", 1, "dense"): 11,
    ("nbest_lm", "C", 1, "dense"): 2, ("nbest_lm", "E", 1, "dense"): 1, ("nbest_lm", "F", 1, "dense"): 1,
}


def combos(name, L):
    return WS + ([WS_EDGE] if (name, L) == ("A", 2) else [])


def seed_of(part, name, L, kind):
    return SEEDS.get((part, name, L, kind), 0)


@functools.lru_cache(maxsize=None)
def head(name, L, kind):
    """(cfg, state dict, float64 head) of a head of tests/rnnt_cluster_cases.py with L predictor layers."""
    from gigaam_amd import synth
    cfg = K.head_cfg(name)
    cfg["head"]["decoder"]["pred_rnn_layers"] = L
    sd = synth.make_state_dict(cfg, seed=K.HEADS[name][3] + 10 * L, rnnt_blank_bias=BLANK_BIAS if kind == "blank" else None)
    return cfg, sd, R.head_from_state_dict(sd, L)


def sizes(name):
    """(V, H, JH)."""
    return K.HEADS[name][:3]


def encp_of(part, name, L, kind, i, seed=None):
    """encp [4, T, JH] float32 of combination i of a set."""
    seed = seed_of(part, name, L, kind) if seed is None else seed
    return BC.encp(np.random.default_rng([seed, PARTS[part], i]), B, T, sizes(name)[2], ENCP_SCALE)


def hotwords(rng, res_ids, V, n):
    """n phrases of 1-3 tokens: runs of tokens the reference emitted (phrases the beam meets), padded with random ones
    (tests/test_hip_rnnt_beam.py _hotwords)."""
    out = []
    for _ in range(n):
        ids = res_ids[int(rng.integers(0, len(res_ids)))] if res_ids else []
        if len(ids) >= 2:
            i = int(rng.integers(0, len(ids) - 1))
            out.append([int(c) for c in ids[i:i + int(rng.integers(1, 4))]])
        else:
            out.append([int(c) for c in rng.integers(0, V - 1, int(rng.integers(1, 3)))])
    return out


def trie_words(phrases):
    """Words of the hotword trie as gam_set_hotwords lays it out: node offsets [nodes + 1] and one word per edge."""
    nodes = {()}
    for p in phrases:
        for i in range(1, len(p) + 1):
            nodes.add(tuple(p[:i]))
    return 2 * len(nodes)


def _plain_ids(hd, encp, W, S):
    return [R.beam_search(hd, encp[b].astype(np.float64), W, S, ENC_LEN[b])["ids"] for b in range(B)]


def _one(ref):
    """What the tests read of a 1-best reference run; ``margin``: its smallest decision margin (R.min_margin)."""
    return {"ids": [int(v) for v in ref["ids"]], "frames": [int(v) for v in ref["frames"]], "score": float(ref["score"]),
            "logp": float(ref["logp"]), "margin": float(R.min_margin(ref))}


def _many(ref, W):
    """What the tests read of an N-best reference run; ``qualifies``: N.qualifies at n_best = W and the op-level margin."""
    return {"hyps": [{"ids": [int(v) for v in h["ids"]], "frames": [int(v) for v in h["frames"]], "score": float(h["score"]),
                      "logp": float(h["logp"])} for h in ref["hyps"]], "qualifies": bool(N.qualifies(ref, W, N.RNNT_MARGIN))}


# ---- 1. the plain kernel: every head, L and kind; hotwords on every second combination
def compute_beam(name, L, kind, seed=None):
    """[{phrases, refs [4]}] over combos(name, L), by R.beam_search."""
    V = sizes(name)[0]
    hd = head(name, L, kind)[2]
    out = []
    for i, (W, S) in enumerate(combos(name, L)):
        encp = encp_of("beam", name, L, kind, i, seed)
        phrases = hotwords(np.random.default_rng([i, V]), _plain_ids(hd, encp, W, S), V, 6) if i % 2 == 1 else []
        out.append({"phrases": phrases,
                    "refs": [_one(R.beam_search(hd, encp[b].astype(np.float64), W, S, ENC_LEN[b], phrases, BETA)) for b in range(B)]})
    return out


# ---- 2. the LM kernel: LM_SETS, kind "dense"; hotwords on every second combination
def compute_lm(name, L, seed=None):
    """[{phrases, arpa (text), refs [4]}] over LM_WS, by R.beam_search with an LMSpec; the LM's words and sentences come from the
    search without LM, so its lookups hit every order (tests/test_hip_rnnt_beam_lm.py; weights nbest_inputs.LM_ALPHA / LM_BETA)."""
    V = sizes(name)[0]
    hd = head(name, L, "dense")[2]
    tok = BC.tokenizer(V)
    out = []
    for i, (W, S, order) in enumerate(LM_WS):
        encp = encp_of("lm", name, L, "dense", i, seed)
        plain = _plain_ids(hd, encp, W, S)
        text, spec = I.small_lm(np.random.default_rng([i, V, 2]), tok, plain, order)
        phrases = [p[:3] for p in plain if p][:4] if i % 2 == 1 else []
        out.append({"phrases": phrases, "arpa": text,
                    "refs": [_one(R.beam_search(hd, encp[b].astype(np.float64), W, S, ENC_LEN[b], phrases, BETA, lm=spec)) for b in range(B)]})
    return out


# ---- 3. the N-best kernels: NBEST_SETS, kind "dense", n_best = W, no hotwords
def compute_nbest(name, L, with_lm, seed=None):
    """[{arpa (None without the LM), refs [4]}] over WS, by N.rnnt_nbest."""
    V = sizes(name)[0]
    hd = head(name, L, "dense")[2]
    tok = BC.tokenizer(V)
    part = "nbest_lm" if with_lm else "nbest"
    out = []
    for i, (W, S) in enumerate(WS):
        encp = encp_of(part, name, L, "dense", i, seed)
        text, spec = I.small_lm(np.random.default_rng([i, V, 4]), tok, _plain_ids(hd, encp, W, S), 2 + i % 4) if with_lm else (None, None)
        out.append({"arpa": text, "refs": [_many(N.rnnt_nbest(hd, encp[b].astype(np.float64), W, S, ENC_LEN[b], lm=spec), W) for b in range(B)]})
    return out


# ---- 4. the LDS edge: A at L = 2, (32, 16), with a hotword trie that fits in LDS beside it and one that does not
HW_LDS_WORDS = (LDS_LIMIT - 161296) // 4        # 636: the words left beside the kernel's own carve
# the blank-dominant head: at S = 16 an emission-heavy search takes thousands of decisions per utterance and too few utterances keep
# every one of them above the margin; the boosted phrases make this one emit.  The phrase seed was picked like the input seeds.
EDGE_KIND = "blank"
EDGE_SEED = 7


def compute_edge(base_refs):
    """[{phrases, refs [4]}]: the (32, 16) combination of the ("A", 2, EDGE_KIND) beam set with 6 phrases from its reference's ids
    (``base_refs``), then with 1024 phrases of three tokens (a trie the kernel reads from global memory), the first six among them."""
    W, S = WS_EDGE
    i = combos("A", 2).index(WS_EDGE)
    hd = head("A", 2, EDGE_KIND)[2]
    V = sizes("A")[0]
    encp = encp_of("beam", "A", 2, EDGE_KIND, i)
    rng = np.random.default_rng(EDGE_SEED)
    small = hotwords(rng, [r["ids"] for r in base_refs], V, 6)
    big = small + [[int(c) for c in rng.integers(0, V - 1, 3)] for _ in range(1024 - len(small))]
    return [{"phrases": phrases,
             "refs": [_one(R.beam_search(hd, encp[b].astype(np.float64), W, S, ENC_LEN[b], phrases, BETA)) for b in range(B)]}
            for phrases in (small, big)]


# ---- the stored references
def set_key(part, name, L, kind="dense"):
    return f"{part}/{name}/{L}/{kind}"


def all_sets():
    """[(part, head, L, kind)] of every stored set but the edge."""
    return ([("beam", n, L, k) for n, L in HEAD_L for k in KINDS] + [("lm", n, L, "dense") for n, L in LM_SETS] +
            [(p, n, L, "dense") for n, L in NBEST_SETS for p in ("nbest", "nbest_lm")])


def compute_set(part, name, L, kind, seed=None):
    if part == "beam":
        return compute_beam(name, L, kind, seed)
    return compute_lm(name, L, seed) if part == "lm" else compute_nbest(name, L, part == "nbest_lm", seed)


def write_refs(data, path=REFS_PATH):
    """{set_key: cases, "edge": cases} as gzipped JSON inside an .npz (tests/golden/make_rnnt_head_refs.py)."""
    raw = gzip.compress(json.dumps(data, sort_keys=True).encode("utf-8"), mtime=0)
    np.savez(path, refs=np.frombuffer(raw, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def stored_refs():
    with np.load(REFS_PATH) as z:
        return json.loads(gzip.decompress(z["refs"].tobytes()).decode("utf-8"))


def _with_inputs(part, name, L, kind, cases):
    ws = LM_WS if part == "lm" else (combos(name, L) if part == "beam" else WS)
    assert len(cases) == len(ws), (part, name, L, kind)
    return [dict(c, W=ws[i][0], S=ws[i][1], encp=encp_of(part, name, L, kind, i)) for i, c in enumerate(cases)]


@functools.lru_cache(maxsize=None)
def beam_cases(name, L, kind):
    """[{W, S, encp, phrases, refs [4] of {ids, frames, score, logp, margin}}] over combos(name, L)."""
    return _with_inputs("beam", name, L, kind, stored_refs()[set_key("beam", name, L, kind)])


@functools.lru_cache(maxsize=None)
def lm_cases(name, L):
    """[{W, S, encp, phrases, arpa, refs [4]}] over LM_WS."""
    return _with_inputs("lm", name, L, "dense", stored_refs()[set_key("lm", name, L)])


@functools.lru_cache(maxsize=None)
def nbest_cases(name, L, with_lm):
    """[{W, S, encp, arpa, refs [4] of {hyps [{ids, frames, score, logp}], qualifies}}] over WS."""
    part = "nbest_lm" if with_lm else "nbest"
    return _with_inputs(part, name, L, "dense", stored_refs()[set_key(part, name, L)])


@functools.lru_cache(maxsize=None)
def edge_cases():
    i = combos("A", 2).index(WS_EDGE)
    return [dict(c, W=WS_EDGE[0], S=WS_EDGE[1], encp=encp_of("beam", "A", 2, EDGE_KIND, i)) for c in stored_refs()["edge"]]


def margin_of(ref):
    return ref["margin"]


def share(cases, nbest=False):
    """(qualifying, all) utterances of a list of cases (stored or computed)."""
    ok = n = 0
    for c in cases:
        for ref in c["refs"]:
            ok += bool(ref["qualifies"] if nbest else ref["margin"] > MARGIN)
            n += 1
    return ok, n


# ---- 5. the kernel's LDS carve, transcribed (gam_rnnt_beam.h gam_rb_fixed_bytes / gam_rb_union_bytes / gam_rb_lm_bytes)
def _up16(x):
    return (x + 15) & ~15


def rb_fixed_bytes(W, S):
    P = (S + 1) * W
    return _up16(2 * 32 * 8 + 2 * 32 * 9 * 4 + 32 * 4 + 16 * 4 + P * 8 + P * 9 * 4 + P * 4 + ((P + 31) // 32) * 4)


def rb_union_members(W, Kc, H, JH, L):
    """Bytes of the three members of the union region: (joint rows, candidates, hidden rows)."""
    Wp = (W + 15) // 16 * 16
    return Wp * (JH + 4) * 4, W * Kc * (8 + 4 * 4), (2 if L > 1 else 1) * Wp * (H + 4) * 4


def rb_union_bytes(W, Kc, H, JH, L):
    return _up16(max(rb_union_members(W, Kc, H, JH, L)))


def rb_lm_bytes(W, S, V):
    return _up16((64 + (S + 1) * W) * (16 + 8 + 3 * 4) + V)


def rb_lds_bytes(name, L, W, S, with_lm=False, hw_words=0):
    V, H, JH = sizes(name)
    return rb_fixed_bytes(W, S) + rb_union_bytes(W, min(W, V - 1), H, JH, L) + (rb_lm_bytes(W, S, V) if with_lm else 0) + 4 * hw_words


# ---- 6. confidence: the six heads at L = 1 on the cluster matrix's own state dicts and batches, C and E again at L = 2
CONF_SETS = [(name, 1) for name in sorted(K.HEADS)] + [("C", 2), ("E", 2)]
CONF_U = [33, 17, 16, 1, 5, 0]          # random paths: tokens per utterance (lengths 60, 33, 17, 16, 1, 0 frames)


@functools.lru_cache(maxsize=None)
def conf_head(name, L):
    """(cfg, state dict, float64 head, encp [6, 60, JH] float32, lengths): the head and batch of rnnt_cluster_cases.inputs(name); at
    L = 2 the same sizes, seed and blank bias with a second predictor layer."""
    cfg, sd, encoded, lengths = K.inputs(name)
    if L != 1:
        from gigaam_amd import synth
        cfg = K.head_cfg(name)
        cfg["head"]["decoder"]["pred_rnn_layers"] = L
        sd = synth.make_state_dict(cfg, seed=K.HEADS[name][3], rnnt_blank_bias=K.HEADS[name][4])
    hd = R.head_from_state_dict(sd, L)
    encp = np.stack([R.encoder_projection(hd, encoded[b]) for b in range(len(lengths))]).astype(np.float32)
    return cfg, sd, hd, encp, list(lengths)


@functools.lru_cache(maxsize=None)
def conf_paths(name, L):
    """{"greedy": rows, "random": rows, "invalid": rows}, rows = [(ids, frames)] per utterance.  greedy: the float64 greedy decode
    (rnnt_cluster_cases.reference at L = 1); random: valid paths of CONF_U tokens, several on one frame; invalid: the random rows
    with an out-of-range id in row 1 and decreasing frames in row 2."""
    _, _, hd, encp, lengths = conf_head(name, L)
    V = sizes(name)[0]
    if L == 1:
        greedy = [(r["ids"], r["frames"]) for r in K.reference(name)]
    else:
        _, _, encoded, _ = K.inputs(name)
        greedy = []
        for b, Tb in enumerate(lengths):
            r = R.greedy_trace(hd, encoded[b], Tb, K.MAX_SYMBOLS)
            greedy.append((r["ids"], r["frames"]))
    rng = np.random.default_rng(len(name) + 7 * L + V)
    rand = []
    for b, Tb in enumerate(lengths):
        n = CONF_U[b]
        rand.append((rng.integers(0, V - 1, n).tolist(), sorted(rng.integers(0, Tb, n).tolist()) if n else []))
    bad = [(list(i), list(f)) for i, f in rand]
    bad[1][0][3] = V - 1                                  # the blank id is no token
    bad[2][1][6] = bad[2][1][5] - 1                       # frames decrease
    return {"greedy": greedy, "random": rand, "invalid": bad}


INVALID_STATUS = [1, 0, 0, 1, 1, 1]


# ---- 7. gam_rnnt_joint / gam_rnnt_predict: heads C, D and E, B = 2, T = 5, U = 4
JOINT_HEADS = ["C", "D", "E"]


@functools.lru_cache(maxsize=None)
def joint_inputs(name):
    """(enc [2, 5, d_model] float32, labels [2][3]): the joint's grid is enc x the predictor outputs after 0..3 labels."""
    cfg = conf_head(name, 1)[0]
    V = sizes(name)[0]
    rng = np.random.default_rng(31 + V + len(name))
    enc = rng.standard_normal((2, 5, cfg["encoder"]["d_model"])).astype(np.float32)
    return enc, rng.integers(0, V - 1, (2, 3)).tolist()
