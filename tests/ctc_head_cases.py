"""Crafted inputs and the numpy / float64 reference of the CTC head matrix (tests/test_hip_ctc_head_matrix.py on the GPU,
tests/test_ctc_head_cases_host.py on the CPU): the token transpose, the head GEMM, gam_log_softmax_kernel and the batched
gam_ctc_greedy_kernel (gam_decode.h), and gam_emo_head_kernel.

Heads (d_model 768, one encoder layer that never runs: the cases hand ``encoded`` to the heads directly):

  tap<V>   V in TAP_V: weight [I_V | 0], bias 0.  Every product of the head GEMM is x * 1 or y * 0 and every partial sum is x + 0,
           whatever the order and whatever the split of K: logits[b, t, v] == encoded[b, v, t] bit for bit, for any finite input.
           The test writes the logits it wants, exact ties included; channels V.. of ``encoded`` hold noise that must not matter.
  planted  V = 1025 (> d_model: no tap; 17 strides per lane of the wave form): synth's random head at seed 0, frame t =
           6 W[lab_t] / |W[lab_t]| + 0.05 noise.
  tie, tie_hi  the planted head with duplicated weight rows and equal biases (TIE_PAIRS): the logits of a pair are the same fmaf
           chain over the same A row and identical W rows, so they tie bit for bit in any vocabulary.  (700, 1024) has a head of
           its own: in one head with (0, 1024) the three rows would be one group and class 0 would win it every time.

The expected labels are labels_ref (first maximum) of the float64 logits; on the tie heads the higher member of a pair is struck
out first, which states the rule "the lower index wins" without relying on two float64 dot products of equal rows being equal."""
import functools

import numpy as np

from ctc_greedy_long_ref import collapse_ref, labels_ref

D_MODEL = 768
NT = 512                                   # GAM_CTC_NT: frames per compaction pass of gam_ctc_greedy_kernel
TAP_V = [2, 34, 64, 33, 63, 66, 257]
PLANTED_V = 1025
TIE_PAIRS = {"tie": [(5, 37), (63, 64), (7, 71), (0, 1024)], "tie_hi": [(700, 1024), (5, 37)]}
HEADS = [f"tap{v}" for v in TAP_V] + ["planted", "tie", "tie_hi"]
T_GRID = [1, 63, 64, 511, 512, 513, 1024, 1025, 1537]
T_BORDER = 1100                            # three passes: both pass borders (511|512, 1023|1024) inside
BORDERS = [NT, 2 * NT]
MIN_MARGIN = 2e-3                          # twice TOL_LOGP, the rule of tests/test_rnnt_cluster_plan_host.py
# gam_ctc_greedy (gam_api.hip): LDS = (T' + GAM_CTC_NT / 64 + 8) ints, refused above 60 KiB
T_LIMIT = 60 * 1024 // 4 - (NT // 64 + 8)

EMO_NC = [1, 4, 65, 130]
EMO_T = [1, 63, 64, 65, 200]
PAD = 1e30                                 # emotion frames at t >= n


def head_v(head):
    return int(head[3:]) if head.startswith("tap") else PLANTED_V


def is_tap(head):
    return head.startswith("tap")


def thread_form(V):
    """The argmax form gam_ctc_greedy_kernel takes: one thread per frame for even V <= 64, one wave per frame otherwise."""
    return V <= 64 and V % 2 == 0


def head_cfg(head):
    from gigaam_amd import synth
    cfg = synth.model_cfg("v2_ctc", n_layers=1)
    cfg["head"]["num_classes"] = head_v(head)
    return cfg


@functools.lru_cache(maxsize=None)
def head_state(head):
    """(cfg, state dict) of a head."""
    import torch
    from gigaam_amd import synth
    cfg = head_cfg(head)
    sd = synth.make_state_dict(cfg, seed=0)
    V = head_v(head)
    if is_tap(head):
        w = torch.zeros((V, D_MODEL, 1), dtype=torch.float32)
        w[torch.arange(V), torch.arange(V), 0] = 1.0
        sd["head.decoder_layers.0.weight"] = w
        sd["head.decoder_layers.0.bias"] = torch.zeros((V,), dtype=torch.float32)
    for lo, hi in TIE_PAIRS.get(head, []):
        sd["head.decoder_layers.0.weight"][hi] = sd["head.decoder_layers.0.weight"][lo]
        sd["head.decoder_layers.0.bias"][hi] = sd["head.decoder_layers.0.bias"][lo]
    return cfg, sd


@functools.lru_cache(maxsize=None)
def head_wb(head):
    """(W [V, D] float32, bias [V] float32) as numpy."""
    _, sd = head_state(head)
    return sd["head.decoder_layers.0.weight"][:, :, 0].numpy().copy(), sd["head.decoder_layers.0.bias"].numpy().copy()


def canon(head):
    """class -> the class that wins its tie group (itself when it is in none)."""
    c = np.arange(head_v(head))
    for lo, hi in TIE_PAIRS.get(head, []):
        c[hi] = lo
    return c


def blank_is_tied(head):
    return any(hi == head_v(head) - 1 for _, hi in TIE_PAIRS.get(head, []))


# --------------------------------------------------------------------------- reference
def logits64(head, encoded):
    """float64 logits [B, T, V] of encoded float32 [B, D, T]: the exact logits of a tap head, the float64 head product otherwise."""
    V = head_v(head)
    if is_tap(head):
        return np.ascontiguousarray(encoded[:, :V, :].transpose(0, 2, 1)).astype(np.float64)
    w, b = head_wb(head)
    return np.einsum("bdt,vd->btv", encoded.astype(np.float64), w.astype(np.float64), optimize=True) + b.astype(np.float64)


def labels_and_margin(head, encoded):
    """(labels [B, T] with the first-maximum rule, the smallest top-1 / top-2 margin over DISTINCT classes): the higher member of
    every tie pair is struck out, so the lower one wins and the pair's zero gap is not counted as a margin."""
    lg = logits64(head, encoded)
    c = canon(head)
    lg[:, :, c != np.arange(c.shape[0])] = -np.inf
    B, T, V = lg.shape
    lab = labels_ref(lg.reshape(B * T, V)).reshape(B, T)
    if V > 1 and B * T:
        top2 = np.partition(lg.reshape(B * T, V), V - 2, axis=1)[:, V - 2:]
        margin = float((top2[:, 1] - top2[:, 0]).min())
    else:
        margin = float("inf")
    return lab, margin


def clamp_len(n, T):
    return min(max(int(n), 0), T)


def decode_ref(lab, enc_len, blank):
    """labels [B, T], lengths -> [(ids, frames)] of the greedy decode cut at clamp(len, 0, T)."""
    return [collapse_ref(lab[b, :clamp_len(n, lab.shape[1])], blank) for b, n in enumerate(enc_len)]


def log_softmax64(lg):
    m = lg.max(axis=-1, keepdims=True)
    return lg - (m + np.log(np.exp(lg - m).sum(axis=-1, keepdims=True)))


def logsumexp64(x):
    m = x.max(axis=-1)
    return m + np.log(np.exp(x - m[..., None]).sum(axis=-1))


# --------------------------------------------------------------------------- inputs from labels
def _seed(*parts):
    """A seed sequence from names and numbers (no hash(): stable across processes)."""
    return [int(p) if isinstance(p, (int, np.integer)) else sum((i + 1) * ord(ch) for i, ch in enumerate(str(p))) for p in parts]


def encode_labels(head, lab, seed):
    """labels [B, T] -> encoded float32 [B, D, T] whose frame (b, t) peaks at class lab[b, t].  Tap: N(0, 0.5) logits with + 6 at the
    label, N(0, 3) in the channels the head does not read.  Planted / tie: 6 W[lab] / |W[lab]| + 0.05 noise.  The noise differs in b,
    channel and t, so a transposed or shifted read decodes something else."""
    lab = np.asarray(lab)
    B, T = lab.shape
    V = head_v(head)
    rng = np.random.default_rng(_seed(head, seed, T))
    if is_tap(head):
        enc = (3.0 * rng.standard_normal((B, D_MODEL, T))).astype(np.float32)
        enc[:, :V, :] = (0.5 * rng.standard_normal((B, V, T))).astype(np.float32)
        bb, tt = np.meshgrid(np.arange(B), np.arange(T), indexing="ij")
        enc[bb, lab, tt] += np.float32(6.0)
        return enc
    w, _ = head_wb(head)
    unit = w / np.linalg.norm(w.astype(np.float64), axis=1, keepdims=True).astype(np.float32)
    enc = np.float32(6.0) * unit[lab].transpose(0, 2, 1) + np.float32(0.05) * rng.standard_normal((B, D_MODEL, T)).astype(np.float32)
    return np.ascontiguousarray(enc, dtype=np.float32)


def run_labels(B, T, V, rng):
    """Runs of up to three equal labels, about a third of the frames blank (as _random_lp of tests/test_hip_ctc_greedy_long.py)."""
    lab = np.repeat(rng.integers(0, V, size=(B, (T + 2) // 3)), 3, axis=1)[:, :T]
    return np.where(rng.random((B, T)) < 0.33, V - 1, lab)


def _peaks_behind_len(lab, enc_len, V):
    """Frames at t >= len hold non-blank peaks that differ from their neighbours: a decode without the t < len test emits them."""
    B, T = lab.shape
    for b, n in enumerate(enc_len):
        n = clamp_len(n, T)
        lab[b, n:] = (np.arange(n, T) + b) % (V - 1)
    return lab


def _case(head, name, kind, lab, enc_len, seed):
    return dict(head=head, name=name, kind=kind, planted=np.asarray(lab), enc_len=[int(n) for n in enc_len],
                encoded=encode_labels(head, lab, seed))


GRID_BATCHES = ("a", "b")


def grid_lens(T, which):
    return [T, T + 9, (T + 1) // 2, 0] if which == "a" else [-3, 1, NT, NT + 1]


def grid_case(head, T, which):
    """The length grid: per T' a batch with enc_len (T', T' + 9, ceil(T' / 2), 0) and one with (-3, 1, 512, 513).  Not cached: the
    largest is 19 MB and there are 180 of them."""
    V = head_v(head)
    lens = grid_lens(T, which)
    rng = np.random.default_rng(_seed(head, "grid", T, which))
    lab = run_labels(4, T, V, rng)
    for p in BORDERS:                          # utterance 0: a token on the first frame of every later pass, whatever T' - p is
        if T > p:
            lab[0, p - 1], lab[0, p] = V - 1, (1 + p % (V - 2) if V > 2 else 0)
    lab = _peaks_behind_len(lab, lens, V)
    return _case(head, f"grid-T{T}-{which}", "grid", lab, lens, 1)


BORDER_ROWS = ["same", "label-blank-label", "blank-behind", "different", "run-starts", "cut-512", "cut-513", "starts-cut-512",
               "starts-cut-513"]


@functools.lru_cache(maxsize=None)
def border_case(head):
    """One batch, T' = T_BORDER, a row per scenario, each at both pass borders p = 512, 1024; everything else blank but three early
    tokens (a non-zero ``base`` when the second pass starts).  k2 = k for V = 2, which has one non-blank class."""
    V, T = head_v(head), T_BORDER
    blank, k = V - 1, min(3, V - 2)
    k2 = (k + 1) % (V - 1)
    lab = np.full((len(BORDER_ROWS), T), blank)
    lens = [T] * len(BORDER_ROWS)
    lab[:, [2, 40, 300]] = k
    for r, row in enumerate(BORDER_ROWS):
        for p in BORDERS:
            if row == "same":
                lab[r, p - 1:p + 1] = k
            elif row == "label-blank-label":
                lab[r, [p - 2, p]] = k
            elif row == "blank-behind":
                lab[r, [p - 1, p + 1]] = k
            elif row == "different":
                lab[r, p - 1], lab[r, p] = k, k2
            elif row == "run-starts":
                lab[r, p:p + 3] = k
        if "cut" in row:                            # a run over the border (cut-*) or from the border on (starts-cut-*), cut by enc_len
            lab[r, (NT if row.startswith("starts") else NT - 2):NT + 4] = k
            lens[r] = int(row[-3:])
    lab = _peaks_behind_len(lab, lens, V)
    return _case(head, "borders", "border", lab, lens, 2)


@functools.lru_cache(maxsize=None)
def extreme_case(head):
    """All blank (count 0); one label throughout (count 1, frame 0); alternating non-blank labels (count = T': buffers full)."""
    V, T = head_v(head), T_BORDER
    lab = np.full((3, T), V - 1)
    lab[1] = min(3, V - 2)
    lab[2] = np.arange(T) % (V - 1)
    return _case(head, "extremes", "extreme", lab, [T, T, T], 3)


@functools.lru_cache(maxsize=None)
def limit_case():
    """tap34, B = 1, T' = T_LIMIT: the largest the launcher accepts, a 60 KiB dynamic-LDS launch."""
    V = 34
    rng = np.random.default_rng(_seed("limit"))
    return _case("tap34", "limit", "limit", run_labels(1, T_LIMIT, V, rng), [T_LIMIT], 4)


_EXPECTED = {}


def expected(case):
    """(labels [B, T], margin, [(ids, frames)]) of a label-built case by the float64 reference; computed once per (head, name) and
    shared, not to be changed."""
    key = (case["head"], case["name"])
    if key not in _EXPECTED:
        lab, margin = labels_and_margin(case["head"], case["encoded"])
        _EXPECTED[key] = (lab, margin, decode_ref(lab, case["enc_len"], head_v(case["head"]) - 1))
    return _EXPECTED[key]


# --------------------------------------------------------------------------- exact ties (tap heads)
TIE_VALUE = np.float32(2.0)


def tie_rows(V):
    """[(name, row float32 [V], classes that hold the row's maximum -- the first is the expected label)] for a tap head.  Every
    other value of a row is distinct noise at least 3 below the tie."""
    rng = np.random.default_rng(_seed("tierows", V))
    blank = V - 1
    rows = []

    def noise():
        return (rng.permutation(V).astype(np.float32) / np.float32(V) - np.float32(8.0)).astype(np.float32)

    def tied(name, classes, value=TIE_VALUE):
        classes = sorted(set(int(c) for c in classes))
        if len(classes) >= 2 and classes[-1] < V and classes[0] >= 0:
            row = noise()
            row[classes] = value
            rows.append((name, row, classes))

    if V >= 3:
        a, b = sorted(rng.choice(V - 1, size=2, replace=False).tolist())
        tied("two", [a, b])
    if V >= 4:
        tied("three", rng.choice(V - 1, size=3, replace=False).tolist())
    row = noise()                                   # the maximum at class 0, every value negative
    row[0] = np.float32(-1.0)
    rows.append(("negative-max-at-0", row, [0]))
    if V % 2 == 0 and V >= 4:
        j = 2 * int(rng.integers(0, V // 2 - 1))
        tied("pair-halves", [j, j + 1])             # the .x and .y of one 8-byte load
    tied("last-pair", [V - 2, V - 1])               # (blank against the class below it; even V: the last 8-byte pair)
    if V >= 3:
        tied("blank-and-lower", [int(rng.integers(0, V - 2)), blank])
    tied("blank-and-0", [0, blank])
    rows.append(("constant", np.full((V,), np.float32(0.25)), list(range(V))))
    rows.append(("all-lowest", np.full((V,), np.float32(-3e38)), list(range(V))))
    for d in (1, 32, 64):                           # neighbouring lanes; the first shuffle distance; two strides of one lane
        if V - 1 - d > 0:
            v = int(rng.integers(0, V - 1 - d))
            tied(f"lanes-v-v+{d}", [v, v + d])
    if V > 128:
        tied("strides-0-1-2", [5, 69, 133])
        tied("stride-border", [63, 64])
    return rows


@functools.lru_cache(maxsize=None)
def tie_case(head):
    """B = 2 (the rows in two orders); every tie row sits between two frames that peak at blank, so its label is emitted on its own."""
    V = head_v(head)
    rows = tie_rows(V)
    T = 2 * len(rows) + 1
    rng = np.random.default_rng(_seed("tiecase", V))
    enc = (3.0 * rng.standard_normal((2, D_MODEL, T))).astype(np.float32)
    sep = (rng.permutation(V).astype(np.float32) / np.float32(V) - np.float32(8.0)).astype(np.float32)
    sep[V - 1] = np.float32(6.0)
    enc[:, :V, :] = sep[None, :, None]
    want = np.full((2, T), V - 1)
    names = [[None] * T, [None] * T]
    for b in range(2):
        order = list(range(len(rows))) if b == 0 else list(reversed(range(len(rows))))
        for i, r in enumerate(order):
            enc[b, :V, 2 * i + 1] = rows[r][1]
            want[b, 2 * i + 1] = rows[r][2][0]
            names[b][2 * i + 1] = rows[r][0]
    return dict(head=head, name="ties", kind="tie", encoded=enc, enc_len=[T, T], want=want, names=names, rows=rows)


# --------------------------------------------------------------------------- log-prob cases
LOGP_SHAPES = [(3, 5), (2, 70)]              # 15 rows (no multiple of the kernel's 4 rows per workgroup) and 140
LOGP_KINDS_TAP = ["spread0", "underflow", "near1e4", "normal"]
LOGP_KINDS_PLANTED = ["zero-input", "underflow", "peaked", "normal"]


def logp_kinds(head):
    return LOGP_KINDS_TAP if is_tap(head) else LOGP_KINDS_PLANTED


@functools.lru_cache(maxsize=None)
def logp_case(head, shape):
    """encoded [B, D, T'] whose row (b, t) is of kind kinds[(b T' + t) % 4], and the kind of every row.
    Tap: spread 0 (one value); N(0, 60) with one class 150 above the rest (every other exponential underflows); all values near
    + 1e4; N(0, 1).
    Planted / tie (the logits are a product, not free): zero input (logits = bias); 40 W[k] / |W[k]| (peak ~ 138 above the rest);
    6 W[k] / |W[k]|; N(0, 1) input."""
    B, T = shape
    V = head_v(head)
    kinds = logp_kinds(head)
    rng = np.random.default_rng(_seed("logp", head, B, T))
    enc = (3.0 * rng.standard_normal((B, D_MODEL, T))).astype(np.float32)
    kind_of = np.empty((B, T), dtype=object)
    if not is_tap(head):
        w, _ = head_wb(head)
        unit = w / np.linalg.norm(w.astype(np.float64), axis=1, keepdims=True).astype(np.float32)
    for b in range(B):
        for t in range(T):
            kind = kinds[(b * T + t) % 4]
            kind_of[b, t] = kind
            if kind == "spread0":
                x = np.full((V,), np.float32(rng.standard_normal()))
            elif kind == "underflow" and is_tap(head):
                x = 60.0 * rng.standard_normal(V)
                x[int(rng.integers(0, V))] = x.max() + 150.0
            elif kind == "near1e4":
                x = 1e4 + rng.standard_normal(V)
            elif kind == "normal" and is_tap(head):
                x = rng.standard_normal(V)
            elif kind == "zero-input":
                x = np.zeros((D_MODEL,))
            elif kind == "underflow":
                x = 40.0 * unit[int(rng.integers(0, V))] + 0.05 * rng.standard_normal(D_MODEL)
            elif kind == "peaked":
                x = 6.0 * unit[int(rng.integers(0, V))] + 0.05 * rng.standard_normal(D_MODEL)
            else:
                x = rng.standard_normal(D_MODEL)
            enc[b, :x.shape[0], t] = np.asarray(x, dtype=np.float32)
    return enc, kind_of


# --------------------------------------------------------------------------- non-finite rows
def nonfinite_logits(V, T=NT + 30, seed=0):
    """[T, V] float32 peaked rows (runs, a third blank) where frame t % 7 == 3 is all NaN and frame t % 7 == 5 holds ONE NaN (at the
    class that would have won); returns (rows, all-NaN mask, single-NaN mask)."""
    rng = np.random.default_rng(_seed("nonfinite", V, seed))
    lab = run_labels(1, T, V, rng)[0]
    x = (0.5 * rng.standard_normal((T, V))).astype(np.float32)
    x[np.arange(T), lab] += np.float32(6.0)
    t = np.arange(T)
    all_nan, one_nan = t % 7 == 3, t % 7 == 5
    x[all_nan, :] = np.nan
    x[t[one_nan], lab[one_nan]] = np.nan
    return x, all_nan, one_nan


# --------------------------------------------------------------------------- emotion head
def emo_cfg(nc):
    from gigaam_amd import synth
    cfg = synth.model_cfg("emo", n_layers=1)
    cfg["head"]["out_features"] = nc
    return cfg


@functools.lru_cache(maxsize=None)
def emo_state(nc):
    from gigaam_amd import synth
    cfg = emo_cfg(nc)
    return cfg, synth.make_state_dict(cfg, seed=0)


def emo_lens(T):
    """enc_len of the batch with lengths (the kernel clamps n to [1, T']); the call without lengths is apart."""
    return [T, 1, 0, T + 5, 64, 65]


@functools.lru_cache(maxsize=None)
def emo_case(nc, T, with_lens):
    """(encoded [B, D, T'], enc_len or None): N(0, 1) frames; with lengths, the frames at t >= clamp(len, 1, T') hold PAD."""
    rng = np.random.default_rng(_seed("emo", nc, T, int(with_lens)))
    lens = emo_lens(T) if with_lens else None
    B = len(lens) if with_lens else 2
    enc = rng.standard_normal((B, D_MODEL, T)).astype(np.float32)
    if with_lens:
        for b, n in enumerate(lens):
            enc[b, :, min(max(n, 1), T):] = np.float32(PAD)
    return enc, lens


def emo_ref(nc, enc, lens):
    """float64: mean over the first clamp(len, 1, T') frames, Linear, softmax -> [B, nc]."""
    _, sd = emo_state(nc)
    w, b = sd["head.weight"].numpy().astype(np.float64), sd["head.bias"].numpy().astype(np.float64)
    B, _, T = enc.shape
    out = np.zeros((B, nc))
    for i in range(B):
        n = T if lens is None else min(max(lens[i], 1), T)
        lg = w @ enc[i, :, :n].astype(np.float64).mean(axis=1) + b
        e = np.exp(lg - lg.max())
        out[i] = e / e.sum()
    return out
