"""CPU: the float64 reference of CTC alignment with wildcards (tests/ctc_align_star_ref.py) against brute force and torch's CTC loss,
the two properties the default penalty was chosen for, and the host side of ``align(..., wildcard=)`` (gigaam_amd/wildcard.py)."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_align_ref as R
import ctc_align_star_ref as RS

LN2 = math.log(2)


# ------------------------------------------------------------------ the reference against brute force
def _collapse(labels, blank):
    out, prev = [], None
    for l in labels:
        if l != prev and l != blank:
            out.append(l)
        prev = l
    return out


def _brute(lp, star, y, T):
    """Every label sequence of T frames that collapses to y: (best score, its labels, log-sum-exp of all)."""
    V = lp.shape[1]
    blank, wild = V - 1, V
    alphabet = sorted(set(y)) + [blank]
    em = lambda t, l: float(star[t]) if l == wild else float(lp[t, l])
    best, best_labels, scores = -np.inf, None, []
    for seq in itertools.product(alphabet, repeat=T):
        if _collapse(seq, blank) != list(y):
            continue
        sc = sum(em(t, l) for t, l in enumerate(seq))
        scores.append(sc)
        if sc > best:
            best, best_labels = sc, list(seq)
    ll = float(np.logaddexp.reduce(scores)) if scores else -np.inf
    return best, best_labels, ll


def test_reference_matches_brute_force_with_wildcards_in_every_position():
    rng = np.random.default_rng(3)
    V = 4                                   # labels 0..2, blank 3, wildcard 4
    targets = [list(t) for U in range(4) for t in itertools.product([0, 1, V], repeat=U)]
    assert [V, V, V] in targets and [0, V, 0] in targets and [V] in targets
    n = 0
    for y in targets:
        for T in range(0, 7):
            lp = np.log(rng.dirichlet(np.ones(V), size=max(T, 1)))
            star = rng.uniform(-2.0, 0.0, size=max(T, 1))
            score, states = RS.viterbi(lp, star, y, T)
            ll = RS.forward_loglik(lp, star, y, T)
            if T == 0:
                assert (states == [] and score == 0.0 and ll == 0.0) if not y else (states is None and ll == -np.inf)
                continue
            b_score, b_labels, b_ll = _brute(lp, star, y, T)
            assert (states is None) == (b_labels is None), (y, T)
            assert RS.feasible(T, y, V) == (b_labels is not None), (y, T)
            if states is None:
                assert score == -np.inf and ll == -np.inf
                continue
            assert abs(score - b_score) < 1e-12 and abs(ll - b_ll) < 1e-12, (y, T)
            labels = RS.state_labels(states, y, V)
            assert labels == b_labels, (y, T)              # (continuous values: the optimum is unique)
            assert RS.path_states(labels, y, V) == states
            assert abs(RS.rescore(lp, star, labels) - score) < 1e-12
            n += 1
    assert n > 150


def test_reference_rejects_blank_and_ids_past_the_wildcard():
    V = 6
    assert RS.feasible(3, [0, V, 1], V) and not R.feasible(3, [0, V, 1], V)
    assert not RS.feasible(3, [0, V - 1], V) and not RS.feasible(3, [V + 1], V) and not RS.feasible(3, [-1], V)
    assert RS.feasible(3, [V, V], V) and not RS.feasible(2, [V, V], V)      # two adjacent wildcards are a repeat
    assert RS.feasible(2, [V, 0], V) and RS.feasible(1, [V], V) and not RS.feasible(0, [V], V)


def test_reference_loglik_matches_torch_ctc_loss_on_the_augmented_matrix():
    rng = np.random.default_rng(8)
    worst = 0.0
    for V, T, U in ((5, 12, 4), (34, 60, 20), (34, 25, 25), (257, 90, 30)):
        lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((T, V))), dim=-1).numpy()
        star = lp.max(axis=1) - LN2
        for trial in range(4):
            y = [int(v) for v in rng.integers(0, V - 1, U)]
            for u in rng.choice(U, size=1 + trial % 3, replace=False):
                y[u] = V
            if not RS.feasible(T, y, V):
                assert RS.forward_loglik(lp, star, y) == -np.inf
                continue
            aug = torch.from_numpy(RS.augment(lp, star))
            loss = F.ctc_loss(aug[:, None, :], torch.tensor([RS.map_target(y, V)]), torch.tensor([T]), torch.tensor([U]), blank=V,
                              reduction="none")
            ll = RS.forward_loglik(lp, star, y)
            worst = max(worst, abs(ll + float(loss[0])))
    assert worst < 1e-11, worst


# ------------------------------------------------------------------ what the default penalty is for
def _peaked_utterance(rng, V=34):
    """A greedy path that spells tokens y (runs of 1-3 frames, 0-3 blanks between them, one at least between equal tokens) and
    log-probs peaked on it: (lp [T, V] float32 log-softmax, y)."""
    U = int(rng.integers(5, 13))
    y = [int(v) for v in rng.integers(0, V - 1, U)]
    labels = [V - 1] * int(rng.integers(0, 4))
    for u, v in enumerate(y):
        gap = int(rng.integers(0, 4))
        if u > 0 and y[u - 1] == v:
            gap = max(gap, 1)
        if u > 0:
            labels += [V - 1] * gap
        labels += [v] * int(rng.integers(1, 4))
    labels += [V - 1] * int(rng.integers(0, 4))
    x = rng.standard_normal((len(labels), V)).astype(np.float32)
    x[np.arange(len(labels)), labels] = 9.0
    return torch.log_softmax(torch.from_numpy(x), dim=-1).numpy(), y


def test_wildcard_at_ln2_takes_the_removed_span_and_nothing_else():
    """300 seeded peaked utterances, an inner span y[a:b] replaced by one wildcard, star = rowmax - ln 2: every kept token keeps the
    first frame it has in the full alignment, and the wildcard's run covers every removed token's run and touches no neighbour's."""
    rng = np.random.default_rng(2024)
    V = 34
    moved = uncovered = 0
    for _ in range(300):
        lp, y = _peaked_utterance(rng, V)
        U = len(y)
        _, full = R.viterbi(lp, y)
        f_first, f_last = R.token_runs(full, U)
        a = int(rng.integers(1, U - 1))
        b = int(rng.integers(a + 1, U))            # 1 <= a < b <= U - 1: an inner span
        part = y[:a] + [V] + y[b:]
        star = RS.star_row(lp, LN2)
        _, states = RS.viterbi(lp, star, part)
        assert states is not None
        first, last = RS.token_runs(states, len(part))
        kept_full = f_first[:a] + f_first[b:]
        kept_part = first[:a] + first[a + 1:]
        moved += kept_full != kept_part
        ok = first[a] <= f_first[a] and last[a] >= f_last[b - 1]                 # covers the removed runs
        ok = ok and first[a] > f_last[a - 1] and last[a] < f_first[b]            # touches no neighbour's run
        uncovered += not ok
    assert moved == 0 and uncovered == 0, (moved, uncovered)


# ------------------------------------------------------------------ gigaam_amd/wildcard.py
VOCAB = [" ", "а", "б", "в", "г"]


def _tok():
    from gigaam_amd.decoding import Tokenizer
    return Tokenizer(VOCAB)


def test_text_is_split_at_the_wildcard_and_wildcards_merge():
    from gigaam_amd import wildcard as W
    tok, wid = _tok(), len(VOCAB) + 1
    enc = lambda text, w="*": W.encode(tok, text, w, wid, True)
    assert enc("аб*в") == [1, 2, wid, 3]
    assert enc("*аб") == [wid, 1, 2] and enc("аб*") == [1, 2, wid] and enc("*") == [wid]
    assert enc("а * б") == [1, 0, wid, 0, 2]                      # spaces stay where they are
    assert enc("а**б") == [1, wid, 2] and enc("***") == [wid]     # empty pieces between wildcards: one wildcard
    assert enc("а<gap>б", "<gap>") == [1, wid, 2]
    assert enc("абв") == [1, 2, 3] and enc("") == []
    assert W.encode(tok, "аб", None, wid, False) == [1, 2]
    # token-id lists: the wildcard id needs one of the keywords; adjacent ones merge
    assert W.encode(tok, [1, wid, wid, 2], None, wid, True) == [1, wid, 2]
    assert W.encode(tok, [1, 2], None, wid, False) == [1, 2]
    with pytest.raises(ValueError, match="outside the vocabulary"):
        W.encode(tok, [1, wid, 2], None, wid, False)
    with pytest.raises(ValueError, match="not in the vocabulary"):
        enc("аб*x")                                                # a piece the tokenizer cannot spell
    assert W.text_of(tok, [1, 2, wid, 3], wid, "*") == "аб*в" and W.text_of(tok, [wid, 1], wid, "*") == "*а"


def test_wildcard_keywords_are_checked():
    from gigaam_amd import wildcard as W
    tok = _tok()
    assert W.check(tok, "*", LN2) == LN2 and W.check(tok, None, 0.0) == 0.0 and W.check(tok, "<gap>", 3) == 3.0
    with pytest.raises(ValueError, match="can spell"):
        W.check(tok, "а", LN2)
    with pytest.raises(ValueError, match="can spell"):
        W.check(tok, " ", LN2)
    with pytest.raises(ValueError, match="non-empty"):
        W.check(tok, "", LN2)
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="wildcard_penalty"):
            W.check(tok, "*", bad)


def test_gaps_and_words_from_an_aligned_host_dict():
    """What ``Aligned.host()`` returns for "аб *в г*" on 20 frames -> words per wildcard-free run and a Gap per wildcard."""
    from gigaam_amd import wildcard as W
    from gigaam_amd.types import Gap, Word
    tok, wid = _tok(), len(VOCAB) + 1
    ids = W.encode(tok, "аб *в г*", "*", wid, True)
    assert ids == [1, 2, 0, wid, 3, 0, 4, wid]
    h = {"tok_first": np.array([[0, 2, 3, 4, 9, 11, 12, 14, -1]], dtype=np.int32),
         "tok_last": np.array([[1, 2, 3, 8, 10, 11, 13, 19, -1]], dtype=np.int32), "status": np.array([1], dtype=np.int32)}
    n = len(ids)
    first, last = h["tok_first"][0, :n].tolist(), h["tok_last"][0, :n].tolist()
    shift = 0.04
    words, gaps = W.short_result(tok, ids, first, last, shift, wid)
    assert words == [Word("аб", 0 * shift, 3 * shift), Word("в", 9 * shift, 10 * shift), Word("г", 12 * shift, 13 * shift)]
    assert gaps == [Gap(4 * shift, 9 * shift, 4, 8), Gap(14 * shift, 20 * shift, 14, 19)]
    for w in words:                                               # no word spans a gap
        assert all(w.end <= g.start + 1e-12 or w.start >= g.end - 1e-12 for g in gaps)
    # without the split "в г" and "аб" would still be words, but a word "бв" could form across a gap: "аб*в" has no space there
    ids2 = W.encode(tok, "аб*в", "*", wid, True)
    words2, gaps2 = W.short_result(tok, ids2, [0, 1, 2, 7], [0, 1, 6, 8], shift, wid)
    assert [w.text for w in words2] == ["аб", "в"] and len(gaps2) == 1
    assert W.runs(ids, wid) == ([(0, 3), (4, 7)], [3, 7]) and W.runs([wid], wid) == ([], [0])


def test_longform_gap_may_cross_speech_regions():
    from gigaam_amd import wildcard as W
    from gigaam_amd.timestamps_utils import concat_frames_to_segments
    tok, wid = _tok(), len(VOCAB) + 1
    ids = [1, wid, 2]                                             # "а*б" over two regions of 10 frames each
    seg_frames, boundaries, shifts = [10, 10], [(1.0, 1.4), (5.0, 5.4)], [0.04, 0.04]
    starts = [b[0] for b in boundaries]
    ts, tf, _ = concat_frames_to_segments([2, 6, 15], seg_frames, starts, shifts)
    ls, lf, _ = concat_frames_to_segments([3, 13, 16], seg_frames, starts, shifts)
    words, segs, gaps = W.longform_result(tok, ids, ts, tf, ls, lf, boundaries, shifts, wid)
    assert [w.text for w in words] == ["а", "б"]
    assert [s.text for s in segs] == ["а", "б"]
    (g,) = gaps
    assert (g.segment, g.end_segment, g.start_frame, g.end_frame) == (0, 1, 6, 3)
    assert g.start == round(1.0 + 6 * 0.04, 3) and g.end == round(5.0 + 4 * 0.04, 3)
    assert words[0].end <= g.start and words[1].start >= g.end
