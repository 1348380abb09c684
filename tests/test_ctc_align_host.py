"""CPU: Tokenizer.encode, and the float64 forced-alignment reference (tests/ctc_align_ref.py) checked against torch's CTC loss,
brute-force path enumeration and the golden greedy decodes."""
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from common import ROOT, split_ragged

import ctc_align_ref as R
from gigaam_amd import synth
from gigaam_amd.decoding import Tokenizer

CTC_CASES = ["v1_ctc_l2", "v2_ctc_l2", "v3_ctc_l2", "v3_e2e_ctc_l2"]


def _golden(name):
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))
    return gold, split_ragged(gold["ids"], gold["frames"], gold["counts"].tolist())


def test_tokenizer_encode_char_round_trip():
    tok = Tokenizer(synth.CHAR_VOCAB)
    text = "съешь же ещё этих мягких французских булок"
    ids = tok.encode(text.replace("ё", "е"))
    assert tok.decode(ids) == text.replace("ё", "е")
    rng = np.random.default_rng(0)
    ids = rng.integers(0, len(synth.CHAR_VOCAB), 200).tolist()
    assert tok.encode(tok.decode(ids)) == ids
    assert tok.encode("") == []


def test_tokenizer_encode_names_every_unknown_character():
    tok = Tokenizer(synth.CHAR_VOCAB)
    with pytest.raises(ValueError) as e:
        tok.encode("привет, Мир!")
    msg = str(e.value)
    for c in (",", "М", "!"):
        assert repr(c) in msg, msg
    with pytest.raises(ValueError):
        tok.encode("ё")           # no silent normalisation


def test_tokenizer_encode_sentencepiece_round_trip():
    pytest.importorskip("sentencepiece")
    tok = Tokenizer([], os.path.join(ROOT, "tests", "golden", "spm256.model"))
    for ids in ([3, 4, 5], [8, 1, 2, 9, 10], list(range(3, 40))):
        text = tok.decode(ids)
        enc = tok.encode(text)
        assert all(isinstance(i, int) for i in enc)
        assert tok.decode(enc) == text
    assert tok.encode(tok.decode([3, 4, 5])) == [3, 4, 5]


@pytest.mark.parametrize("name", CTC_CASES)
def test_reference_loglik_equals_torch_ctc_loss(name):
    gold, ref = _golden(name)
    lp = torch.from_numpy(gold["log_probs"]).double()
    elen = gold["enc_len"].tolist()
    V = lp.shape[2]
    targets = [ids for ids, _ in ref]
    tl = torch.tensor([len(t) for t in targets])
    flat = torch.tensor([i for t in targets for i in t], dtype=torch.long)
    loss = F.ctc_loss(lp.transpose(0, 1), flat, torch.tensor(elen), tl, blank=V - 1, reduction="none", zero_infinity=False)
    for b, t in enumerate(targets):
        got = R.forward_loglik(gold["log_probs"][b], t, elen[b])
        assert abs(got + float(loss[b])) <= 1e-9 * max(1.0, abs(got)), (b, got, -float(loss[b]))


def _brute_force(lp, y):
    """Every label sequence of length T that collapses to y: (best score, tie-rule path as states, log-sum-exp of all)."""
    T, V = lp.shape
    blank = V - 1
    best, best_key, best_states, scores = -np.inf, None, None, []
    for labels in itertools.product(range(V), repeat=T):
        states = R.path_states(labels, y, blank)
        if states is None:
            continue
        sc = float(sum(lp[t, l] for t, l in enumerate(labels)))
        scores.append(sc)
        key = tuple(reversed(states))      # the tie rule: largest state sequence read from the last frame backwards
        if sc > best or (sc == best and key > best_key):
            best, best_key, best_states = sc, key, states
    lse = float(np.logaddexp.reduce(scores)) if scores else -np.inf
    return best, best_states, lse


@pytest.mark.parametrize("ties", [False, True])
def test_reference_viterbi_equals_brute_force(ties):
    rng = np.random.default_rng(7 if ties else 3)
    V = 4
    n = 0
    for T in range(1, 7):
        for _ in range(6):
            U = int(rng.integers(0, min(T, 3) + 1))
            y = rng.integers(0, V - 1, U).tolist()
            if ties:   # dyadic values: exact sums, many equal paths
                lp = rng.choice([0.0, -0.5, -1.0, -2.0], size=(T, V))
            else:
                lp = np.log(rng.dirichlet(np.ones(V), size=T))
            score, states = R.viterbi(lp, y)
            bf, bf_states, lse = _brute_force(lp, y)
            if bf_states is None:
                assert states is None and not R.feasible(T, y, V)
                continue
            n += 1
            assert score == pytest.approx(bf, abs=1e-12)
            assert states == bf_states, (T, y, lp)
            assert R.forward_loglik(lp, y) == pytest.approx(lse, abs=1e-9)
            labels = R.state_labels(states, y, V - 1)
            assert R.path_states(labels, y, V - 1) == states
            assert R.rescore(lp, labels) == pytest.approx(score, abs=1e-12)
    assert n >= 20


def _margins(lp):
    """Per-frame top-1 / top-2 margin of log-probs [T, V]."""
    top = np.sort(np.asarray(lp, dtype=np.float64), axis=1)
    return top[:, -1] - top[:, -2]


@pytest.mark.parametrize("name", CTC_CASES)
def test_reference_viterbi_reproduces_golden_greedy_frames(name):
    """The greedy path is the global optimum of its own transcript: aligning the golden ids gives back the golden frames (on
    every token whose frame boundary is not a near-tie) and scores the sum of per-frame maxima."""
    gold, ref = _golden(name)
    checked = 0
    for b, (ids, frames) in enumerate(ref):
        T = int(gold["enc_len"][b])
        lp = gold["log_probs"][b][:T]
        score, states = R.viterbi(lp, ids, T)
        assert states is not None
        assert score == pytest.approx(float(lp.astype(np.float64).max(axis=1).sum()), abs=1e-9)
        first, _ = R.token_runs(states, len(ids))
        m = _margins(lp)
        for u, f in enumerate(frames):
            if min(m[max(f - 1, 0)], m[f]) > 1e-6:
                assert first[u] == f, (b, u)
                checked += 1
    assert checked >= 0.9 * sum(len(i) for i, _ in ref)
