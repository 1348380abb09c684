"""GPU, op level: gam_op_ctc_greedy_long (gigaam_amd/csrc/gam_stitch.h) -- the CTC greedy decode of ONE utterance of any length as three
plain launches over blocks of 512 frames (128 in the one-wave-per-frame form) -- against the numpy reference (tests/ctc_greedy_long_ref.py): ids, frames and count must be
equal exactly.  The optional cross-check against the width-1 beam search is left out: a width-1 prefix beam search sums the paths of a
prefix, so it equals the greedy decode only where every frame's maximum outweighs the rest of its row by a margin that depends on T."""
import numpy as np
import pytest
import torch

from ctc_greedy_long_ref import collapse_ref, greedy_ref
from test_hip_ctc_align import _op_engine

pytestmark = pytest.mark.gpu

FB = 512                                     # frames per block (GAM_GL_FB; the wave form's 128 divides it: its borders are borders there too)
T_CASES = [0, 1, 511, 512, 513, 1025, 3 * 512 + 7, 70001]
V_CASES = [2, 33, 34, 64, 66, 257, 1025]     # one thread per frame: even V <= 64; one wave per frame otherwise


def _decode(lp):
    """log-probs (torch, any device) [T, V] -> (ids, frames) host lists through the op and ``HipEngine.collect``."""
    from gigaam_amd.engine import Decoded, HipEngine
    dec = _op_engine().op_ctc_greedy_long(lp)
    assert isinstance(dec, Decoded) and dec.ids.shape == (1, lp.shape[0])
    rows, flag = HipEngine.collect(dec)
    assert not flag and len(rows) == 1
    assert int(dec.counts.cpu()[0]) == len(rows[0][0])
    return rows[0]


def _random_lp(T, V, seed):
    """Peaked rows on the device: runs of up to three equal labels, about a third of the frames blank."""
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    lp = torch.randn((T, V), generator=g, device="cuda:0")
    if T:
        lab = torch.randint(0, V, ((T + 2) // 3,), generator=g, device="cuda:0").repeat_interleave(3)[:T]
        lab = torch.where(torch.rand((T,), generator=g, device="cuda:0") < 0.33, torch.full_like(lab, V - 1), lab)
        lp[torch.arange(T, device="cuda:0"), lab] += 6.0
    return torch.log_softmax(lp, dim=1)


def _from_labels(lab, V):
    lab = np.asarray(lab)
    lp = np.full((lab.shape[0], V), -5.0, dtype=np.float32)
    lp[np.arange(lab.shape[0]), lab] = -0.01
    return lp


@pytest.mark.parametrize("V", V_CASES)
@pytest.mark.parametrize("T", T_CASES)
def test_random_log_probs_decode_like_the_reference(T, V):
    lp = _random_lp(T, V, seed=1000 * V + T % 997)
    ids, frames = _decode(lp)
    want_ids, want_frames = greedy_ref(lp.cpu().numpy())
    assert ids == want_ids and frames == want_frames
    if T >= 511:
        assert 0 < len(ids) < T


@pytest.mark.parametrize("V", [34, 257])
def test_runs_and_repeats_across_the_block_borders(V):
    T, blank, tok = 3 * FB + 7, V - 1, 5
    borders = [FB, 2 * FB, 3 * FB]
    # one run of a label across every border: emitted once, at its first frame
    lab = np.full((T,), blank)
    for b in borders:
        lab[b - 2:b + 2] = tok
    assert _decode(torch.from_numpy(_from_labels(lab, V))) == ([tok] * 3, [b - 2 for b in borders])
    # the same label on both sides of a border with one blank between (the blank before, then behind the border): emitted twice
    lab = np.full((T,), blank)
    lab[[FB - 2, FB]] = tok                   # blank at FB - 1
    lab[[2 * FB - 1, 2 * FB + 1]] = tok       # blank at 2 FB
    assert _decode(torch.from_numpy(_from_labels(lab, V))) == ([tok] * 4, [FB - 2, FB, 2 * FB - 1, 2 * FB + 1])
    # a label that changes exactly at the border, and one that starts on a block's first frame
    lab = np.full((T,), blank)
    lab[FB - 1], lab[FB], lab[2 * FB], lab[0] = tok, tok + 1, tok, tok + 2
    assert _decode(torch.from_numpy(_from_labels(lab, V))) == ([tok + 2, tok, tok + 1, tok], [0, FB - 1, FB, 2 * FB])
    # all blank; all distinct neighbours (count = T)
    assert _decode(torch.from_numpy(_from_labels(np.full((T,), blank), V))) == ([], [])
    lab = np.arange(T) % (V - 1)
    assert _decode(torch.from_numpy(_from_labels(lab, V))) == (lab.tolist(), list(range(T)))


@pytest.mark.parametrize("V", [34, 66, 257, 1025])
def test_exact_ties_take_the_first_maximum(V):
    rng = np.random.default_rng(V)
    T, blank = FB + 9, V - 1
    lp = rng.standard_normal((T, V)).astype(np.float32) - 8.0
    want = np.zeros((T,), dtype=np.int64)
    for t in range(T):
        kind = t % 4
        if kind == 0:                          # two equal maxima in different lanes of the wave (and different passes of its loop)
            a, b = sorted(rng.choice(V - 1, size=2, replace=False).tolist())
            if V > 64 and (b - a) % 64 == 0:
                b -= 1
            if a == b:
                b = a + 1
        elif kind == 1:                        # ... in the SAME lane of the wave-per-frame form: classes 64 apart
            a = int(rng.integers(0, max(V - 65, 1)))
            b = a + 64 if a + 64 < V else a + 1
        elif kind == 2:                        # blank ties with a token: the token is first
            a, b = int(rng.integers(0, blank)), blank
        else:                                  # every class equal: class 0
            lp[t, :] = 1.0
            a, b = 0, 0
        lp[t, a] = lp[t, b] = 2.0
        want[t] = a
    assert (lp.argmax(axis=1) == want).all()
    assert _decode(torch.from_numpy(lp)) == collapse_ref(want, blank)


@pytest.mark.parametrize("V", [34, 257])
def test_rows_of_minus_infinity_but_one_class(V):
    rng = np.random.default_rng(7 + V)
    T = FB + 40
    lab = rng.integers(0, V, size=T)
    lab[::5] = V - 1
    lp = np.full((T, V), -np.inf, dtype=np.float32)
    lp[np.arange(T), lab] = 0.0
    assert _decode(torch.from_numpy(lp)) == collapse_ref(lab, V - 1)


def test_a_shorter_call_after_a_longer_one_reads_no_stale_workspace():
    V = 34
    long_lp = _from_labels(np.arange(4 * FB + 3) % (V - 1), V)
    assert len(_decode(torch.from_numpy(long_lp))[0]) == 4 * FB + 3
    lab = np.full((FB + 1,), V - 1)
    lab[[3, FB]] = 2
    assert _decode(torch.from_numpy(_from_labels(lab, V))) == ([2, 2], [3, FB])
    assert _decode(torch.zeros((0, V))) == ([], [])


@pytest.mark.parametrize("V", [1, 1026])
def test_a_vocabulary_outside_the_limits_is_an_error(V):
    from gigaam_amd._lib import GigaAMHipError
    with pytest.raises(GigaAMHipError, match="V="):
        _op_engine().op_ctc_greedy_long(torch.zeros((4, V)))
