"""CPU: the float64 reference of transducer forced alignment (tests/rnnt_align_ref.py) against independent statements of the same
quantities -- rnnt_beam_ref.exact_loglik with a cap that never binds, brute-force enumeration of every lattice path -- on the golden
RNN-T cases, and the argument checks of the Python layers that need no GPU."""
import numpy as np
import pytest
import torch

from beam_common import small_sd
from common import load_case, split_ragged

import rnnt_align_ref as A
import rnnt_beam_ref as R

RNNT_CASES = ["v1_rnnt_l2", "v2_rnnt_l2", "v3_rnnt_l2", "v3_e2e_rnnt_l2", "v2_rnnt_l2_dense", "v2_rnnt_l2_lstm2", "v3_e2e_rnnt_l2_dense"]
# Cases where the reference's best path of the golden greedy ids IS the greedy decode's on at least one utterance.  Measured here
# with the reference alone: it is on none of the three utterances of v2_rnnt_l2_dense, v2_rnnt_l2_lstm2 and v3_e2e_rnnt_l2_dense
# (emission-heavy joints: the greedy decode, one argmax at a time under its symbol cap, is not the optimum of its own transcript).
GREEDY_IS_BEST = ["v1_rnnt_l2", "v2_rnnt_l2", "v3_rnnt_l2", "v3_e2e_rnnt_l2"]


@pytest.mark.parametrize("L", [1, 2])
def test_reference_loglik_equals_the_capped_dp_when_the_cap_never_binds(L):
    """exact_loglik's S = len(y) + 1 symbols per frame can never be reached by len(y) tokens: it is then the transducer loss."""
    rng = np.random.default_rng(40 + L)
    V = 5
    head = R.head_from_state_dict(small_sd(rng, V, L=L), L)
    n = 0
    for T in (1, 2, 4, 6):
        for U in (0, 1, 3, 5):
            y = rng.integers(0, V - 1, U).tolist()
            encp = rng.standard_normal((T, 8)) * 0.7
            pred = R.Predictor(head)
            joint = lambda t, p: R.joint_lp(head, encp[t], pred(p))     # noqa: E731
            lat = A.lattice(head, encp, y, T)
            want = R.exact_loglik(joint, y, T, len(y) + 1)
            got = A.forward_loglik(lat)
            assert got == pytest.approx(want, abs=1e-10), (T, y)
            assert np.allclose(lat, A.lattice_from_joint(joint, y, T), rtol=0, atol=1e-12)      # (a frame's rows in one product)
            for S in (1, 2, len(y) + 1):      # the decoders' capped model on the same lattice
                assert A.capped_loglik(lat, S) == pytest.approx(R.exact_loglik(joint, y, T, S), abs=1e-10), (T, y, S)
            score, fr, ok = A.viterbi(lat)
            assert ok and score <= got + 1e-12 and A.valid_path(fr, T)
            assert A.rescore(lat, fr) == pytest.approx(score, abs=1e-10)
            n += 1
    assert n == 16


@pytest.mark.parametrize("ties", [False, True])
def test_reference_viterbi_equals_brute_force(ties):
    rng = np.random.default_rng(11 if ties else 5)
    n, tied = 0, 0
    for T in range(1, 6):
        for U in range(0, 5):
            for _ in range(3):
                if ties:    # dyadic values: exact sums, many equal paths
                    lat = rng.choice([0.0, -0.5, -1.0, -2.0], size=(T, U + 1, 2))
                else:
                    lat = np.log(rng.dirichlet(np.ones(3), size=(T, U + 1)))[..., :2]
                score, fr, ok = A.viterbi(lat)
                best, tot, paths = A.brute_force(lat)
                assert ok and score == pytest.approx(best, abs=1e-12)
                assert A.forward_loglik(lat) == pytest.approx(tot, abs=1e-9)
                assert fr == A.tie_rule_path(paths), (T, U, lat)
                tied += len(paths) > 1
                n += 1
    assert n == 75 and (tied >= 10 if ties else tied == 0)


def test_reference_edge_cases():
    assert A.viterbi(np.zeros((0, 1, 2))) == (0.0, [], True) and A.forward_loglik(np.zeros((0, 1, 2))) == 0.0
    assert A.viterbi(np.zeros((0, 3, 2))) == (-np.inf, [], False) and A.forward_loglik(np.zeros((0, 3, 2))) == -np.inf
    lat = np.full((2, 2, 2), -1.0)
    lat[:, 0, 1] = -np.inf        # the only token can never be emitted
    assert A.viterbi(lat) == (-np.inf, [], False) and A.forward_loglik(lat) == -np.inf
    # T = 1, U = 3: every token in the one frame
    lat = np.log(np.full((1, 4, 2), 0.25))
    score, fr, ok = A.viterbi(lat)
    assert ok and fr == [0, 0, 0] and score == pytest.approx(4 * np.log(0.25))
    assert not A.valid_path([1, 0], 3) and not A.valid_path([0, 3], 3) and A.valid_path([], 0)


@pytest.mark.parametrize("name", RNNT_CASES)
def test_reference_viterbi_reproduces_golden_greedy_frames(name):
    """Aligning the golden greedy ids with the reference: the likelihood bounds the best path, the best path scores no less than
    the greedy decode's, and on at least one utterance of every GREEDY_IS_BEST case the best path IS the greedy decode's (the
    condition tests/test_hip_rnnt_align.py asks of the kernel)."""
    ck, _, _, gold = load_case(name)
    L = ck["cfg"]["head"]["decoder"]["pred_rnn_layers"]
    head = R.head_from_state_dict(ck["state_dict"], L)
    rows = split_ragged(gold["ids"], gold["frames"], gold["counts"].tolist())
    same = 0
    for b, (ids, frames) in enumerate(rows):
        T = int(gold["enc_len"][b])
        lat = A.lattice(head, R.encoder_projection(head, gold["encoded"][b]), ids, T)
        score, fr, ok = A.viterbi(lat)
        assert ok and A.forward_loglik(lat) >= score
        assert score >= A.rescore(lat, frames) - 1e-9      # the greedy path is a lattice path
        same += fr == frames
    assert same >= 1 or name not in GREEDY_IS_BEST, name


def _model(decoding):
    from gigaam_amd.model import GigaAMASR
    m = GigaAMASR.__new__(GigaAMASR)
    object.__setattr__(m, "decoding", decoding)
    return m


def test_rnnt_align_argument_checks_need_no_gpu():
    from gigaam_amd import synth
    from gigaam_amd.decoding import CTCGreedyDecoding, RNNTBeamDecoding, RNNTGreedyDecoding
    wav, lens = torch.zeros((2, 1600)), torch.tensor([1600, 1600])
    ctc = _model(CTCGreedyDecoding(synth.CHAR_VOCAB))
    with pytest.raises(TypeError, match="transducer alignment needs an RNN-T head"):
        ctc.rnnt_align_batch(wav, lens, ["а", "б"])
    with pytest.raises(TypeError, match="transducer alignment needs an RNN-T head"):
        ctc.rnnt_align("missing.wav", "а")
    for dec in (RNNTGreedyDecoding(synth.CHAR_VOCAB), RNNTBeamDecoding(synth.CHAR_VOCAB, beam_size=4)):
        m = _model(dec)
        with pytest.raises(TypeError, match="forced alignment needs a CTC head"):
            m.align_batch(wav, lens, ["а", "б"])
        with pytest.raises(ValueError, match="1 texts for a batch of 2"):
            m.rnnt_align_batch(wav, lens, ["а"])
        with pytest.raises(ValueError, match="characters not in the vocabulary"):
            m.rnnt_align_batch(wav, lens, ["а", "q~"])
        with pytest.raises(ValueError, match="at most 1024 tokens"):
            dec.align(None, None, None, [[0] * 1025])
