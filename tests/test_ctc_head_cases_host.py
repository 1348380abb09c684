"""Host: the inputs of the CTC head matrix (tests/ctc_head_cases.py, run on the GPU by tests/test_hip_ctc_head_matrix.py) judged by
the numpy / float64 reference alone -- what each case was built for holds before any kernel sees it.

No case is excused on the GPU: every frame of every label-built case has a float64 top-1 / top-2 margin over distinct classes above
MIN_MARGIN (2e-3, twice TOL_LOGP), so ids, frames and counts are compared exactly there; the share of frames left out of the exact
comparison is 0, which test_no_frame_is_excused states."""
import numpy as np
import pytest

from common import TOL_LOGP

import ctc_head_cases as K

_FRAMES = {"checked": 0, "excused": 0}


def _assert_case_is_clean(case):
    """The planted labels come back, with a margin: returns (labels, decoded)."""
    head = case["head"]
    lab, margin, dec = K.expected(case)
    assert np.array_equal(lab, K.canon(head)[case["planted"]]), (head, case["name"])
    assert margin > K.MIN_MARGIN, (head, case["name"], margin)
    _FRAMES["checked"] += lab.size
    return lab, dec


def test_constants():
    assert K.MIN_MARGIN == 2 * TOL_LOGP
    assert K.T_LIMIT == 15344                                        # (T' + 8 + 8) * 4 <= 60 KiB
    assert [K.thread_form(v) for v in K.TAP_V] == [True, True, True, False, False, False, False]
    assert not K.thread_form(K.PLANTED_V)
    for head in K.HEADS:
        w, b = K.head_wb(head)
        assert w.shape == (K.head_v(head), K.D_MODEL) and w.dtype == np.float32
        if K.is_tap(head):
            assert np.array_equal(w, np.eye(K.head_v(head), K.D_MODEL, dtype=np.float32)) and not b.any()
    pairs = set(K.TIE_PAIRS["tie"]) | set(K.TIE_PAIRS["tie_hi"])
    assert {(5, 37), (63, 64), (7, 71), (0, 1024), (700, 1024)} <= pairs
    for head, pp in K.TIE_PAIRS.items():
        w, b = K.head_wb(head)
        pw, pb = K.head_wb("planted")
        for lo, hi in pp:
            assert lo < hi and np.array_equal(w[lo], w[hi]) and b[lo] == b[hi]
        rest = np.setdiff1d(np.arange(K.PLANTED_V), [hi for _, hi in pp])
        assert np.array_equal(w[rest], pw[rest]) and np.array_equal(b[rest], pb[rest])      # the planted head otherwise


@pytest.mark.parametrize("head", K.HEADS)
def test_length_grid_reproduces_its_labels(head):
    V = K.head_v(head)
    for T in K.T_GRID:
        for which in K.GRID_BATCHES:
            case = K.grid_case(head, T, which)
            assert case["encoded"].shape == (4, K.D_MODEL, T) and case["encoded"].dtype == np.float32
            assert np.isfinite(case["encoded"]).all()
            lab, dec = _assert_case_is_clean(case)
            for b, n in enumerate(case["enc_len"]):
                n = K.clamp_len(n, T)
                ids, frames = dec[b]
                assert all(f < n for f in frames)
                # frames at t >= len peak at classes that are no blank and differ from their neighbours: a decode that forgets the
                # length emits every one of them
                tail = lab[b, n:]
                assert (tail != V - 1).all() or K.blank_is_tied(head)
                assert V == 2 or K.blank_is_tied(head) or (tail[1:] != tail[:-1]).all()
            if which == "a" and T >= 511:
                ids, frames = dec[0]
                assert 0 < len(ids) < T                                        # tokens and dropped frames both occur
                if not K.blank_is_tied(head):
                    assert (lab[0] == V - 1).sum() > T // 5                    # about a third of the frames are blank
                for p in K.BORDERS:                                            # tokens on both sides of each pass border
                    if T > p:
                        assert any(f < p for f in frames) and any(f >= p for f in frames), (head, T, p)
                        assert any(p - K.NT <= f < p for f in frames), (head, T, p)


@pytest.mark.parametrize("head", K.HEADS)
def test_pass_border_rows(head):
    V = K.head_v(head)
    case = K.border_case(head)
    lab, dec = _assert_case_is_clean(case)
    if K.blank_is_tied(head):      # the blank of these heads ties with a class, which wins: the rows are still decoded on the GPU
        return
    k = min(3, V - 2)
    k2 = (k + 1) % (V - 1)
    early = ([k, k, k], [2, 40, 300])
    want = {
        "same": ([k, k], [511, 1023]),
        "label-blank-label": ([k] * 4, [510, 512, 1022, 1024]),
        "blank-behind": ([k] * 4, [511, 513, 1023, 1025]),
        "different": ([k, k2, k, k2], [511, 512, 1023, 1024]) if V > 2 else ([k, k], [511, 1023]),
        "run-starts": ([k, k], [512, 1024]),
        "cut-512": ([k], [510]),
        "cut-513": ([k], [510]),
        "starts-cut-512": ([], []),
        "starts-cut-513": ([k], [512]),
    }
    for r, row in enumerate(K.BORDER_ROWS):
        assert dec[r] == (early[0] + want[row][0], early[1] + want[row][1]), (head, row, dec[r])


@pytest.mark.parametrize("head", K.HEADS)
def test_extreme_rows(head):
    V, T = K.head_v(head), K.T_BORDER
    case = K.extreme_case(head)
    lab, dec = _assert_case_is_clean(case)
    if K.blank_is_tied(head):
        return
    assert dec[0] == ([], [])
    assert dec[1] == ([min(3, V - 2)], [0])
    if V > 2:
        assert dec[2] == ((np.arange(T) % (V - 1)).tolist(), list(range(T)))    # count = len: the result buffers are full
    else:
        assert dec[2] == ([0], [0])


def test_limit_case():
    case = K.limit_case()
    assert case["encoded"].shape == (1, K.D_MODEL, K.T_LIMIT)
    lab, dec = _assert_case_is_clean(case)
    assert 0 < len(dec[0][0]) < K.T_LIMIT and dec[0][1][-1] > K.T_LIMIT - K.NT     # tokens in the last of the 30 passes


@pytest.mark.parametrize("V", K.TAP_V)
def test_tie_rows_are_exact_ties_in_float32(V):
    case = K.tie_case(f"tap{V}")
    names = {name for name, _, _ in case["rows"]}
    assert {"negative-max-at-0", "last-pair", "blank-and-0", "constant", "all-lowest"} <= names
    if V >= 4:
        assert {"two", "three", "blank-and-lower", "lanes-v-v+1"} <= names
    if V % 2 == 0 and V >= 4:
        assert "pair-halves" in names
    assert ("lanes-v-v+32" in names) == (V > 33) and ("lanes-v-v+64" in names) == (V > 65)
    for name, row, classes in case["rows"]:
        assert row.dtype == np.float32 and row.shape == (V,) and np.isfinite(row).all()
        assert np.nonzero(row == row.max())[0].tolist() == classes, (V, name)      # these classes, and no other, hold the maximum
        assert int(np.argmax(row)) == classes[0] and classes[0] != V - 1, (V, name)     # the winner is never the blank
        if name == "pair-halves":
            assert classes[0] % 2 == 0 and classes[1] == classes[0] + 1
        if name == "negative-max-at-0":
            assert row.max() < 0 and classes == [0]
    enc, want = case["encoded"], case["want"]
    lg = np.ascontiguousarray(enc[:, :V, :].transpose(0, 2, 1))
    assert np.array_equal(lg.argmax(axis=2), want)
    # every tie row stands between two blank frames: its label is emitted on its own, none is hidden by the collapse
    dec = K.decode_ref(want, case["enc_len"], V - 1)
    for b in range(2):
        assert dec[b][1] == list(range(1, want.shape[1], 2)) and dec[b][0] == want[b, 1::2].tolist()
    _FRAMES["checked"] += want.size


@pytest.mark.parametrize("head", K.HEADS)
def test_log_prob_rows_are_what_they_are_named(head):
    for shape in K.LOGP_SHAPES:
        enc, kind_of = K.logp_case(head, shape)
        assert enc.shape == (shape[0], K.D_MODEL, shape[1]) and np.isfinite(enc).all()
        lg = K.logits64(head, enc)
        spread = lg.max(axis=2) - lg.min(axis=2)
        assert {k for k in kind_of.ravel()} == set(K.logp_kinds(head))
        assert (spread[kind_of == "spread0"] == 0).all()
        assert (spread[kind_of == "underflow"] > 104).all()               # exp(-104) is below float32's smallest subnormal
        assert (lg[kind_of == "near1e4"] > 9990).all()
        lp = K.log_softmax64(lg)
        assert np.abs(K.logsumexp64(lp)).max() < 1e-12


@pytest.mark.parametrize("nc", K.EMO_NC)
def test_emotion_cases(nc):
    for T in K.EMO_T:
        enc, lens = K.emo_case(nc, T, True)
        assert lens == [T, 1, 0, T + 5, 64, 65]
        for b, n in enumerate(lens):
            n = min(max(n, 1), T)
            assert np.isfinite(enc[b, :, :n]).all() and (np.abs(enc[b, :, :n]) < 10).all() and (enc[b, :, n:] == np.float32(1e30)).all()
        p = K.emo_ref(nc, enc, lens)
        assert p.shape == (len(lens), nc) and np.abs(p.sum(axis=1) - 1).max() < 1e-12
        enc2, none = K.emo_case(nc, T, False)
        assert none is None and np.abs(K.emo_ref(nc, enc2, None).sum(axis=1) - 1).max() < 1e-12
        if nc > 1 and T > 1:
            assert np.abs(p[0] - p[1]).max() > 1e-3                          # the length matters to the result


def test_no_frame_is_excused():
    """Runs last: every frame of every case above entered the exact comparison."""
    assert _FRAMES["checked"] > 0 and _FRAMES["excused"] == 0
    print(f"frames checked {_FRAMES['checked']}, left out of the exact comparison: {_FRAMES['excused']} (share 0)")
