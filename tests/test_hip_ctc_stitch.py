"""GPU, op level: gam_op_ctc_stitch (gigaam_amd/csrc/gam_stitch.h) -- the kept rows of every window's log-probs copied into one
[T_total, V] stream -- bit for bit against numpy slicing.  ``out`` is a slice of a larger buffer prefilled with a sentinel: the rows in
front of it and behind it are guards, and every row the plan does not name must still hold the sentinel afterwards."""
import numpy as np
import pytest
import torch

from test_hip_ctc_align import _op_engine

pytestmark = pytest.mark.gpu

TP = 37
GUARD = 3                      # an odd number of guard rows: with V = 34 `out` starts 8 bytes off a 16-byte boundary
SENTINEL = -12345.5


def _expected(big, lp, enc_len, lo, hi, dst, t_total):
    """The contract in numpy, applied to the guarded buffer ``big`` in place -> status."""
    out = big[GUARD:GUARD + t_total]
    status = []
    for b in range(lp.shape[0]):
        n_valid = min(max(int(enc_len[b]), 0), lp.shape[1])
        l, h, d = int(lo[b]), int(hi[b]), int(dst[b])
        if h <= l:
            status.append(1)
            continue
        lc, hc = max(l, 0), min(h, n_valid)
        ok = int(l >= 0 and h <= n_valid)
        n = max(hc - lc, 0)
        d0 = d + lc - l
        if n and (d0 < 0 or d0 + n > t_total):
            ok, n = 0, 0
        out[d0:d0 + n] = lp[b, lc:lc + n]
        status.append(ok)
    return status


def _run(lp, enc_len, lo, hi, dst, t_total, big=None):
    eng = _op_engine()
    B, _, V = lp.shape
    if big is None:
        big = np.full((t_total + 2 * GUARD, V), SENTINEL, dtype=np.float32)
    big_dev = torch.from_numpy(big).to("cuda:0")
    status = eng.op_ctc_stitch(torch.from_numpy(lp), torch.tensor(enc_len, dtype=torch.int32), torch.tensor(lo, dtype=torch.int32),
                               torch.tensor(hi, dtype=torch.int32), torch.tensor(dst, dtype=torch.int64),
                               big_dev[GUARD:GUARD + t_total])
    want = big.copy()
    want_status = _expected(want, lp, enc_len, lo, hi, dst, t_total)
    got = big_dev.cpu().numpy()
    assert status.dtype == torch.int32 and status.cpu().tolist() == want_status
    assert (got.view(np.int32) == want.view(np.int32)).all()
    return got, want_status


def _lp(B, V, seed):
    return np.random.default_rng(seed).standard_normal((B, TP, V)).astype(np.float32)


def _ragged(B):
    return [TP, 29, 36, 1, 30][:B]


@pytest.mark.parametrize("V", [34, 257, 1025])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_a_tiling_plan_is_copied_bit_for_bit(B, V):
    lp, enc_len = _lp(B, V, 10 * B + V), _ragged(B)
    lo = [0, 3, 2, 0, 5][:B]                       # odd and even first rows: every access width at V = 34
    hi = list(enc_len)
    hi[0] = TP - 4
    dst, t = [], 1                                 # row 0 of `out` stays unplanned, and one row between windows 0 and 1
    for b in range(B):
        dst.append(t + (1 if b == 1 else 0))
        t = dst[-1] + max(hi[b] - lo[b], 0)
    t_total = t + 2
    got, status = _run(lp, enc_len, lo, hi, dst, t_total)
    assert status == [1] * B
    out = got[GUARD:GUARD + t_total]
    assert (out[0] == SENTINEL).all() and (out[t:] == SENTINEL).all()
    assert (out[dst[0]:dst[0] + hi[0]] == lp[0, :hi[0]]).all()


@pytest.mark.parametrize("V", [34, 257, 1025])
def test_clipped_and_empty_and_misplaced_windows(V):
    B = 5
    lp, enc_len = _lp(B, V, 77 + V), _ragged(B)
    lo = [4, 10, 0, 0, 7]
    hi = [4, 33, 36, 0, 7 + 23]                    # empty (hi == lo) | hi > enc_len = 29: clipped | whole | empty (hi < ... = 0) | fits
    dst = [0, 2, 100, 0, 21]                       # window 2 (36 rows at 100) ends past T_total = 120: nothing of it is written
    got, status = _run(lp, enc_len, lo, hi, dst, 120)
    assert status == [1, 0, 0, 1, 1]
    out = got[GUARD:GUARD + 120]
    assert (out[2:21] == lp[1, 10:29]).all() and (out[21:44] == lp[4, 7:30]).all() and (out[44:] == SENTINEL).all()
    # the same window placed in front of row 0, one row past the end, and exactly at the end
    for d, ok in ((-1, 0), (120 - 36 + 1, 0), (120 - 36, 1)):
        _, status = _run(lp[2:3], enc_len[2:3], [0], [36], [d], 120)
        assert status == [ok]
    # a negative first row is clipped: the valid rows land where the plan puts them
    _, status = _run(lp[:1], [TP], [-2], [5], [10], 120)
    assert status == [0]


@pytest.mark.parametrize("V", [34, 257])
def test_two_calls_fill_one_stream(V):
    lp_a, lp_b = _lp(3, V, 5), _lp(2, V, 6)
    t_total = 3 * 20 + 2 * 15
    big = np.full((t_total + 2 * GUARD, V), SENTINEL, dtype=np.float32)
    got, status = _run(lp_a, [TP] * 3, [5] * 3, [25] * 3, [0, 20, 40], t_total, big)
    assert status == [1] * 3
    got, status = _run(lp_b, [TP, 16], [1, 1], [16, 16], [60, 75], t_total, got.copy())
    assert status == [1] * 2
    want = np.concatenate([lp_a[0, 5:25], lp_a[1, 5:25], lp_a[2, 5:25], lp_b[0, 1:16], lp_b[1, 1:16]])
    assert (got[GUARD:GUARD + t_total].view(np.int32) == want.view(np.int32)).all()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + t_total:] == SENTINEL).all()
