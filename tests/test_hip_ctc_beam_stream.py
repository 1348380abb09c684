"""GPU: the resumable CTC prefix beam search (gam_op_ctc_beam_stream, gam_ctc_beam_stream_kernel in gigaam_amd/csrc/gam_beam_stream.h):
one call against the batch kernel bit for bit, split invariance, streams past the batch kernel's 8192 frames and across the rebase
frames against the float64 reference (tests/ctc_beam_ref.py, tests/ctc_lm_ref.py), two interleaved streams, the side-stream launch
and every refusal.

Margin rule (tests/test_hip_ctc_beam.py): the kernel ranks in fp32, the reference in fp64, so ids / frames are exact only where the
reference's smallest decision margin exceeds MARGIN (<= 40 frames) / MARGIN_LONG (beyond).  Every input below is chosen so that it
does: a case that misses its margin FAILS."""
import struct

import numpy as np
import pytest
import torch

from beam_common import bar as _bar, ctc_hotwords as _hotwords, ctc_op_engine, log_probs as _log_probs, run_ctc_op as _run_op
from beam_common import tokenizer as _tokenizer
from common import report

import ctc_beam_ref as R
import test_hip_ctc_beam_lm as TL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BEGIN, END = 1, 2
MARGIN = 2e-5
MARGIN_LONG = 1e-4
BOOST, ALPHA, BETA = 1.5, 0.8, 0.6


def _op_engine():
    return ctc_op_engine(__name__)


def _rebase():
    from gigaam_amd.engine import HipEngine
    return HipEngine.BEAM_STREAM_REBASE


def _dev(lp):
    return torch.from_numpy(np.ascontiguousarray(lp, dtype=np.float32)).to(DEV)


def _result(eng, s, check=True):
    """The stream's result as it is on the device now (not through ``finish``: no call is made)."""
    return eng._finish(s.out, False).host(check)


def _single(eng, lp, W, max_frames=None):
    """ONE call with BEGIN | END over the whole stream."""
    T, V = lp.shape
    s = eng.beam_stream(W, T if max_frames is None else max_frames)
    eng.op_ctc_beam_stream(_dev(lp) if T else None, V, 0, BEGIN | END, W, s.state, s.out)
    return _result(eng, s)


def _pieces(eng, lp, W, cuts, overlap=False):
    """The stream fed in the pieces that ``cuts`` make (a repeated cut: a call with n = 0), END as a call of its own."""
    s = eng.beam_stream(W, lp.shape[0])
    x, edges = _dev(lp), [0] + [int(c) for c in cuts] + [lp.shape[0]]
    for a, b in zip(edges[:-1], edges[1:]):
        s.push(x[a:b], overlap=overlap)
    h = s.finish().host()
    torch.cuda.synchronize()
    assert s.t_next == lp.shape[0] and s.ended
    return h


def _bits(x):
    return struct.pack("<d", x)


def _same(a, b):
    assert a["count"] == b["count"] and a["status"] == b["status"] == 1
    assert a["ids"].tolist() == b["ids"].tolist() and a["frames"].tolist() == b["frames"].tolist()
    assert _bits(a["score"]) == _bits(b["score"]) and _bits(a["logp"]) == _bits(b["logp"]), (a["score"], b["score"], a["logp"], b["logp"])


def _same_as_batch(eng, got, lp, W):
    """ids, frames, count, and score / logp once rounded to f32, against ``op_ctc_beam`` on the same rows as one utterance."""
    want = _run_op(eng, lp[None], [lp.shape[0]], W)
    ids, frames = want["rows"][0]
    assert got["status"] == 1 and got["count"] == len(ids)
    assert got["ids"].tolist() == ids and got["frames"].tolist() == frames
    for k in ("score", "logp"):
        assert np.float32(got[k]).tobytes() == want[k][0].tobytes(), (k, got[k], float(want[k][0]))


def _against_reference(got, ref, margin, errs):
    m = R.min_margin(ref)
    assert m > margin, f"the reference's smallest margin {m:.3e} does not exceed {margin:.0e}: choose another input"
    assert got["ids"].tolist() == ref["ids"] and got["frames"].tolist() == ref["frames"]
    for k in ("score", "logp"):
        e = abs(got[k] - ref[k])
        errs[k] = max(errs.get(k, 0.0), e / max(1.0, abs(ref[k])))
        print(f"{k}: got {got[k]!r} reference {ref[k]!r} error {e:.3e} bar {_bar(ref[k]):.3e} (margin {m:.3e})")
        assert e <= _bar(ref[k]), (k, got[k], ref[k])


class _Setup:
    """Hotwords and / or an LM on the op engine for the time of a test; cleared behind it."""

    def __init__(self, eng, tmp_path, rng, lp, mode, n_hot=8, order=3, n_words=40):
        V = lp.shape[1]
        self.eng, self.phrases, self.spec = eng, [], None
        if "hot" in mode:
            self.phrases = _hotwords(rng, lp[None], n_hot)
        self.lm = None
        if "lm" in mode:
            self.tok = _tokenizer(V)
            classes = TL.token_classes(self.tok)
            self.lm, self.spec = TL._make_lm(tmp_path, rng, self.tok, TL._word_ids(rng, lp[None], classes, n_words), order, ALPHA, BETA)

    def __enter__(self):
        self.eng.set_hotwords(self.phrases, BOOST)
        if self.lm is not None:
            self.eng.set_lm(self.lm, self.tok, ALPHA, BETA)
        else:
            self.eng.set_lm(None)
        return self

    def __exit__(self, *exc):
        self.eng.set_lm(None)
        self.eng.set_hotwords([])

    def reference(self, lp, W):
        return R.beam_search(lp, W, lp.shape[0], self.phrases, BOOST, self.spec)


# (T, V, W, kind): T in {1, 2, 40}, V in {2, 34, 257, 1025}, W in {1, 4, 8, 32}, peaked and flat -- a few shapes per axis
ONE_CALL = [(1, 2, 1, "flat"), (2, 2, 32, "flat"), (2, 34, 4, "peaked"), (40, 34, 8, "peaked"), (40, 34, 8, "flat"), (40, 34, 1, "flat"),
            (40, 257, 32, "flat"), (1, 257, 4, "peaked"), (40, 1025, 32, "peaked"), (40, 1025, 4, "flat")]


# (V = 2 has one non-blank id: no two-best hotword picker and no tokenizer, so it runs plain only)
ONE_CALL_MODES = [c + (m,) for c in ONE_CALL for m in ("plain", "hot", "lm", "hot+lm") if c[1] > 2 or m == "plain"]


@pytest.mark.parametrize("T,V,W,kind,mode", ONE_CALL_MODES)
def test_one_call_equals_the_batch_kernel_bit_for_bit(tmp_path, T, V, W, kind, mode):
    """Check 1."""
    eng = _op_engine()
    rng = np.random.default_rng(T * 100000 + V * 40 + W + len(kind) + len(mode))
    lp = _log_probs(rng, 1, T, V, kind)[0]
    with _Setup(eng, tmp_path, rng, lp, mode):
        got = _single(eng, lp, W)
        _same_as_batch(eng, got, lp, W)
        # a pool for more frames than the stream has changes nothing
        _same(_single(eng, lp, W, max_frames=T + 3), got)


@pytest.mark.parametrize("mode", ["plain", "hot+lm"])
def test_a_stream_without_a_frame_is_empty(tmp_path, mode):
    """Check 1, T = 0: count 0, score = logp = 0 -- in one call, and with BEGIN, an n = 0 call and END apart."""
    eng = _op_engine()
    rng = np.random.default_rng(3)
    lp = _log_probs(rng, 1, 8, 34, "flat")[0]
    with _Setup(eng, tmp_path, rng, lp, mode):
        for got in (_single(eng, lp[:0], 4, max_frames=0), _single(eng, lp[:0], 4, max_frames=5), _pieces(eng, lp[:0], 4, [0, 0])):
            assert (got["status"], got["count"], got["score"], got["logp"]) == (1, 0, 0.0, 0.0) and got["ids"].shape == (0,)
        # the batch kernel's enc_len = 0
        want = _run_op(eng, lp[None], [0], 4)
        assert want["rows"][0] == ([], []) and float(want["score"][0]) == 0.0 == float(want["logp"][0])


def _cuttings(T, seed):
    fixed = [c for c in (0, 1, 2, 5, 39) if c <= T]       # pieces of 0, 1, 1, 3, 34 frames and the rest, and an n = 0 call in the middle
    rng = np.random.default_rng(seed)
    return [sorted(fixed + [fixed[len(fixed) // 2]])] + [sorted(rng.integers(0, T + 1, int(rng.integers(1, 10))).tolist()) for _ in range(3)]


@pytest.mark.parametrize("V,W,kind", [(34, 8, "flat"), (34, 4, "peaked"), (257, 32, "flat")])
def test_any_cutting_gives_the_bits_of_the_single_call(tmp_path, V, W, kind):
    """Check 2, hotwords and LM on: the fixed cuts with an n = 0 call in the middle and END as a call of its own, three random ones.
    The single call is also held against the float64 reference: its smallest margins here are 1.4e-4, 5.8e-2 and 1.1e-4 (measured on
    the CPU), above MARGIN."""
    eng = _op_engine()
    T = 40
    rng = np.random.default_rng(V + W)
    lp = _log_probs(rng, 1, T, V, kind)[0]
    with _Setup(eng, tmp_path, rng, lp, "hot+lm") as st:
        want = _single(eng, lp, W)
        _same_as_batch(eng, want, lp, W)
        assert want["count"] > 0
        for cuts in _cuttings(T, V * W):
            _same(_pieces(eng, lp, W, cuts), want)
        _against_reference(want, st.reference(lp, W), MARGIN, {})


LONG_T, LONG_V, LONG_SEED, LONG_BOOST = 9000, 34, 0, 2.0


@pytest.fixture(scope="module")
def long_case():
    """T = 9000 > the batch kernel's 8192, V = 34, peaked, seed 0; 20 hotword phrases drawn from the same generator behind the
    log-probs."""
    rng = np.random.default_rng(LONG_SEED)
    lp = _log_probs(rng, 1, LONG_T, LONG_V, "peaked")[0]
    return lp, _hotwords(rng, lp[None], 20)


def _long_cuts():
    r = _rebase()
    return [[r], [r + 1], [8192], [8193], [r, r + 1, 8192, 8193]]      # R-1 | R, R | R+1, 8191 | 8192, 8192 | 8193, and all of them


def test_a_stream_past_8192_frames_matches_the_float64_reference(long_case):
    """Check 3, W = 4: one call, and every cutting at a rebase frame and at the batch kernel's frame limit gives its bits."""
    eng = _op_engine()
    lp, _ = long_case
    ref = R.beam_search(lp, 4)      # (smallest margin 3.4e-3, measured on the CPU; about 5 s there)
    eng.set_hotwords([])
    eng.set_lm(None)
    one = _single(eng, lp, 4)
    assert one["count"] > 4000 and int(one["frames"].max()) > 8192
    errs = {}
    _against_reference(one, ref, MARGIN_LONG, errs)
    for cuts in _long_cuts():
        _same(_pieces(eng, lp, 4, cuts), one)
    report("ctc_beam_stream_long", **errs)


def test_a_stream_past_8192_frames_with_hotwords_matches_the_float64_reference(long_case):
    """Check 3, W = 8 with 20 hotword phrases at the default boost 2.0: the committed bonus (422 at the end) is rebased eight times."""
    eng = _op_engine()
    lp, phrases = long_case
    ref = R.beam_search(lp, 8, LONG_T, phrases, LONG_BOOST)      # (smallest margin 3.2e-4, measured on the CPU; about 20 s there)
    eng.set_lm(None)
    eng.set_hotwords(phrases, LONG_BOOST)
    try:
        one = _single(eng, lp, 8)
        errs = {}
        _against_reference(one, ref, MARGIN_LONG, errs)
        assert abs(one["score"] - one["logp"]) >= 100.0      # the score carries the committed bonus, offsets included
        for cuts in _long_cuts():
            _same(_pieces(eng, lp, 8, cuts), one)
    finally:
        eng.set_hotwords([])
    report("ctc_beam_stream_long_hotwords", **errs)


REBASE_SEED, REBASE_V, REBASE_W = 1, 34, 8      # the reference's smallest margin: 5.7e-3 (seeds 2 .. 5: 5.0e-4, 4.0e-3, 8.8e-3, 9.7e-5)


def _offsets(s):
    """(off, cb_off, lm_off) of a stream's state record (gam_beam_stream.h GamBeamStreamHdr: three f64 from byte 48)."""
    return tuple(s.state[12:18].cpu().numpy().view(np.float64).tolist())


def test_the_rebase(tmp_path):
    """Check 4: 2 R + 100 frames with an LM and hotwords against the float64 reference (two rebases; both offsets have moved), and
    on the same input a stream of R frames -- the longest without a rebase -- against the batch kernel bit for bit.
    Seed 1: the reference's smallest margin is 5.7e-3, its LM term -270.6 and its committed bonus 57.0, measured on the CPU."""
    eng = _op_engine()
    r = _rebase()
    T = 2 * r + 100
    rng = np.random.default_rng(REBASE_SEED)
    lp = _log_probs(rng, 1, T, REBASE_V, "peaked")[0]
    with _Setup(eng, tmp_path, rng, lp, "hot+lm", n_hot=20, n_words=120) as st:
        ref = st.reference(lp, REBASE_W)
        s = eng.beam_stream(REBASE_W, T)
        s.push(_dev(lp))
        got = s.finish().host()
        errs = {}
        _against_reference(got, ref, MARGIN_LONG, errs)
        off, cb_off, lm_off = _offsets(s)
        print(f"offsets: off {off!r} cb_off {cb_off!r} lm_off {lm_off!r}; reference lm term {ref['lm']!r}")
        assert cb_off != 0.0 and lm_off != 0.0 and abs(ref["lm"]) > 100.0
        for cuts in ([r], [r + 1], [2 * r - 1, 2 * r, 2 * r + 1]):
            _same(_pieces(eng, lp, REBASE_W, cuts), got)
        # no rebase below R: frames 0 .. R - 1 are the batch kernel's arithmetic, and nothing has reached the offsets
        s = eng.beam_stream(REBASE_W, r)
        s.push(_dev(lp[:r]))
        short = s.finish().host()
        _same_as_batch(eng, short, lp[:r], REBASE_W)
        assert _offsets(s)[1:] == (0.0, 0.0)
    report("ctc_beam_stream_rebase", **errs)


def test_two_streams_pushed_alternately_through_two_states(tmp_path):
    """Check 5."""
    eng = _op_engine()
    rng = np.random.default_rng(55)
    T, V, W = 150, 34, 8
    lps = [_log_probs(rng, 1, T, V, "flat")[0] for _ in range(2)]
    with _Setup(eng, tmp_path, rng, lps[0], "hot+lm"):
        want = [_single(eng, lp, W) for lp in lps]
        assert want[0]["ids"].tolist() != want[1]["ids"].tolist()
        ss = [eng.beam_stream(W, T), eng.beam_stream(W, T)]
        xs = [_dev(lp) for lp in lps]
        edges = ([0, 10, 64, 65, 150], [0, 70, 71, 128, 150])
        for i in range(4):
            for j in (0, 1):
                ss[j].push(xs[j][edges[j][i]:edges[j][i + 1]])
        for j in (0, 1):
            _same(ss[j].finish().host(), want[j])


def test_side_stream_pushes_equal_launch_stream_pushes(tmp_path):
    """Check 6."""
    eng = _op_engine()
    rng = np.random.default_rng(66)
    T, V, W = 1500, 34, 8
    lp = _log_probs(rng, 1, T, V, "peaked")[0]
    with _Setup(eng, tmp_path, rng, lp, "hot+lm"):
        cuts = [100, 1023, 1024, 1400]
        a = _pieces(eng, lp, W, cuts, overlap=False)
        b = _pieces(eng, lp, W, cuts, overlap=True)
        _same(b, a)
        assert a["count"] > 100


STATUS_WORD = 5      # engine.BeamStreamDecoded: score | logp | count | status


def test_the_kernel_refuses_calls_that_do_not_continue_the_stream(tmp_path):
    """Check 7: status 0, every output and the state unchanged; behind a refused call the right call carries on."""
    from gigaam_amd._lib import GigaAMHipError
    eng = _op_engine()
    rng = np.random.default_rng(77)
    T, V, W = 90, 34, 8
    lp = _log_probs(rng, 1, T, V, "flat")[0]
    x = _dev(lp)
    x35 = _dev(_log_probs(rng, 1, T, V + 1, "flat")[0])
    tok = _tokenizer(V)
    lm, _ = TL._make_lm(tmp_path, rng, tok, TL._word_ids(rng, lp[None], TL.token_classes(tok), 40), 3, ALPHA, BETA)
    phrases, other = _hotwords(rng, lp[None], 8), _hotwords(rng, lp[None], 8)
    assert phrases != other
    eng.set_lm(None)
    eng.set_hotwords(phrases, BOOST)
    try:
        want = _single(eng, lp, W)

        def refused(s, call):
            torch.cuda.synchronize()
            state, whole = s.state.clone(), s.out.whole.clone()
            s.out.status.fill_(5)
            call()
            assert _result(eng, s, check=False)["status"] == 0
            s.out.status.copy_(whole[STATUS_WORD:STATUS_WORD + 1])
            torch.cuda.synchronize()
            assert torch.equal(s.state, state) and torch.equal(s.out.whole[:-1], whole[:-1])

        op = eng.op_ctc_beam_stream
        # no BEGIN, on a zeroed state
        s = eng.beam_stream(W, T)
        s.out.whole.fill_(-7)
        refused(s, lambda: op(x[:40], V, 0, 0, W, s.state, s.out))
        refused(s, lambda: op(None, V, 0, END, W, s.state, s.out))
        s.push(x[:40])
        # a frame skipped or repeated
        refused(s, lambda: op(x[40:], V, 41, 0, W, s.state, s.out))
        refused(s, lambda: op(x[40:], V, 39, END, W, s.state, s.out))
        refused(s, lambda: op(None, V, 0, 0, W, s.state, s.out))
        # another W (narrower: the pool holds it; wider: it does not), another V
        refused(s, lambda: op(x[40:], V, 40, 0, 4, s.state, s.out))
        refused(s, lambda: op(x[40:], V, 40, 0, 16, s.state, s.out))
        refused(s, lambda: op(x35[40:], V + 1, 40, 0, W, s.state, s.out))
        # rows beyond max_frames: one row more than the pool holds
        refused(s, lambda: op(torch.cat([x[40:], x[:1]]), V, 40, 0, W, s.state, s.out))
        # ... and the stream goes on as if nothing had been tried
        s.push(x[40:])
        _same(s.finish().host(), want)
        # calls after END
        refused(s, lambda: op(x[:10], V, T, 0, W, s.state, s.out))
        refused(s, lambda: op(None, V, T, END, W, s.state, s.out))
        _same(_result(eng, s), want)
        # set_hotwords between two calls, and the first set again: the generation has moved on
        s = eng.beam_stream(W, T)
        s.push(x[:40])
        eng.set_hotwords(other, BOOST)
        refused(s, lambda: op(x[40:], V, 40, 0, W, s.state, s.out))
        eng.set_hotwords(phrases, BOOST)
        refused(s, lambda: op(x[40:], V, 40, 0, W, s.state, s.out))
        # set_lm between two calls; the stream object reports the refusal when its result is read
        s = eng.beam_stream(W, T)
        s.push(x[:40])
        eng.set_lm(lm, tok, ALPHA, BETA)
        refused(s, lambda: op(x[40:], V, 40, 0, W, s.state, s.out))
        s.push(x[40:])
        with pytest.raises(GigaAMHipError, match="refused"):
            s.finish().host()
        with pytest.raises(GigaAMHipError, match="has ended"):
            s.push(x[:1])
        # a stream begun under the LM is refused once the LM is gone
        s = eng.beam_stream(W, T)
        s.push(x[:40])
        eng.set_lm(None)
        refused(s, lambda: op(x[40:], V, 40, 0, W, s.state, s.out))
        # BEGIN itself is refused when the pool cannot hold the call's rows
        s = eng.beam_stream(W, 39)
        s.out.whole.fill_(-7)
        refused(s, lambda: op(x[:40], V, 0, BEGIN, W, s.state, s.out))
        _same(_pieces(eng, lp, W, [40]), want)
    finally:
        eng.set_lm(None)
        eng.set_hotwords([])


def _raw(eng, s, lp, n, v, t_base, flags, W, state_bytes=None, **null):
    """The library call as it is -> its return code.  ``null``: the buffers to pass as NULL."""
    from gigaam_amd.engine import _ptr
    o = s.out
    buf = {"log_probs": lp, "state": s.state, "ids": o.ids, "frames": o.frames, "count": o.count, "score": o.score, "logp": o.logp,
           "status": o.status}
    p = {k: _ptr(None if null.get(k) else t) for k, t in buf.items()}
    nbytes = s.state.numel() * 4 if state_bytes is None else state_bytes
    return eng.lib.gam_op_ctc_beam_stream(eng._h, p["log_probs"], n, v, t_base, flags, W, p["state"], nbytes, p["ids"], p["frames"],
                                          p["count"], p["score"], p["logp"], p["status"], eng._stream())


def test_the_library_refuses_bad_arguments_without_a_launch(tmp_path):
    """Check 8: every host error returns non-zero and leaves the state and the result as they were."""
    from gigaam_amd._lib import GigaAMHipError
    eng = _op_engine()
    rng = np.random.default_rng(88)
    V, n, W = 34, 10, 4
    lp = _log_probs(rng, 1, n, V, "flat")[0]
    x = _dev(lp)
    eng.set_hotwords([])
    eng.set_lm(None)
    s = eng.beam_stream(W, n)
    s.out.whole.fill_(-7)
    before = (s.state.clone(), s.out.whole.clone())
    nbytes = s.state.numel() * 4
    bytes_of = lambda w, mf: int(eng.lib.gam_ctc_beam_stream_bytes(eng._h, w, mf))      # noqa: E731
    assert bytes_of(W, n) == nbytes and bytes_of(W, 0) == nbytes - n * W * 16 > 0

    def err():
        return eng.lib.gam_last_error(eng._h).decode()

    for w in (0, 33, -1):
        assert _raw(eng, s, x, n, V, 0, BEGIN, w) != 0 and "beam width" in err(), w
        assert bytes_of(w, n) < 0
    assert bytes_of(W, -1) < 0 and bytes_of(32, 2 ** 26) < 0 and bytes_of(1, 2 ** 31) < 0 and bytes_of(32, 2 ** 26 - 1) > 0
    for v in (1, 1026, 0):
        assert _raw(eng, s, x, n, v, 0, BEGIN, W) != 0 and "bad shape" in err(), v
    assert _raw(eng, s, x, -1, V, 0, BEGIN, W) != 0 and "bad shape" in err()
    assert _raw(eng, s, x, n, V, -1, BEGIN, W) != 0 and "bad shape" in err()
    assert _raw(eng, s, x, n, V, 2 ** 31 - n, BEGIN, W) != 0 and "2^31" in err()
    assert _raw(eng, s, x, n, V, 0, 4, W) != 0 and "flags" in err()
    for nb in (0, bytes_of(W, 0) - 1):
        assert _raw(eng, s, x, n, V, 0, BEGIN, W, state_bytes=nb) != 0 and "state_bytes" in err(), nb
    for name in ("log_probs", "state", "ids", "frames", "count", "score", "logp", "status"):
        assert _raw(eng, s, x, n, V, 0, BEGIN, W, **{name: True}) != 0 and "NULL" in err(), name
    # an LM whose classes are for another V; hotword ids that V does not hold
    tok = _tokenizer(V)
    lm, _ = TL._make_lm(tmp_path, rng, tok, TL._word_ids(rng, lp[None], TL.token_classes(tok), 20), 2, ALPHA, BETA)
    eng.set_lm(lm, tok, ALPHA, BETA)
    try:
        x257 = _dev(_log_probs(rng, 1, n, 257, "flat")[0])
        assert _raw(eng, s, x257, n, 257, 0, BEGIN, W) != 0 and "token classes are for V=34" in err()
    finally:
        eng.set_lm(None)
    eng.set_hotwords([[0, 20]], BOOST)
    try:
        assert _raw(eng, s, x, n, 8, 0, BEGIN, W) != 0 and "hotword token id" in err()
    finally:
        eng.set_hotwords([])
    for w in (0, 33):
        with pytest.raises(GigaAMHipError, match="beam_size"):
            eng.beam_stream(w, n)
    with pytest.raises(GigaAMHipError, match="max_frames"):
        eng.beam_stream(W, -1)
    torch.cuda.synchronize()
    assert torch.equal(s.state, before[0]) and torch.equal(s.out.whole, before[1])
    # (and the limits themselves are legal: a state that holds no frame takes an n = 0 stream; n = 0 needs no rows)
    assert _raw(eng, s, x, 0, V, 0, BEGIN | END, W, state_bytes=bytes_of(W, 0), log_probs=True) == 0
    assert _result(eng, s)["count"] == 0
    assert _raw(eng, s, x, n, V, 0, BEGIN | END, W) == 0
    _same(_result(eng, s), _single(eng, lp, W))
