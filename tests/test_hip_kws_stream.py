"""GPU: the resumable keyword search (gam_op_ctc_kws_stream, gam_ctc_kws_stream_kernel in gigaam_amd/csrc/gam_kws.h): one call against
the batch kernel bit for bit, split invariance, a stream past the batch kernel's 8192 frames against the float64 reference, the
flush of more than 64 hits per call, the carry across calls, two interleaved streams, every refusal, and the side-stream launch."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from common import report

import kws_inputs as I
import kws_ref as R
import test_hip_kws as TK

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BEGIN, END = 1, 2
NEG = -np.inf


def _begin(eng, kws, thr=0.5, max_hits=8):
    eng.set_keywords(kws, TK._min_scores(kws, thr))
    return eng.kws_stream(max_hits)


def _dev(lp):
    return torch.from_numpy(np.ascontiguousarray(lp, dtype=np.float32)).to(DEV)


def _result(eng, s, check=True):
    """The stream's arrays as they are on the device now (not through ``finish``: no call is made)."""
    return eng._finish(s.out, False).host(check)


def _single(eng, lp, kws, thr=0.5, max_hits=8):
    """ONE call with BEGIN | END over the whole stream -> the host arrays and the dense rows [K, T]."""
    s = _begin(eng, kws, thr, max_hits)
    ds, dst = eng.op_ctc_kws_stream(_dev(lp), lp.shape[1], 0, BEGIN | END, s.state, s.out, dense=True)
    h = _result(eng, s)
    h["dense_score"], h["dense_start"] = ds.cpu().numpy(), dst.cpu().numpy()
    return h


def _pieces(eng, lp, kws, cuts, thr=0.5, max_hits=8, overlap=False, dense=True):
    """The stream fed in the pieces that ``cuts`` make (a repeated cut: a call with n = 0), END as a call of its own."""
    s = _begin(eng, kws, thr, max_hits)
    x, edges, rows = _dev(lp), [0] + [int(c) for c in cuts] + [lp.shape[0]], []
    for a, b in zip(edges[:-1], edges[1:]):
        rows.append(s.push(x[a:b], dense=dense, overlap=overlap))
    h = s.finish().host()
    torch.cuda.synchronize()
    if dense:
        h["dense_score"] = torch.cat([r[0] for r in rows], dim=1).cpu().numpy()
        h["dense_start"] = torch.cat([r[1] for r in rows], dim=1).cpu().numpy()
    assert s.t_next == lp.shape[0] and s.ended
    return h


KEYS = ("n_hits", "hit_frames", "hit_score", "dense_score", "dense_start")


def _same(a, b, keys=KEYS):
    for key in keys:
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), key


def _stream_case(name, kind):
    """Utterance 0 (full length) of test_hip_kws.CASES[name] -> (lp [T, V], keywords)."""
    if kind == "dyadic":
        V, Tp, _, plan, _, _ = TK.CASES[name]
        rng = np.random.default_rng(sum(map(ord, name)) + 13)
        return I.log_probs(rng, 1, Tp, V, "dyadic")[0], [I.keyword(rng, U, V, r) for U, r in plan]
    V, Tp, enc_len, kws, lp, _ = TK._case(name, kind)
    assert enc_len[0] == Tp
    return lp[0], kws


CASE_IDS = [(n, k) for n in ("lanes", "full", "tiny") for k in ("peaked", "flat", "dyadic")]


@pytest.mark.parametrize("name,kind", CASE_IDS)
def test_one_call_equals_the_batch_kernel_bit_for_bit(name, kind):
    """Check 1: U in {1, 2, 3, 31, 32, 33} at V = 34, T = 160; U in {64, 63, 17, 5} at V = 257, T = 400; V = 4, T = 5."""
    eng = TK._op_engine()
    lp, kws = _stream_case(name, kind)
    want = TK._run(eng, lp[None], [lp.shape[0]], kws, 0.5, max_hits=8)
    got = _single(eng, lp, kws, 0.5, 8)
    assert (got["status"] == 1).all()
    _same(got, {k: want[k][0] for k in KEYS})
    # the search without the dense rows returns the same hits
    s = _begin(eng, kws, 0.5, 8)
    assert eng.op_ctc_kws_stream(_dev(lp), lp.shape[1], 0, BEGIN | END, s.state, s.out) is None
    _same(_result(eng, s), got, KEYS[:3])


def _cuttings(T, seed):
    fixed = [c for c in (0, 1, 2, 5, 64, 65, 127, 128, 131) if c <= T]       # pieces of 0, 1, 1, 3, 59, 1, 62, 1, 3 frames and the rest
    mid = fixed[len(fixed) // 2]
    rng = np.random.default_rng(seed)
    return [sorted(fixed + [mid])] + [sorted(rng.integers(0, T + 1, int(rng.integers(1, 10))).tolist()) for _ in range(3)]


@pytest.mark.parametrize("name,kind", CASE_IDS)
def test_any_cutting_gives_the_bits_of_the_single_call(name, kind):
    """Check 2: the fixed cuts with an n = 0 call in the middle and END as an n = 0 call of its own, and three seeded random cuttings."""
    eng = TK._op_engine()
    lp, kws = _stream_case(name, kind)
    want = _single(eng, lp, kws, 0.5, 8)
    for cuts in _cuttings(lp.shape[0], len(name) + len(kind)):
        _same(_pieces(eng, lp, kws, cuts), want)


LONG_T, LONG_V, LONG_CUT = 8262, 8, 8190


@pytest.fixture(scope="module")
def long_case():
    """T = 8262 > the batch kernel's 8192, V = 8, U = 1, 2, 5, peaked with planted occurrences; the five-token keyword's LAST occurrence
    lies across the call boundary 8189 | 8190 AND across frames 8191 | 8192.  The float64 reference is computed once."""
    rng = np.random.default_rng(8262)
    kws = [I.keyword(rng, U, LONG_V) for U in (1, 2, 5)]
    top = I.background(rng, LONG_T, LONG_V)
    planted, pos = [], 3
    for base in (3, 4000, 8100):
        pos = base
        for k in (0, 1, 2):
            s, e, pos = I.plant(rng, top, LONG_V, kws[k], pos, LONG_T)
            planted.append((k, s, e))
    s, e, _ = I.plant(rng, top, LONG_V, kws[2], 8185, LONG_T)
    assert s <= LONG_CUT - 1 and e >= 8192
    planted.append((2, s, e))
    lp = I.log_probs(rng, 1, LONG_T, LONG_V, "peaked", top[None])[0]
    return lp, kws, planted, [R.dense(lp, y) for y in kws]


def test_a_stream_past_8192_frames_matches_the_float64_reference(long_case):
    """Check 3, as one call and as calls of 8190 and 72 frames (1024 slots: the one-token keyword occurs some hundred times)."""
    MH = 1024
    eng = TK._op_engine()
    lp, kws, planted, ref = long_case
    ms = TK._min_scores(kws, 0.5)
    one = _single(eng, lp, kws, 0.5, MH)
    two = _pieces(eng, lp, kws, [LONG_CUT], 0.5, MH)
    _same(two, one)
    errs = {}
    for k, y in enumerate(kws):
        E, S = one["dense_score"][k].astype(np.float64), one["dense_start"][k]
        Er, _ = ref[k]
        fin = np.isfinite(Er)
        assert np.array_equal(np.isfinite(E), fin), (k, "-inf pattern")
        assert (E[~fin] == NEG).all() and (S[~fin] == -1).all() and (E[fin] <= 0).all()
        d = np.abs(E[fin] - Er[fin]) / np.maximum(1.0, np.abs(Er[fin]))
        errs["dense"] = max(errs.get("dense", 0.0), float(d.max()))
        print(f"keyword {k}: max dense error {d.max():.3e}")
        assert (d <= 1e-3).all(), (k, float(d.max()))
        sp = R.span_scores(lp, y, S[fin], np.nonzero(fin)[0])
        d = np.abs(sp - Er[fin]) / np.maximum(1.0, np.abs(Er[fin]))
        errs["start"] = max(errs.get("start", 0.0), float(d.max()))
        print(f"keyword {k}: max start error {d.max():.3e}")
        assert (d <= 1e-3).all(), (k, "a returned start is not optimal", float(d.max()))
        # the hits are the streaming rule on the kernel's own rows
        hits, n = R.pick(one["dense_score"][k], one["dense_start"][k], ms[k], MH)
        assert int(one["n_hits"][k]) == n
        got_f, got_s = one["hit_frames"][k], one["hit_score"][k]
        for r, (s, e, sc) in enumerate(hits):
            assert (int(got_f[r, 0]), int(got_f[r, 1])) == (s, e) and got_s[r].tobytes() == np.float32(sc).tobytes(), (k, r)
        assert (got_f[len(hits):] == -1).all() and (got_s[len(hits):] == NEG).all()
    for k, s, e in planted:
        n = int(one["n_hits"][k])
        assert n <= MH
        found = [(int(f[0]), int(f[1]), float(sc)) for f, sc in zip(one["hit_frames"][k, :n], one["hit_score"][k, :n])]
        assert (s, e, 0.0) in found, (k, (s, e), found[-4:])
    report("ctc_kws_stream_long", **errs)


def test_more_than_64_hits_in_one_call_are_flushed_in_order():
    """Check 4: a one-token keyword alternating with blank over 400 peaked frames closes 200 hits, 32 per 64-frame chunk."""
    eng = TK._op_engine()
    V, T, y = 4, 400, [1]
    top = np.where(np.arange(T) % 2 == 0, 1, V - 1)
    lp = I.log_probs(np.random.default_rng(4), 1, T, V, "peaked", top[None])[0]
    hits, n = R.pick(*R.dense(lp, y), math.log(0.5), 4096)
    assert n == 200 and hits == [(t, t, 0.0) for t in range(0, T, 2)]
    for cuts in ([], list(range(64, T, 64)), list(range(37, T, 37))):
        for mh in (256, 100):
            h = _pieces(eng, lp, [y], cuts, 0.5, mh, dense=False)
            keep = min(mh, 200)
            assert int(h["n_hits"][0]) == 200, (cuts[:2], mh)
            assert h["hit_frames"][0, :keep].tolist() == [[s, e] for s, e, _ in hits[:keep]]
            assert (h["hit_score"][0, :keep] == 0.0).all()
            assert (h["hit_frames"][0, keep:] == -1).all() and (h["hit_score"][0, keep:] == NEG).all()


def _peaked(top, V, seed=0):
    return I.log_probs(np.random.default_rng(seed), 1, len(top), V, "peaked", np.asarray(top)[None])[0]


def test_what_is_carried_across_calls():
    """Check 5 (peaked inputs: a planted occurrence scores exactly 0)."""
    eng = TK._op_engine()
    V = 5
    b = V - 1
    # the last token's run spans a call boundary: the hit ends on the run's last frame, in the later call
    lp = _peaked([b, 0, 1, 1, 1, b], V)
    for cuts in ([3], [4], [3, 4]):
        h = _pieces(eng, lp, [[0, 1]], cuts)
        assert int(h["n_hits"][0]) == 1 and h["hit_frames"][0, 0].tolist() == [1, 4] and float(h["hit_score"][0, 0]) == 0.0
    # the prefix in call 1, all-blank rows in call 2, the suffix in call 3: found once, from call 1's frame
    lp = _peaked([b, 0, 1, b, b, b, b, 2, b], V)
    h = _pieces(eng, lp, [[0, 1, 2]], [3, 7])
    assert int(h["n_hits"][0]) == 1 and h["hit_frames"][0, 0].tolist() == [1, 7] and float(h["hit_score"][0, 0]) == 0.0
    assert (h["hit_frames"][0, 1:] == -1).all() and (h["hit_score"][0, 1:] == NEG).all()
    _same(h, _single(eng, lp, [[0, 1, 2]]))
    # END on a stream without an open candidate adds nothing
    lp = _peaked([b] * 70, V)
    h = _pieces(eng, lp, [[0, 1, 2], [3]], [64])
    assert (h["n_hits"] == 0).all() and (h["hit_frames"] == -1).all() and (h["hit_score"] == NEG).all()
    # a stream that begins at a later frame counts from there
    lp = _peaked([b, 0, 1, 1, b], V)
    s = _begin(eng, [[0, 1]])
    s.t_next = 2_000_000_000
    s.push(_dev(lp[:2]))
    s.push(_dev(lp[2:]))
    h = s.finish().host()
    assert int(h["n_hits"][0]) == 1 and h["hit_frames"][0, 0].tolist() == [2_000_000_001, 2_000_000_003]


def test_two_streams_pushed_alternately_through_two_states():
    """Check 6."""
    eng = TK._op_engine()
    rng = np.random.default_rng(66)
    V, T = 34, 150
    kws = [I.keyword(rng, U, V, r) for U, r in ((1, 0), (3, 1), (7, 0))]
    lps = []
    for _ in range(2):
        top, pos = I.background(rng, T, V), 2
        for y in kws:
            _, _, pos = I.plant(rng, top, V, y, pos + int(rng.integers(0, 25)), T)
        lps.append(I.log_probs(rng, 1, T, V, "peaked", top[None])[0])
    want = [_single(eng, lp, kws) for lp in lps]
    assert not np.array_equal(want[0]["hit_frames"], want[1]["hit_frames"])
    eng.set_keywords(kws, TK._min_scores(kws, 0.5))
    ss = [eng.kws_stream(8), eng.kws_stream(8)]
    xs, rows = [_dev(lp) for lp in lps], ([], [])
    edges = ([0, 10, 64, 65, 150], [0, 70, 71, 128, 150])
    for i in range(4):
        for j in (0, 1):
            rows[j].append(ss[j].push(xs[j][edges[j][i]:edges[j][i + 1]], dense=True))
    for j in (0, 1):
        h = ss[j].finish().host()
        h["dense_score"] = torch.cat([r[0] for r in rows[j]], dim=1).cpu().numpy()
        h["dense_start"] = torch.cat([r[1] for r in rows[j]], dim=1).cpu().numpy()
        _same(h, want[j])


def _raw(eng, s, lp, n, v, t_base, flags, **null):
    """The library call as it is -> its return code.  ``null``: the buffers to pass as NULL."""
    from gigaam_amd.engine import _ptr
    o = s.out
    buf = {"log_probs": lp, "state": s.state, "hit_frames": o.hit_frames, "hit_score": o.hit_score, "n_hits": o.n_hits, "status": o.status}
    p = {k: _ptr(None if null.get(k) else t) for k, t in buf.items()}
    return eng.lib.gam_op_ctc_kws_stream(eng._h, p["log_probs"], n, v, t_base, flags, p["state"], s.max_hits, p["hit_frames"], p["hit_score"],
                                         p["n_hits"], p["status"], C.c_void_p(0), C.c_void_p(0), eng._stream())


def test_the_library_refuses_bad_arguments_without_a_launch():
    """Check 7, first half: every error leaves the buffers as they were."""
    from gigaam_amd._lib import GigaAMHipError
    eng = TK._op_engine()
    V, n = 6, 10
    lp = _dev(I.log_probs(np.random.default_rng(1), 1, n, V, "flat")[0])
    s = _begin(eng, [[0, 1], [2]])
    s.out.whole.fill_(-7)
    before = (s.state.clone(), s.out.whole.clone())

    def err():
        return eng.lib.gam_last_error(eng._h).decode()

    assert _raw(eng, s, lp, -1, V, 0, BEGIN) != 0 and "bad shape" in err()
    assert _raw(eng, s, lp, n, V, -1, BEGIN) != 0 and "bad shape" in err()
    assert _raw(eng, s, lp, n, V, 2 ** 31 - n, BEGIN) != 0 and "2^31" in err()
    assert _raw(eng, s, lp, n, V, 2 ** 31 - n - 1, 4) != 0 and "flags" in err()
    for name in ("log_probs", "state", "hit_frames", "hit_score", "n_hits", "status"):
        assert _raw(eng, s, lp, n, V, 0, BEGIN, **{name: True}) != 0 and "NULL" in err(), name
    assert _raw(eng, s, lp, n, 3, 0, BEGIN) != 0 and "token id" in err()        # id 2 >= V - 1 = 2
    for mh in (0, 4097):
        bad = eng.kws_stream(mh)
        with pytest.raises(GigaAMHipError, match="max_hits"):
            bad.push(lp)
    eng.set_keywords([], 0.0)
    assert _raw(eng, s, lp, n, V, 0, BEGIN) != 0 and "no keyword set" in err()
    assert eng.lib.gam_ctc_kws_state_bytes(eng._h) < 0
    with pytest.raises(GigaAMHipError, match="no keyword set"):
        eng.kws_stream(8)
    torch.cuda.synchronize()
    assert torch.equal(s.state, before[0]) and torch.equal(s.out.whole, before[1])
    # (and the limits themselves are legal)
    t = _begin(eng, [[0, 1], [2]], max_hits=4096)
    assert eng.lib.gam_ctc_kws_state_bytes(eng._h) == t.state.numel() * 4 > 0
    assert _raw(eng, t, lp, n, V, 2 ** 31 - n - 1, BEGIN | END) == 0
    assert (_result(eng, t)["status"] == 1).all()


def test_the_kernel_refuses_calls_that_do_not_continue_the_stream():
    """Check 7, second half: status 0, every output and the state unchanged."""
    eng = TK._op_engine()
    rng = np.random.default_rng(77)
    V, T = 8, 90
    kws, other = [[0, 1], [2], [3, 4, 5]], [[0, 1], [2], [3, 4, 6]]
    top, pos = I.background(rng, T, V), 2
    for y in kws + kws:
        _, _, pos = I.plant(rng, top, V, y, pos, T)
    lp = I.log_probs(rng, 1, T, V, "peaked", top[None])[0]
    x = _dev(lp)
    want = _single(eng, lp, kws)
    assert (want["n_hits"] >= 2).all()

    def refused(s, call):
        torch.cuda.synchronize()
        state, whole = s.state.clone(), s.out.whole.clone()
        s.out.status.fill_(5)
        call()
        h = _result(eng, s, check=False)
        assert (h["status"] == 0).all()
        s.out.status.copy_(whole[s.out.k:2 * s.out.k])
        torch.cuda.synchronize()
        assert torch.equal(s.state, state) and torch.equal(s.out.whole[:-1], whole[:-1])

    # the first call without BEGIN, on a zeroed state
    s = _begin(eng, kws)
    s.out.whole.fill_(-7)
    refused(s, lambda: eng.op_ctc_kws_stream(x[:40], V, 0, 0, s.state, s.out))
    refused(s, lambda: eng.op_ctc_kws_stream(None, V, 0, END, s.state, s.out))
    # a frame skipped or repeated; the stream then goes on as if nothing had been tried
    s.push(x[:40])
    refused(s, lambda: eng.op_ctc_kws_stream(x[40:], V, 41, 0, s.state, s.out))
    refused(s, lambda: eng.op_ctc_kws_stream(x[40:], V, 39, END, s.state, s.out))
    refused(s, lambda: eng.op_ctc_kws_stream(None, V, 0, 0, s.state, s.out))
    # another keyword set between two calls (the same sizes: only the generation tells), then the first one again
    eng.set_keywords(other, TK._min_scores(other, 0.5))
    refused(s, lambda: eng.op_ctc_kws_stream(x[40:], V, 40, 0, s.state, s.out))
    eng.set_keywords(kws, TK._min_scores(kws, 0.5))
    refused(s, lambda: eng.op_ctc_kws_stream(x[40:], V, 40, 0, s.state, s.out))
    # ... so that stream is lost; a new one over the same rows, and calls after its END
    s = _begin(eng, kws)
    s.push(x[:40])
    s.push(x[40:])
    h = s.finish().host()
    _same(h, want, KEYS[:3])
    refused(s, lambda: eng.op_ctc_kws_stream(x[:10], V, T, 0, s.state, s.out))
    refused(s, lambda: eng.op_ctc_kws_stream(None, V, T, END, s.state, s.out))
    _same(_result(eng, s, check=False), want, KEYS[:3])
    # the stream object reports a refusal when its result is read
    from gigaam_amd._lib import GigaAMHipError
    s = _begin(eng, kws)
    s.push(x[:40])
    eng.set_keywords(other, TK._min_scores(other, 0.5))
    s.push(x[40:])
    with pytest.raises(GigaAMHipError, match="refused"):
        s.finish().host()
    with pytest.raises(GigaAMHipError, match="has ended"):
        s.push(x[:1])


def test_a_keyword_set_of_another_size_is_refused_before_any_launch():
    """The library launches a wave per keyword of the set at hand and cannot see the buffers' sizes: a stream made for K keywords must
    not reach it once the set has another K -- larger or smaller, between two pushes or before the first (where BEGIN would fill and
    store for every keyword of the new set)."""
    from gigaam_amd._lib import GigaAMHipError
    eng = TK._op_engine()
    V, T = 8, 90
    lp = I.log_probs(np.random.default_rng(9), 1, T, V, "peaked")[0]
    x = _dev(lp)
    kws = [[0, 1], [2], [3, 4, 5]]
    larger = kws + [[int(c)] for c in np.random.default_rng(1).integers(0, V - 1, 997)]
    smaller = kws[:2]
    want = _single(eng, lp, kws)
    for other in (larger, smaller):
        # between two pushes
        s = _begin(eng, kws)
        s.push(x[:40])
        guard = torch.full((4096,), -7, dtype=torch.int32, device=DEV)       # (a neighbour in memory: allocated right behind the stream's buffers)
        torch.cuda.synchronize()
        state, whole = s.state.clone(), s.out.whole.clone()
        eng.set_keywords(other, TK._min_scores(other, 0.5))
        for call in (lambda: s.push(x[40:]), lambda: s.push(x[40:], overlap=True), lambda: s.finish(),
                     lambda: eng.op_ctc_kws_stream(x[40:], V, 40, 0, s.state, s.out)):
            with pytest.raises(GigaAMHipError, match="another set"):
                call()
        assert (s.t_next, s.begun, s.ended) == (40, True, False)
        # before the first push: no BEGIN reaches the library
        eng.set_keywords(kws, TK._min_scores(kws, 0.5))
        f = eng.kws_stream(8)
        f.out.whole.fill_(-7)
        eng.set_keywords(other, TK._min_scores(other, 0.5))
        for call in (lambda: f.push(x[:40]), lambda: f.finish(), lambda: eng.op_ctc_kws_stream(x[:40], V, 0, BEGIN, f.state, f.out)):
            with pytest.raises(GigaAMHipError, match="another set"):
                call()
        torch.cuda.synchronize()
        assert not f.begun and (f.state == 0).all() and (f.out.whole == -7).all()
        assert torch.equal(s.state, state) and torch.equal(s.out.whole, whole) and (guard == -7).all()
        # with its own set at hand again the generation has moved on: the kernel's refusal, and still nothing is written
        eng.set_keywords(kws, TK._min_scores(kws, 0.5))
        s.push(x[40:])
        assert (_result(eng, s, check=False)["status"] == 0).all()
        torch.cuda.synchronize()
        assert torch.equal(s.state, state) and torch.equal(s.out.whole[2 * s.k:-1], whole[2 * s.k:-1]) and (guard == -7).all()
    _same(_pieces(eng, lp, kws, [40], dense=False), want, KEYS[:3])


def test_side_stream_pushes_equal_launch_stream_pushes(long_case):
    """Check 8: the long stream in five pieces, ``overlap=True`` against ``overlap=False``."""
    eng = TK._op_engine()
    lp, kws, _, _ = long_case
    cuts = [1000, 4097, 8190, 8191]
    a = _pieces(eng, lp, kws, cuts, 0.5, 64, overlap=False)
    b = _pieces(eng, lp, kws, cuts, 0.5, 64, overlap=True)
    _same(b, a)
    assert (a["n_hits"] > 0).all()
