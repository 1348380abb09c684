"""GPU, op level: gam_op_ctc_confidence_long (gigaam_amd/csrc/gam_confidence.h) -- the token confidences of ONE utterance of any
length -- against the float64 reference of tests/confidence_long_ref.py, and bit for bit against gam_op_ctc_confidence with B = 1 on
streams that op takes.

Crafted peaked log-probs go straight into the op, so the reference reads the same fp32 bits: the argmaxes and the spans are exact
and no case is left out.  Bar: |conf - ref| <= common.TOL_LOGP (a confidence is at most 1); spans and statuses exactly.  The worst
errors go through ``common.report`` before they are asserted."""
import numpy as np
import pytest
import torch

from common import TOL_LOGP, report

import confidence_long_ref as L
import confidence_ref as C

pytestmark = pytest.mark.gpu

MEASURES = ["prob", "entropy"]
AGGS = ["mean", "min", "prod"]
PAIRS = [(m, a) for m in MEASURES for a in AGGS]
POISON = 0x7fffff00     # in the padding of ids / frames: never read

_OP_ENGINE = []


def _op_engine():
    if not _OP_ENGINE:
        from gigaam_amd import synth
        from gigaam_amd.engine import HipEngine, build_config
        cfg = synth.model_cfg("v2_ctc")
        _OP_ENGINE.append(HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], None), {}, torch.device("cuda:0")))
    return _OP_ENGINE[0]


def _stream(rng, T, V, long_run=0):
    """(log-probs f32 [T, V], the class whose value is the peak of each frame): runs of 1-5 frames of one token between 0-4 blank
    frames, two runs sometimes touching, a token at frame 0 and one at frame T - 1, and (``long_run``) one token that owns that many
    frames in a row."""
    blank = V - 1
    cls = np.full(T, blank, dtype=np.int64)
    t, prev, placed_long = 0, -1, long_run == 0
    while t < T - 1:
        k = int(rng.integers(0, blank))
        if k == prev:
            k = (k + 1) % blank
        n = int(rng.integers(1, 6))
        if not placed_long and t > T // 4:
            n, placed_long = long_run, True
        n = min(n, T - 1 - t)
        cls[t:t + n] = k
        t += n + (int(rng.integers(0, 5)) if t else 2)
        prev = k
    cls[T - 1] = (int(cls[T - 2]) + 1) % blank if cls[T - 2] != blank else 0      # a token of its own at the last frame
    x = torch.from_numpy(rng.standard_normal((T, V)).astype(np.float32))
    x[torch.arange(T), torch.from_numpy(cls)] = 9.0
    lp = torch.log_softmax(x, dim=-1).numpy()
    assert (lp.argmax(axis=1) == cls).all()
    return lp, cls


def _token_list(rng, cls, V, early=0.15):
    """The greedy list of ``cls`` with a share of the tokens entered one frame EARLY, on the blank frame in front of their run (the
    entry frame's argmax is then another class; the span goes on through the run)."""
    blank = V - 1
    ids, frames = [], []
    prev = blank
    for t, k in enumerate(cls.tolist()):
        if k != blank and k != prev:
            ids.append(k)
            frames.append(t)
        prev = k
    other = 0
    for u in range(1, len(ids)):
        f = frames[u]
        if cls[f - 1] == blank and frames[u - 1] < f - 1 and rng.random() < early:
            frames[u] = f - 1
            other += 1
    return ids, frames, other


def _dev_tokens(ids, frames, cap):
    i_t = torch.full((cap,), POISON, dtype=torch.int32)
    f_t = torch.full((cap,), POISON, dtype=torch.int32)
    i_t[:len(ids)] = torch.tensor(ids, dtype=torch.int32)
    f_t[:len(ids)] = torch.tensor(frames, dtype=torch.int32)
    return i_t.cuda(), f_t.cuda()


def _check(h, lp, ids, frames, measure, agg, wildcard, what):
    conf, span, ok = L.ctc_confidence_long(lp, ids, frames, measure, agg, wildcard=wildcard)
    n, V = len(ids), lp.shape[1]
    assert h["status"].tolist() == [ok], what
    assert h["span"][0, :n].tolist() == span, what
    assert (h["conf"][0, n:] == -1.0).all() and (h["span"][0, n:] == 0).all(), what
    got = h["conf"][0, :n].astype(np.float64)
    scored = np.asarray([i != V for i in ids], dtype=bool)
    if ok:
        assert ((got[scored] >= 0.0) & (got[scored] <= 1.0)).all() and (got[~scored] == -1.0).all(), what
    return float(np.abs(got - np.asarray(conf)).max()) if n else 0.0


@pytest.mark.parametrize("T,V,pairs", [(8193, 34, PAIRS), (20000, 34, PAIRS), (8193, 65, PAIRS),
                                       (9000, 1025, [("prob", "mean"), ("entropy", "prod")])])
def test_long_confidence_matches_float64_reference(T, V, pairs):
    eng = _op_engine()
    rng = np.random.default_rng(T + V)
    lp, cls = _stream(rng, T, V, long_run=3000)
    ids, frames, other = _token_list(rng, cls, V)
    count = len(ids)
    cap = count + 37 + (1 if (count + 37) % 256 == 0 else 0)
    assert count > 600 and cap % 256 != 0 and frames[0] == 0 and frames[-1] == T - 1 and other >= 20
    spans = L.ctc_confidence_long(lp, ids, frames)[1]
    assert max(spans) in (3000, 3001) and {1, 2, 3, 4, 5, 6} <= set(spans)      # (3001: the long run entered one frame early)
    i_t, f_t = _dev_tokens(ids, frames, cap)
    lp_d = torch.from_numpy(lp).cuda()
    errs = {}
    for measure, agg in pairs:
        h = eng.op_ctc_confidence_long(lp_d, i_t, f_t, count, measure=measure, aggregation=agg).host()
        assert not h["flag"] and h["conf"].shape == (1, cap)
        e = _check(h, lp, ids, frames, measure, agg, False, (T, V, measure, agg))
        print(f"long confidence T={T} V={V} {measure}/{agg}: worst |conf - ref| = {e:.3e}")
        errs[f"{measure}_{agg}"] = e
    report(f"ctc_confidence_long_op_{T}_{V}", **errs)
    for k, e in errs.items():
        assert e <= TOL_LOGP, (T, V, k, e)
    # the decode's own result feeds the pass where it lies: the greedy list, no host round trip
    dec = eng.op_ctc_greedy_long(lp_d)
    h = eng.op_ctc_confidence_long(lp_d, dec, measure=pairs[0][0], aggregation=pairs[0][1]).host()
    g_ids, g_frames = C.ctc_greedy(lp, T)
    assert h["conf"].shape == (1, T)
    assert _check(h, lp, g_ids, g_frames, pairs[0][0], pairs[0][1], False, (T, V, "greedy")) <= TOL_LOGP


@pytest.mark.parametrize("T", [1, 700, 8192])
def test_long_confidence_is_bit_identical_to_the_batch_op(T):
    eng = _op_engine()
    for V, pairs in ((34, PAIRS), (65, [("entropy", "mean")])):
        rng = np.random.default_rng(T * 7 + V)
        lp, cls = _stream(rng, T, V, long_run=40 if T > 100 else 0) if T > 1 else (
            torch.log_softmax(torch.from_numpy(rng.standard_normal((1, V)).astype(np.float32)), dim=-1).numpy(), None)
        ids, frames, _ = _token_list(rng, cls, V, early=0.3) if T > 1 else ([5], [0], 0)
        cap = len(ids) + 3
        i_t, f_t = _dev_tokens(ids, frames, cap)
        lp_d = torch.from_numpy(lp).cuda()
        cnt = torch.tensor([len(ids)], dtype=torch.int32)
        for measure, agg in pairs:
            long = eng.op_ctc_confidence_long(lp_d, i_t, f_t, len(ids), measure=measure, aggregation=agg).host()
            batch = eng.op_ctc_confidence(lp_d[None], torch.tensor([T], dtype=torch.int32), i_t[None], f_t[None], cnt, measure=measure,
                                          aggregation=agg).host()
            assert int(batch["status"][0]) == 1
            for k in ("conf", "span", "status"):
                assert long[k].tobytes() == batch[k].tobytes(), (T, V, measure, agg, k)


def test_long_confidence_validity_is_grid_wide_and_wildcards():
    eng = _op_engine()
    T, V = 3000, 34
    rng = np.random.default_rng(11)
    lp, cls = _stream(rng, T, V)
    ids, frames, _ = _token_list(rng, cls, V)
    n = len(ids)
    assert n >= 600
    cap = n + 5
    lp_d = torch.from_numpy(lp).cuda()

    def run(ids_, frames_, count=None, wildcard=False, cap_=cap):
        i_t, f_t = _dev_tokens(ids_, frames_, cap_)
        return eng.op_ctc_confidence_long(lp_d, i_t, f_t, len(ids_) if count is None else count, wildcard=wildcard).host()

    def refused(h, what):
        assert h["status"].tolist() == [0], what
        assert (h["conf"] == -1.0).all() and (h["span"] == 0).all(), what

    assert run(ids, frames)["status"].tolist() == [1]
    refused(run(ids[:-1] + [V - 1], frames), "blank as the LAST id only")
    refused(run(ids[:-1] + [-3], frames), "a negative id in the last token")
    refused(run(ids, frames[:255] + [frames[255], frames[255]] + frames[257:]), "equal frames across entries 255 / 256")
    refused(run(ids, frames[:-1] + [T]), "a frame equal to T")
    refused(run(ids, frames, count=cap + 1), "count = cap + 1")
    refused(run(ids, frames, count=-1), "a negative count")
    h = run(ids, frames, count=0)
    assert h["status"].tolist() == [1] and (h["conf"] == -1.0).all() and (h["span"] == 0).all()
    # id V: refused without the switch; with it scored around
    stars = sorted(rng.choice(np.arange(1, n - 1), size=40, replace=False).tolist()) + [n - 1]
    w_ids = [V if u in stars or u == 0 else i for u, i in enumerate(ids)]
    refused(run(w_ids, frames), "id V with wildcard = 0")
    for measure, agg in (("prob", "mean"), ("entropy", "min")):
        i_t, f_t = _dev_tokens(w_ids, frames, cap)
        h = eng.op_ctc_confidence_long(lp_d, i_t, f_t, n, measure=measure, aggregation=agg, wildcard=True).host()
        assert h["status"].tolist() == [1]
        assert [u for u in range(n) if h["conf"][0, u] == -1.0] == [0] + stars and [u for u in range(n) if h["span"][0, u] == 0] == [0] + stars
        assert _check(h, lp, w_ids, frames, measure, agg, True, ("wildcards", measure, agg)) <= TOL_LOGP
    refused(eng.op_ctc_confidence_long(lp_d, *_dev_tokens(ids[:-1] + [V + 1], frames, cap), n, wildcard=True).host(), "id V + 1")
    # a wildcard in the middle of a token's run cuts that token's span: the run of token u is entered again by a wildcard
    u = next(k for k in range(1, n - 1) if frames[k + 1] - frames[k] >= 4 and cls[frames[k] + 2] == ids[k])
    c_ids, c_frames = ids[:u + 1] + [V] + ids[u + 1:], frames[:u + 1] + [frames[u] + 2] + frames[u + 1:]
    h = run(c_ids, c_frames, wildcard=True, cap_=cap + 1)
    assert h["status"].tolist() == [1] and int(h["span"][0, u]) == 2 and int(h["span"][0, u + 1]) == 0
    assert _check(h, lp, c_ids, c_frames, "prob", "mean", True, "a wildcard inside a run") <= TOL_LOGP


def test_long_confidence_host_errors_and_the_shared_workspace():
    from gigaam_amd._lib import GigaAMHipError
    eng = _op_engine()
    lib = eng.lib
    d = torch.zeros((4, 34), device="cuda:0")
    o = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    p, lp = o.data_ptr(), d.data_ptr()
    fn = lib.gam_op_ctc_confidence_long
    bufs = [torch.zeros(4, dtype=torch.int32, device="cuda:0") for _ in range(6)]      # ids, frames, count, conf, span, status
    bufs[1].copy_(torch.arange(4, dtype=torch.int32))
    bufs[2].fill_(4)
    assert fn(eng._h, lp, 4, 34, *(b.data_ptr() for b in bufs[:3]), 4, 0, 0, 0, *(b.data_ptr() for b in bufs[3:]), None) == 0
    torch.cuda.synchronize()
    assert bufs[5][0].item() == 1 and bufs[4].tolist() == [1, 1, 1, 1]
    for args, msg in (((lp, 4, 1026, p, p, p, 4, 0, 0, 0, p, p, p), b"V=1026"), ((lp, 4, 1, p, p, p, 4, 0, 0, 0, p, p, p), b"V=1"),
                      ((lp, 0, 34, p, p, p, 4, 0, 0, 0, p, p, p), b"T=0"), ((lp, 1 << 31, 34, p, p, p, 4, 0, 0, 0, p, p, p), b"T=2147483648"),
                      ((lp, 4, 34, p, p, p, -1, 0, 0, 0, p, p, p), b"cap=-1"), ((lp, 4, 34, p, p, p, 4, 2, 0, 0, p, p, p), b"unknown measure 2"),
                      ((lp, 4, 34, p, p, p, 4, 0, 3, 0, p, p, p), b"unknown aggregation 3"),
                      ((lp, 4, 34, p, p, p, 4, 0, 0, 2, p, p, p), b"wildcard=2"), ((None, 4, 34, p, p, p, 4, 0, 0, 0, p, p, p), b"NULL buffer"),
                      ((lp, 4, 34, None, p, p, 4, 0, 0, 0, p, p, p), b"NULL buffer"), ((lp, 4, 34, p, p, None, 4, 0, 0, 0, p, p, p), b"NULL buffer"),
                      ((lp, 4, 34, p, p, p, 4, 0, 0, 0, p, p, None), b"NULL buffer")):
        assert fn(eng._h, *args, None) != 0, msg
        assert msg in lib.gam_last_error(eng._h), (msg, lib.gam_last_error(eng._h))
    bufs[2].fill_(0)
    bufs[5].fill_(7)
    assert fn(eng._h, lp, 4, 34, None, None, bufs[2].data_ptr(), 0, 0, 0, 0, None, None, bufs[5].data_ptr(), None) == 0      # cap = 0: no token buffers
    torch.cuda.synchronize()
    assert bufs[5][0].item() == 1
    with pytest.raises(ValueError, match="unknown confidence measure"):
        eng.op_ctc_confidence_long(d, [1], [0], measure="margin")
    with pytest.raises(ValueError, match="unknown confidence aggregation"):
        eng.op_ctc_confidence_long(d, [1], [0], aggregation="max")
    with pytest.raises(GigaAMHipError, match="without frames"):
        eng.op_ctc_confidence_long(d, [1])
    h = eng.op_ctc_confidence_long(d, [1, 2], [0, 3]).host()             # host lists: uploaded, count = their length
    assert h["status"].tolist() == [1] and h["span"].tolist() == [[1, 1]]
    # the batch op after a long call on the same handle (one workspace): its usual bytes
    rng = np.random.default_rng(2)
    B, Tp, V = 3, 50, 34
    blp = torch.log_softmax(torch.from_numpy(rng.standard_normal((B, Tp, V)).astype(np.float32)), dim=-1).cuda()
    enc_len = torch.tensor([50, 31, 7], dtype=torch.int32)
    ids, frames = [[1, 2, 3], [4, 5], [6]], [[0, 10, 49], [3, 30], [6]]
    before = eng.op_ctc_confidence(blp, enc_len, ids, frames, measure="entropy").host()
    lp_long, cls = _stream(rng, 9000, V)
    l_ids, l_frames, _ = _token_list(rng, cls, V)
    assert eng.op_ctc_confidence_long(torch.from_numpy(lp_long).cuda(), l_ids, l_frames, measure="prob").host()["status"].tolist() == [1]
    after = eng.op_ctc_confidence(blp, enc_len, ids, frames, measure="entropy").host()
    for k in ("conf", "span", "status"):
        assert before[k].tobytes() == after[k].tobytes(), k
