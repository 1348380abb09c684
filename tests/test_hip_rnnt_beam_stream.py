"""GPU: the resumable RNN-T beam search (gam_op_rnnt_beam_stream, gigaam_amd/csrc/gam_rnnt_beam_stream.h) at the op level.

Exactness.  Against the batch kernel (gam_op_rnnt_beam) and between cuttings of one stream every comparison is bit for bit whatever
the margin: both run ONE search text (gam_rb_body) on the same rows, and below a rebase period nothing differs.  Against float64
(the stored references of tests/rnnt_head_cases.py; tests/rnnt_beam_stream_ref.py for the long streams) ids and frames are compared
exactly and scores within ``BC.bar`` for the utterances whose smallest decision margin exceeds the bar the CPU tests hold
(tests/test_rnnt_head_cases_host.py: at least 90 % of every set; tests/test_rnnt_beam_stream_host.py: the long inputs, none skipped)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import beam_common as BC
import nbest_inputs as I
import rnnt_beam_stream_ref as SB
import rnnt_head_cases as HC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BEGIN, END = SB.BEGIN, SB.END
HDR_WORDS = (128 + 32 * 80) // 4          # the header and the 32 beam entries

_ENGINES = {}


def _engine(name, L, kind):
    key = (name, L, kind)
    if key not in _ENGINES:
        from gigaam_amd.engine import HipEngine, build_config
        cfg, sd, _ = HC.head(name, L, kind)
        _ENGINES[key] = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), sd, torch.device(DEV))
    return _ENGINES[key]


def _lm(tmp_path, text, i=0):
    from gigaam_amd import lm as LM
    p = tmp_path / f"lm{i}.arpa"
    p.write_text(text, encoding="utf-8")
    return LM.NgramLM.from_arpa(str(p))


def _clear(eng):
    eng.set_lm(None)
    eng.set_hotwords([])


def _fixed_bytes(eng, W, S):
    c = eng.cfg
    return 128 + 32 * 80 + (S + 1) * W * (2 * int(c.pred_rnn_layers) * int(c.pred_hidden) + int(c.joint_hidden)) * 4


class Raw:
    """A state record and a result, driven call by call through ``op_rnnt_beam_stream``."""

    def __init__(self, eng, W, S, max_frames, state_words=None):
        from gigaam_amd.engine import BeamStreamDecoded
        self.eng, self.W, self.S, self.max_frames = eng, W, S, max_frames
        self.nbytes = int(eng.lib.gam_rnnt_beam_stream_bytes(eng._h, W, S, max_frames))
        assert self.nbytes == _fixed_bytes(eng, W, S) + max_frames * S * W * 16
        self.exact = self.nbytes      # the record's size; ``nbytes``: what a call passes as state_bytes (a larger buffer: all of it)
        self.state = torch.zeros((state_words or self.nbytes // 4,), dtype=torch.int32, device=DEV)
        self.nbytes = self.state.numel() * 4
        self.out = BeamStreamDecoded.empty(torch.device(DEV), max_frames * S)
        self.out.whole.fill_(-7)

    def call(self, rows, t_base, flags, W=None, S=None, eng=None, state_bytes=None, cap=None):
        rows = None if rows is None or len(rows) == 0 else torch.as_tensor(rows, dtype=torch.float32, device=DEV).contiguous()
        with torch.cuda.device(torch.device(DEV)):
            (eng or self.eng).op_rnnt_beam_stream(rows, t_base, flags, self.W if W is None else W, self.S if S is None else S, self.state,
                                                  self.nbytes if state_bytes is None else state_bytes, self.out, cap)
        return int(self.out.status.cpu()[0])

    def result(self):
        """(ids, frames, score bits, logp bits) of the END call."""
        torch.cuda.synchronize()
        n = int(self.out.count.cpu()[0])
        sc = self.out.score.cpu().numpy().view(np.int64)[0]
        lp = self.out.logp.cpu().numpy().view(np.int64)[0]
        return self.out.ids[:n].cpu().tolist(), self.out.frames[:n].cpu().tolist(), int(sc), int(lp)

    def floats(self):
        return float(self.out.score.cpu().numpy().view(np.float64)[0]), float(self.out.logp.cpu().numpy().view(np.float64)[0])

    def header(self):
        torch.cuda.synchronize()
        return self.state[:HDR_WORDS].cpu().numpy().copy()

    def snapshot(self):
        torch.cuda.synchronize()
        return self.state.clone(), self.out.whole.clone()


def _stream(eng, rows, cuts, W, S, t0=0, end_alone=False, headers=None):
    """The stream cut at ``cuts`` -> (ids, frames, score bits, logp bits); ``headers``: {frame: header and entries} is filled / compared
    after every call that does not end the stream."""
    edges = [0] + list(cuts) + [len(rows)]
    r = Raw(eng, W, S, len(rows))
    for j, (a, b) in enumerate(zip(edges, edges[1:])):
        last = j == len(edges) - 2
        ends = last and not end_alone
        assert r.call(rows[a:b], t0 + a, (BEGIN if j == 0 else 0) | (END if ends else 0)) == 1, (cuts, j)
        if headers is not None and not ends:
            h = r.header()
            if b in headers:
                assert np.array_equal(h, headers[b]), (cuts, b)
            headers[b] = h
    if end_alone:
        assert r.call(None, t0 + len(rows), END) == 1
    return r.result(), r


def _f32_bits(x):
    return int(np.float32(x).view(np.int32))


# ---- (a) one call against the batch kernel and float64
SETS = [("C", 1, "blank"), ("C", 1, "dense"), ("D", 1, "blank"), ("D", 1, "dense"), ("F", 1, "blank"), ("F", 1, "dense"), ("A", 2, "blank"),
        ("A", 2, "dense")]


def _one_call_cases(eng, name, cases, lm_of=None):
    ok = n = 0
    errs = {}
    widths = set()
    for i, c in enumerate(cases):
        W, S = c["W"], c["S"]
        eng.set_hotwords(c["phrases"], HC.BETA)
        if lm_of is not None:
            eng.set_lm(lm_of(i, c), BC.tokenizer(HC.sizes(name)[0]), I.LM_ALPHA, I.LM_BETA)
        h = BC.run_rnnt_op(eng, c["encp"], HC.ENC_LEN, W, S)
        widths.add(W > 16)
        for b, T in enumerate(HC.ENC_LEN):
            (ids, frames, sc, lp), r = _stream(eng, c["encp"][b, :T], [], W, S)
            score, logp = r.floats()
            assert (ids, frames) == tuple(h["rows"][b]), (name, W, S, b)
            assert _f32_bits(score) == _f32_bits(h["score"][b]) and _f32_bits(logp) == _f32_bits(h["logp"][b]), (name, W, S, b)
            ref = c["refs"][b]
            n += 1
            if ref["margin"] > HC.MARGIN:
                ok += 1
                assert ids == ref["ids"] and frames == ref["frames"], (name, W, S, b)
                for k, got in (("score", score), ("logp", logp)):
                    e = abs(got - ref[k])
                    errs[k] = max(errs.get(k, 0.0), e / max(1.0, abs(ref[k])))
                    assert e <= BC.bar(ref[k]), (name, W, S, b, k, got, ref[k])
    assert widths == {False, True}      # both row-tile counts ran
    print(f"head {name}: {ok} of {n} utterances above the margin; largest relative errors {errs}")
    assert ok >= 0.9 * n - 1e-9


@pytest.mark.parametrize("name,L,kind", SETS)
def test_one_call_is_the_batch_kernel_and_float64(name, L, kind):
    eng = _engine(name, L, kind)
    try:
        eng.set_lm(None)
        _one_call_cases(eng, name, HC.beam_cases(name, L, kind))
    finally:
        _clear(eng)


@pytest.mark.parametrize("name,L", [("C", 1), ("A", 2)])
def test_one_call_with_the_lm_is_the_batch_kernel_and_float64(name, L, tmp_path):
    eng = _engine(name, L, "dense")
    try:
        _one_call_cases(eng, name, HC.lm_cases(name, L), lambda i, c: _lm(tmp_path, c["arpa"], i))
    finally:
        _clear(eng)


# ---- (b) cuttings, (c) a stream without a frame
@pytest.mark.parametrize("with_lm", [False, True])
def test_every_cutting_gives_the_single_call_bits_and_the_same_record(with_lm, tmp_path):
    """Head D, dense, W = 16, S = 3 with hotwords (the LM case: head C, the LM set's combination 3, W = 16, S = 3, order 5): every cut
    position of the 10-frame stream, one frame per call, empty calls, END alone.  The header and the 32 beam entries after a call
    that stops at frame f are the same bytes whatever cutting led there."""
    name = "C" if with_lm else "D"
    eng = _engine(name, 1, "dense")
    c = (HC.lm_cases if with_lm else lambda n, L: HC.beam_cases(n, L, "dense"))(name, 1)[3]
    W, S, T = c["W"], c["S"], HC.T
    assert (W, S) == (16, 3) and c["phrases"]
    try:
        eng.set_hotwords(c["phrases"], HC.BETA)
        eng.set_lm(_lm(tmp_path, c["arpa"]) if with_lm else None, BC.tokenizer(HC.sizes(name)[0]), I.LM_ALPHA, I.LM_BETA)
        rows = c["encp"][0]
        want, _ = _stream(eng, rows, [], W, S)
        assert len(want[0]) > 0
        headers = {}
        for f in range(T + 1):      # the record after one BEGIN call of f rows
            r = Raw(eng, W, S, T)
            assert r.call(rows[:f], 0, BEGIN) == 1
            headers[f] = r.header()
        assert not np.array_equal(headers[3], headers[4])
        cuttings = [[p] for p in range(1, T)] + [list(range(1, T)), [0], [T], [0, 0, 4, 4, 4, T, T], [3, 3]]
        for cuts in cuttings:
            for end_alone in (False, True):
                got, _ = _stream(eng, rows, cuts, W, S, end_alone=end_alone, headers=headers)
                assert got == want, (cuts, end_alone)
        # (c) a stream without a frame
        r = Raw(eng, W, S, 0)
        assert r.call(None, 5, BEGIN | END) == 1
        assert r.result()[:2] == ([], []) and r.floats() == (0.0, 0.0)
        r = Raw(eng, W, S, 4)
        assert r.call(None, 0, BEGIN) == 1 and r.call(None, 0, 0) == 1 and r.call(None, 0, END) == 1
        assert r.result()[:2] == ([], []) and r.floats() == (0.0, 0.0)
    finally:
        _clear(eng)


# ---- (d) across the rebase
@functools.lru_cache(maxsize=None)
def _long(kind, lm_seed):
    seed = SB.LONG_SEEDS[kind]
    hd, encp, phrases = SB.long_input(seed, kind)
    text, spec = SB.long_lm(seed, hd, encp, lm_seed) if lm_seed is not None else (None, None)
    ok, margin, bar, peak, res = SB.long_qualifies(hd, encp, phrases, spec)
    return encp, phrases, text, ok, margin, bar, res


@pytest.mark.parametrize("kind,lm_seed", [("blank", None), ("blank", SB.LONG_LM_SEED), ("dense", None)])
def test_a_stream_across_two_rebase_frames(kind, lm_seed, tmp_path):
    """Head D, T = 2 periods + 40, W = 4, S = 3, six hotwords, boost 1.5 (and an LM of order 3): against float64 under the bar
    tests/test_rnnt_beam_stream_host.py qualifies these inputs by, and bit for bit between one call, cuts around the first rebase
    frame and 17 uneven pieces."""
    from gigaam_amd.engine import HipEngine
    encp, phrases, text, ok, margin, bar, ref = _long(kind, lm_seed)
    assert ok and margin > bar, (margin, bar)
    P = HipEngine.RNNT_BEAM_STREAM_REBASE
    assert P == SB.REBASE and len(encp) == 2 * P + 40
    eng = _engine("D", 1, kind)
    W, S = SB.LONG_W, SB.LONG_S
    try:
        eng.set_hotwords(phrases, HC.BETA)
        eng.set_lm(None if text is None else _lm(tmp_path, text), BC.tokenizer(HC.sizes("D")[0]), I.LM_ALPHA, I.LM_BETA)
        want, r = _stream(eng, encp, [], W, S)
        score, logp = r.floats()
        print(f"kind {kind} lm {lm_seed}: {len(want[0])} tokens, score {score:.6f} (float64 {ref['score']:.6f}), logp {logp:.6f} "
              f"(float64 {ref['logp']:.6f}), margin {margin:.3e}, bar {bar:.3e}")
        assert want[0] == ref["ids"] and want[1] == ref["frames"]
        assert abs(score - ref["score"]) <= BC.bar(ref["score"]) and abs(logp - ref["logp"]) <= BC.bar(ref["logp"])
        rng = np.random.default_rng(17)
        uneven = sorted(int(v) for v in rng.choice(np.arange(1, len(encp)), 16, replace=False))
        for cuts in ([P - 1], [P], [P + 1], uneven):
            got, _ = _stream(eng, encp, cuts, W, S)
            assert got == want, cuts
    finally:
        _clear(eng)


# ---- (e) large frame numbers
def test_a_stream_begun_near_the_end_of_the_integer_range():
    from gigaam_amd._lib import GigaAMHipError
    eng = _engine("D", 1, "dense")
    c = HC.beam_cases("D", 1, "dense")[3]
    W, S = c["W"], c["S"]
    rows = np.concatenate([c["encp"][0], c["encp"][3][:2]])
    assert len(rows) == 12
    try:
        eng.set_hotwords(c["phrases"], HC.BETA)
        local, _ = _stream(eng, rows, [5], W, S)
        assert len(local[0]) > 0
        t_base = 2 ** 31 - 1 - 12
        r = Raw(eng, W, S, 13)
        assert r.call(rows[:5], t_base, BEGIN) == 1 and r.call(rows[5:], t_base + 5, 0) == 1
        before = r.snapshot()
        with pytest.raises(GigaAMHipError, match="below 2\\^31"):      # one more row: frame 2^31 - 1 would make t_base + n = 2^31
            r.call(rows[:1], t_base + 12, 0)
        assert all(torch.equal(x, y) for x, y in zip(before, r.snapshot()))
        assert r.call(None, t_base + 12, END) == 1
        ids, frames, sc, lp = r.result()
        assert ids == local[0] and frames == [t_base + f for f in local[1]] and max(frames) < 2 ** 31 and (sc, lp) == local[2:]
    finally:
        _clear(eng)


# ---- (f) refusals and host errors
def test_refused_calls_leave_everything_alone_and_the_stream_carries_on(tmp_path):
    eng, other = _engine("C", 1, "dense"), _engine("D", 1, "dense")      # H / JH differ; D's record is the smaller one
    c = HC.lm_cases("C", 1)[1]
    W, S, T = c["W"], c["S"], HC.T
    rows = c["encp"][0]
    orows = torch.zeros((2, int(other.cfg.joint_hidden)), device=DEV)
    tok = BC.tokenizer(HC.sizes("C")[0])
    try:
        _clear(other)
        eng.set_hotwords(c["phrases"], HC.BETA)
        eng.set_lm(None)
        want, _ = _stream(eng, rows, [], W, S)
        r = Raw(eng, W, S, T, state_words=4096)      # room for the record of another W or S: those calls reach the kernel
        assert r.nbytes > int(eng.lib.gam_rnnt_beam_stream_bytes(eng._h, W + 1, S + 1, T))

        def refused(*a, **kw):
            before = r.snapshot()
            assert r.call(*a, **kw) == 0, (a, kw)
            after = r.snapshot()
            assert torch.equal(before[0], after[0]), (a, kw)
            # every output word but the status is untouched
            st = r.out.status.data_ptr() - r.out.whole.data_ptr()
            b, a_ = before[1].clone(), after[1].clone()
            b[st // 4] = a_[st // 4] = 0
            assert torch.equal(b, a_), (a, kw)

        refused(rows[:4], 0, 0)                                # never begun (a zeroed record)
        refused(None, 0, END)
        refused(rows, 0, BEGIN, state_bytes=r.exact - 16)      # BEGIN with more rows than the pool holds
        assert r.call(rows[:4], 0, BEGIN) == 1
        refused(rows[4:6], 3, 0)                               # a frame given twice
        refused(rows[4:6], 5, 0)                               # a frame skipped
        refused(rows[4:6], 4, 0, W=W + 1)                      # another W
        refused(rows[4:6], 4, 0, S=S + 1)                      # another S
        refused(orows, 4, 0, eng=other)                        # another head's engine on this record
        refused(None, 4, END, eng=other)
        refused(rows[4:], 4, 0, state_bytes=r.exact - 16)      # a smaller pool than BEGIN saw
        eng.set_hotwords(c["phrases"], HC.BETA + 1.0)          # set_hotwords between two pushes
        refused(rows[4:6], 4, 0)
        eng.set_hotwords(c["phrases"], HC.BETA)                # (the same set again is another generation still)
        refused(rows[4:6], 4, 0)
        # a second record, begun under the set at hand now: set_lm between two pushes, rows beyond max_frames
        r2, r = r, Raw(eng, W, S, T - 1)
        assert r.call(rows[:4], 0, BEGIN) == 1
        eng.set_lm(_lm(tmp_path, c["arpa"]), tok, I.LM_ALPHA, I.LM_BETA)
        refused(rows[4:6], 4, 0)
        eng.set_lm(None)
        refused(rows[4:6], 4, 0)
        r = Raw(eng, W, S, T - 1)
        assert r.call(rows[:4], 0, BEGIN) == 1
        refused(rows[4:], 4, 0)                                # rows beyond max_frames (6 more into a pool of 9)
        assert r.call(rows[4:T - 1], 4, END) == 1              # the right call carries on
        refused(None, T - 1, 0)                                # ended
        refused(None, T - 1, END)
        refused(rows[:1], T - 1, 0)
        assert r.call(rows, 7, BEGIN | END, state_bytes=None) == 0      # BEGIN starts over whatever the record held -- but not beyond the pool
        r = Raw(eng, W, S, T)
        assert r.call(rows[:3], 0, BEGIN | END) == 1 and r.call(rows, 7, BEGIN | END) == 1      # BEGIN on an ended record
        got = r.result()
        assert got[0] == want[0] and got[1] == [f + 7 for f in want[1]] and got[2:] == want[2:]
        del r2
    finally:
        _clear(eng)
        _clear(other)


def test_the_stream_object_raises_after_finish_and_after_a_refusal():
    from gigaam_amd._lib import GigaAMHipError
    eng = _engine("C", 1, "dense")
    c = HC.beam_cases("C", 1, "dense")[3]
    W, S = c["W"], c["S"]
    rows = torch.from_numpy(c["encp"][0])
    try:
        eng.set_hotwords(c["phrases"], HC.BETA)
        want, _ = _stream(eng, c["encp"][0], [], W, S)
        for overlap in (False, True):
            st = eng.rnnt_beam_stream(W, HC.T, S)
            st.push(rows[:3], overlap=overlap)
            st.push(rows[3:3], overlap=overlap)
            st.push(rows[3:], overlap=overlap)
            out = st.finish()
            assert int(out.ids.shape[0]) == HC.T * S
            h = out.host()
            assert (h["ids"].tolist(), h["frames"].tolist()) == want[:2] and h["status"] == 1 and h["count"] == len(want[0])
            assert (int(np.float64(h["score"]).view(np.int64)), int(np.float64(h["logp"]).view(np.int64))) == want[2:]
            with pytest.raises(GigaAMHipError, match="has ended"):
                st.push(rows[:1])
            with pytest.raises(GigaAMHipError, match="has ended"):
                st.finish()
        with pytest.raises(GigaAMHipError, match="must be"):
            eng.rnnt_beam_stream(W, 4, S).push(torch.zeros((2, 3)))
        st = eng.rnnt_beam_stream(W, HC.T, S)      # set_hotwords during the stream: the last call is refused, host() says so
        st.push(rows[:3])
        eng.set_hotwords([])
        st.push(rows[3:])
        with pytest.raises(GigaAMHipError, match="refused"):
            st.finish().host()
        over = eng.rnnt_beam_stream(W, 4, S)        # more rows than max_frames
        over.push(rows[:5])
        with pytest.raises(GigaAMHipError, match="refused"):
            over.finish().host()
        empty = eng.rnnt_beam_stream(W, 0, S).finish().host()      # a stream without a frame
        assert empty["count"] == 0 and empty["score"] == 0.0 and empty["logp"] == 0.0
    finally:
        _clear(eng)


def test_host_errors_are_raised_without_a_launch(tmp_path):
    from gigaam_amd._lib import GigaAMHipError
    eng = _engine("C", 1, "dense")
    c = HC.lm_cases("C", 1)[1]
    W, S = c["W"], c["S"]
    rows = torch.from_numpy(c["encp"][0][:8]).to(DEV)
    try:
        _clear(eng)
        r = Raw(eng, W, S, 8)
        before = r.snapshot()
        for kw in (dict(t_base=-1), dict(t_base=2 ** 31 - 8), dict(W=0), dict(W=33), dict(S=0), dict(S=17), dict(cap=-1), dict(flags=4),
                   dict(state_bytes=_fixed_bytes(eng, W, S) - 4)):
            args = dict(t_base=0, flags=BEGIN)
            args.update(kw)
            with pytest.raises(GigaAMHipError, match="RNN-T beam stream"):
                r.call(rows, args.pop("t_base"), args.pop("flags"), **args)
        for bad in ((0, S, 8), (33, S, 8), (W, 0, 8), (W, 17, 8), (W, S, -1), (32, 16, 2 ** 22)):
            assert int(eng.lib.gam_rnnt_beam_stream_bytes(eng._h, *bad)) < 0, bad
        with pytest.raises(GigaAMHipError, match="RNN-T beam stream"):
            eng.rnnt_beam_stream(32, 2 ** 22, 16)
        # a hotword id >= V - 1; an LM whose classes are for another V
        eng.set_hotwords([[3, HC.sizes("C")[0] - 1]], HC.BETA)
        with pytest.raises(GigaAMHipError, match="hotword token id"):
            r.call(rows, 0, BEGIN)
        eng.set_hotwords([])
        f = _engine("F", 1, "dense")
        f.set_lm(_lm(tmp_path, c["arpa"]), BC.tokenizer(34), I.LM_ALPHA, I.LM_BETA)
        try:
            rf = Raw(f, 4, 1, 2)
            with pytest.raises(GigaAMHipError, match="token classes are for V=34"):
                rf.call(torch.zeros((2, int(f.cfg.joint_hidden))), 0, BEGIN)
        finally:
            f.set_lm(None)
        assert all(torch.equal(x, y) for x, y in zip(before, r.snapshot()))
        # what the wrapper cannot express: n < 0 and NULL buffers, through the C ABI
        lib, p = eng.lib, lambda t: C.c_void_p(t.data_ptr())
        o = r.out
        full = [p(rows), 8, 0, BEGIN | END, W, S, p(r.state), r.nbytes, p(o.ids), p(o.frames), 8 * S, p(o.count), p(o.score), p(o.logp),
                p(o.status), None]
        assert lib.gam_op_rnnt_beam_stream(eng._h, *full) == 0
        torch.cuda.synchronize()
        assert int(o.status.cpu()[0]) == 1
        want = r.result()
        for i, bad in ((1, -1), (0, None), (6, None), (8, None), (9, None), (11, None), (12, None), (13, None), (14, None)):
            a = list(full)
            a[i] = bad
            assert lib.gam_op_rnnt_beam_stream(eng._h, *a) != 0, i
        a = list(full)
        a[6] = C.c_void_p(r.state.data_ptr() + 4)      # a record that is not 16-byte aligned (its entries and nodes are int4)
        assert lib.gam_op_rnnt_beam_stream(eng._h, *a) != 0 and b"16-byte aligned" in lib.gam_last_error(eng._h)
        assert lib.gam_op_rnnt_beam_stream(eng._h, None, 0, 0, BEGIN | END, *full[4:]) == 0      # encp may be NULL when n = 0
        torch.cuda.synchronize()
        assert int(o.count.cpu()[0]) == 0
        assert want == _stream(eng, rows, [], W, S)[0]
        # a head that is not RNN-T
        ctc = BC.ctc_op_engine("rnnt_beam_stream")
        with pytest.raises(GigaAMHipError, match="RNN-T"):
            ctc.rnnt_beam_stream(W, 8, S)
        with pytest.raises(GigaAMHipError, match="RNN-T"):
            ctc.op_rnnt_beam_stream(rows, 0, BEGIN, W, S, r.state, r.nbytes, r.out)
        # LDS over the limit: A at L = 2, (32, 16) fits without the LM and not with it
        a2 = _engine("A", 2, HC.EDGE_KIND)
        need = HC.rb_lds_bytes("A", 2, *HC.WS_EDGE, with_lm=True)
        a2.set_lm(_lm(tmp_path, HC.lm_cases("A", 2)[0]["arpa"], 1), BC.tokenizer(34), 0.5, 1.0)
        try:
            ra = Raw(a2, *HC.WS_EDGE, 2)
            with pytest.raises(GigaAMHipError, match=f"with the LM need {need} bytes"):
                ra.call(torch.zeros((2, 512)), 0, BEGIN | END)
            a2.set_lm(None)
            assert ra.call(torch.zeros((2, 512)), 0, BEGIN | END) == 1
        finally:
            a2.set_lm(None)
    finally:
        _clear(eng)
