"""GPU: the resumable RNN-T greedy decode (gam_op_rnnt_greedy_stream, gigaam_amd/csrc/gam_rnnt_stream.h) with the two calls it
needs (gam_rnnt_encp, gam_op_rnnt_greedy), at the op level.

Exactness.  Against float64: the heads of tests/rnnt_cluster_cases.py and head C with two predictor layers
(tests/rnnt_stream_ref.py) are decided by margins of at least 1.2e-2 by the float64 reference (asserted on the CPU:
tests/test_rnnt_cluster_plan_host.py, tests/test_rnnt_stream_host.py), an order of magnitude above the 1e-3 log-prob bar, so ids,
frames and counts are compared exactly.  Against the batch kernel and between cuttings of one stream the comparison is bit for bit
whatever the margin: both run one device function on the same rows.  Every comparison with the batch kernel is made at cluster
size 0 (the one-workgroup arithmetic), and the setting is restored afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_common as BC
import rnnt_cluster_cases as K
import rnnt_head_cases as HC
import rnnt_stream_ref as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S = K.MAX_SYMBOLS
BEGIN, END = SR.BEGIN, SR.END
CASES = [("A", 1), ("C", 1), ("D", 1), ("E", 1), ("F", 1), ("C", 2)]

_ENGINES = {}


def _case(name, L):
    """(cfg, state dict, encoded, lengths, float64 traces) of a head."""
    if L == 2:
        assert name == "C"
        return SR.l2_case()
    return (*K.inputs(name), K.reference(name))


def _engine_of(key, cfg, sd):
    if key not in _ENGINES:
        from gigaam_amd.engine import HipEngine, build_config
        _ENGINES[key] = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), sd, torch.device(DEV))
    return _ENGINES[key]


def _engine(name, L):
    cfg, sd = _case(name, L)[:2]
    return _engine_of((name, L), cfg, sd)


@pytest.fixture
def cluster0():
    """Run at cluster size 0 on every engine made so far and in the test; restore what the user had set."""
    saved = {}

    def use(eng):
        if id(eng) not in saved:
            saved[id(eng)] = (eng, getattr(eng, "_rnnt_cluster_user", -1))
            eng.set_rnnt_cluster(0)
        return eng

    yield use
    for eng, c in saved.values():
        eng.set_rnnt_cluster(c)


class Raw:
    """A state record, a one-row result and a status word, driven call by call through ``op_rnnt_greedy_stream``."""

    def __init__(self, eng, cap, state_words=None):
        from gigaam_amd.engine import Decoded
        self.eng = eng
        self.nbytes = int(eng.lib.gam_rnnt_greedy_stream_bytes(eng._h))
        assert self.nbytes == 64 + 2 * int(eng.cfg.pred_rnn_layers) * int(eng.cfg.pred_hidden) * 4
        self.state = torch.zeros((state_words or self.nbytes // 4,), dtype=torch.int32, device=DEV)
        self.out = Decoded.packed(torch.device(DEV), 1, max(cap, 1))
        self.out.whole.fill_(-7)
        self.status = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        self.cap = cap

    def call(self, rows, t_base, flags, max_symbols=S, cap=None, eng=None, state_bytes=None):
        eng = eng or self.eng
        rows = None if rows is None or len(rows) == 0 else torch.as_tensor(rows, dtype=torch.float32, device=DEV).contiguous()
        with torch.cuda.device(torch.device(DEV)):
            eng.op_rnnt_greedy_stream(rows, t_base, flags, max_symbols, self.state, self.state.numel() * 4 if state_bytes is None else state_bytes,
                                      self.out, self.status, self.cap if cap is None else cap)
        return int(self.status.cpu()[0])

    def count(self):
        return int(self.out.counts.cpu()[0])

    def result(self):
        n = self.count()
        return self.out.ids[0, :n].cpu().tolist(), self.out.frames[0, :n].cpu().tolist(), n

    def snapshot(self):
        torch.cuda.synchronize()
        return self.state.clone(), self.out.whole.clone()


def _one_call(eng, rows, t_base=0):
    r = Raw(eng, len(rows) * S)
    assert r.call(rows, t_base, BEGIN | END) == 1
    return r.result()


def _cut(eng, rows, cuts, end_alone=False):
    """The stream cut at ``cuts``; returns (ids, frames, count) and the count after every call that carried rows or was empty."""
    edges = [0] + list(cuts) + [len(rows)]
    r, counts = Raw(eng, len(rows) * S), []
    for j, (a, b) in enumerate(zip(edges, edges[1:])):
        last = j == len(edges) - 2
        assert r.call(rows[a:b], a, (BEGIN if j == 0 else 0) | (END if last and not end_alone else 0)) == 1, (cuts, j)
        counts.append(r.count())
    if end_alone:
        assert r.call(None, len(rows), END) == 1
    return r.result(), counts


def _batch_rows(dec):
    torch.cuda.synchronize()
    ids, frames, counts = (x.cpu().numpy() for x in dec[:3])
    return [(ids[b, :counts[b]].tolist(), frames[b, :counts[b]].tolist(), int(counts[b])) for b in range(len(counts))]


@pytest.mark.parametrize("name,L", CASES)
def test_one_call_streams_match_float64_and_the_batch_kernel(name, L, cluster0):
    _, _, encoded, lengths, ref = _case(name, L)
    eng = cluster0(_engine(name, L))
    enc_t, len_t = torch.from_numpy(encoded), torch.tensor(lengths, dtype=torch.int32)
    encp = eng.rnnt_encp(enc_t)
    assert tuple(encp.shape) == (len(lengths), K.T_MAX, int(eng.cfg.joint_hidden))
    whole = _batch_rows(eng.op_rnnt_greedy(encp, len_t, S))
    assert eng.rnnt_last_decode() == (0, -1, False)
    # op_rnnt_greedy on the whole batch is rnnt_greedy(encoded) bit for bit: the same projection GEMM, the same kernel
    assert whole == _batch_rows(eng.rnnt_greedy(enc_t, len_t, S))
    for b, T in enumerate(lengths):
        got = _one_call(eng, encp[b, :T])
        print(f"head {name} L={L} utterance {b}: {got[2]} tokens, reference {len(ref[b]['ids'])}, margin {ref[b]['margin']:.3e}")
        assert got == (ref[b]["ids"], ref[b]["frames"], len(ref[b]["ids"])), (name, L, b)
        assert got == whole[b], (name, L, b)
        assert got == _batch_rows(eng.op_rnnt_greedy(encp[b:b + 1], len_t[b:b + 1], S))[0], (name, L, b)


@pytest.mark.parametrize("name,L", [("C", 1), ("A", 1), ("F", 1), ("C", 2)])
def test_cut_invariance_on_utterance_0(name, L, cluster0):
    """Utterance 0: 60 frames with a quiet span of more than two windows.  Every cutting gives the single call's bits, and the count
    after every call is the reference's prefix count."""
    _, _, encoded, lengths, ref = _case(name, L)
    eng = cluster0(_engine(name, L))
    rows = eng.rnnt_encp(torch.from_numpy(encoded[:1]))[0]
    per = ref[0]["per_frame"]
    T = lengths[0]
    want = _one_call(eng, rows)
    assert want == (ref[0]["ids"], ref[0]["frames"], len(ref[0]["ids"]))
    emitting = next(t for t in range(1, T) if per[t] > 0)                      # a call that begins at an emitting frame
    after_capped = next(t + 1 for t in range(T - 1) if per[t] == S)             # ... and one behind a frame that stopped at max_symbols
    cuttings = [[1], [15], [16], [17], [20], [emitting], [after_capped], list(range(1, T)), [20, 20], [0, 33, T]]
    for cuts in cuttings:
        got, counts = _cut(eng, rows, cuts)
        assert got == want, (name, cuts)
        assert counts == [sum(per[:p]) for p in cuts + [T]], (name, cuts)
    got, counts = _cut(eng, rows, [16, 40], end_alone=True)
    assert got == want and counts == [sum(per[:16]), sum(per[:40]), sum(per)]


def test_nine_thousand_frames_in_one_call_and_in_random_cuttings(cluster0):
    """Head C, blank-dominant, on 9000 frames of seeded encp: one call, three random cuttings and op_rnnt_greedy agree bit for bit."""
    cfg, sd, _ = HC.head("C", 1, "blank")
    eng = cluster0(_engine_of(("C", 1, "blank"), cfg, sd))
    T = 9000
    encp = torch.from_numpy(BC.encp(np.random.default_rng(90), 1, T, HC.sizes("C")[2], HC.ENCP_SCALE)).to(DEV)
    want = _one_call(eng, encp[0])
    print(f"9000 frames: {want[2]} tokens")
    assert 20 < want[2] < T * S and want[1] == sorted(want[1]) and want[1][-1] > 8192
    assert want == _batch_rows(eng.op_rnnt_greedy(encp, torch.tensor([T], dtype=torch.int32), S))[0]
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        cuts = sorted(int(c) for c in rng.integers(0, T + 1, size=int(rng.integers(2, 40))))
        got, _ = _cut(eng, encp[0], cuts)
        assert got == want, (seed, cuts)


def test_a_stream_begun_near_the_end_of_the_integer_range(cluster0):
    _, _, encoded, lengths, ref = _case("C", 1)
    eng = cluster0(_engine("C", 1))
    rows = eng.rnnt_encp(torch.from_numpy(encoded[:1]))[0][:40]
    local = _one_call(eng, rows)
    assert local[2] > 0
    t_base = 2 ** 31 - 1 - 40
    r = Raw(eng, 40 * S)
    assert r.call(rows[:17], t_base, BEGIN) == 1 and r.call(rows[17:], t_base + 17, END) == 1
    ids, frames, n = r.result()
    assert (ids, n) == (local[0], local[2]) and frames == [t_base + f for f in local[1]] and max(frames) < 2 ** 31


def test_two_streams_through_two_states_on_either_stream(cluster0):
    """Two streams pushed alternately through two ``RnntGreedyStream`` objects, on the launch stream and on the decode side stream:
    the same bits as each stream alone."""
    from gigaam_amd.engine import HipEngine
    _, _, encoded, lengths, ref = _case("C", 1)
    eng = cluster0(_engine("C", 1))
    encp = eng.rnnt_encp(torch.from_numpy(encoded[:2]))
    rows = [encp[0, :lengths[0]], encp[1, :lengths[1]]]
    want = [_one_call(eng, r)[:2] for r in rows]
    for overlap in (False, True):
        st = [eng.rnnt_greedy_stream(len(r), S) for r in rows]
        for a in range(0, K.T_MAX, 7):
            for k in (0, 1):
                if a < len(rows[k]):
                    st[k].push(rows[k][a:a + 7], overlap=overlap)
        for k in (1, 0):
            dec = st[k].finish()
            got, flag = HipEngine.collect(dec)
            st[k].check()
            assert not flag and got[0] == want[k], (overlap, k)
            assert int(dec.frames.shape[1]) == len(rows[k]) * S
    st = eng.rnnt_greedy_stream(0, S)           # a stream without a frame
    got, _ = HipEngine.collect(st.finish())
    st.check()
    assert got == [([], [])]
    from gigaam_amd._lib import GigaAMHipError
    with pytest.raises(GigaAMHipError, match="has ended"):
        st.push(rows[0][:1])
    with pytest.raises(GigaAMHipError, match="must be"):
        eng.rnnt_greedy_stream(4, S).push(torch.zeros((2, 3)))
    over = eng.rnnt_greedy_stream(4, S)        # more rows than max_frames: refused, and ``check`` says so
    over.push(rows[0][:5])
    over.finish()
    with pytest.raises(GigaAMHipError, match="refused"):
        over.check()


def test_refused_calls_leave_everything_alone_and_the_stream_carries_on(cluster0):
    _, _, encoded, lengths, ref = _case("C", 1)
    eng = cluster0(_engine("C", 1))
    others = [cluster0(_engine("D", 1)), cluster0(_engine("C", 2)), cluster0(_engine("F", 1))]     # H / JH, L, V and H / JH differ
    rows = eng.rnnt_encp(torch.from_numpy(encoded[:1]))[0]
    other_rows = [torch.zeros((4, int(o.cfg.joint_hidden)), device=DEV) for o in others]
    want = _one_call(eng, rows)
    T = lengths[0]
    big = (64 + 2 * 2 * 512 * 4) // 4          # a buffer that holds the record of every head here
    r = Raw(eng, T * S, state_words=big)

    def refused(*a, **kw):
        before = r.snapshot()
        r.status.fill_(-7)
        assert r.call(*a, **kw) == 0, (a, kw)
        after = r.snapshot()
        assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]), (a, kw)

    refused(rows[:20], 0, 0)                                   # never begun (a zeroed record)
    refused(None, 0, END)
    refused(rows[:20], 0, BEGIN, cap=20 * S - 1)               # BEGIN that could overflow cap
    assert r.call(rows[:20], 0, BEGIN) == 1
    n20 = r.count()
    refused(rows[20:30], 19, 0)                                # a frame given twice
    refused(rows[20:30], 21, 0)                                # a frame skipped
    refused(rows[20:30], 20, 0, max_symbols=S + 1)             # max_symbols changed
    refused(rows[20:30], 20, 0, cap=n20 + 10 * S - 1)          # could overflow cap
    for o, orow in zip(others, other_rows):                    # another head's engine on this record
        refused(orow, 20, 0, eng=o)
        refused(None, 20, END, eng=o)
    assert r.call(rows[20:30], 20, 0, cap=n20 + 10 * S) == 1   # the right call: exactly enough room
    assert r.call(rows[30:], 30, END) == 1
    refused(None, T, 0)                                        # ended
    refused(None, T, END)
    refused(rows[:1], T, 0)
    assert r.result() == want
    assert r.call(rows[:20], 5, BEGIN) == 1                    # BEGIN starts over, whatever the record held
    assert r.result()[0] == _one_call(eng, rows[:20])[0] and r.result()[1][0] >= 5


def test_host_errors_are_raised_without_a_launch():
    from gigaam_amd import synth
    from gigaam_amd._lib import GigaAMHipError
    from gigaam_amd.engine import HipEngine, build_config
    eng = _engine("C", 1)
    _, _, encoded, _, _ = _case("C", 1)
    rows = eng.rnnt_encp(torch.from_numpy(encoded[:1]))[0][:8]
    r = Raw(eng, 8 * S)
    before = r.snapshot()
    for kw in (dict(t_base=-1), dict(t_base=2 ** 31 - 8), dict(max_symbols=0), dict(cap=-1), dict(state_bytes=r.nbytes - 4), dict(flags=4)):
        args = dict(t_base=0, flags=BEGIN, max_symbols=S)
        args.update(kw)
        with pytest.raises(GigaAMHipError, match="RNN-T greedy stream"):
            r.call(rows, args.pop("t_base"), args.pop("flags"), **args)
    assert all(torch.equal(x, y) for x, y in zip(before, r.snapshot()))
    # what the wrapper cannot express: n < 0 and NULL buffers, through the C ABI
    lib, p = eng.lib, lambda t: C.c_void_p(t.data_ptr())
    full = [p(rows), 8, 0, BEGIN, S, p(r.state), r.nbytes, p(r.out.ids), p(r.out.frames), 8 * S, p(r.out.counts), p(r.status), None]
    assert lib.gam_op_rnnt_greedy_stream(eng._h, *full) == 0
    torch.cuda.synchronize()
    assert int(r.status.cpu()[0]) == 1
    for i, bad in ((1, -1), (0, None), (5, None), (7, None), (8, None), (10, None), (11, None)):
        a = list(full)
        a[i] = bad
        assert lib.gam_op_rnnt_greedy_stream(eng._h, *a) != 0, i
    assert lib.gam_op_rnnt_greedy_stream(eng._h, None, 0, 8, END, S, *full[5:]) == 0      # encp may be NULL when n = 0
    torch.cuda.synchronize()
    assert int(r.status.cpu()[0]) == 1 and r.result() == _one_call(eng, rows)
    # a head that is not RNN-T
    cfg = synth.model_cfg("v2_ctc", n_layers=1)
    ctc = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), synth.make_state_dict(cfg, seed=0), torch.device(DEV))
    with pytest.raises(GigaAMHipError, match="RNN-T"):
        ctc.rnnt_greedy_stream(8, S)
    with pytest.raises(GigaAMHipError, match="RNN-T"):
        ctc.op_rnnt_greedy_stream(rows, 0, BEGIN, S, r.state, r.nbytes, r.out, r.status)
    with pytest.raises(GigaAMHipError, match="RNN-T"):
        ctc.rnnt_encp(torch.from_numpy(encoded[:1]))
    # LDS over the limit: V = 2048 at H = JH = 512 needs 184960 bytes, and W_out does not fit LDS either
    cfg = K.head_cfg("A")
    cfg["head"]["decoder"]["num_classes"] = cfg["head"]["joint"]["num_classes"] = 2048
    huge = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), synth.make_state_dict(cfg, seed=0), torch.device(DEV))
    rh = Raw(huge, 8 * S)
    with pytest.raises(GigaAMHipError, match="LDS"):
        rh.call(torch.zeros((8, 512)), 0, BEGIN | END)
    for e in (ctc, huge):
        e.close()
