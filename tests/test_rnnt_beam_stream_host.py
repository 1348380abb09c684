"""Host: the resumable RNN-T beam search without a GPU -- the float64 twin of tests/rnnt_beam_stream_ref.py against
``R.beam_search`` in one call and at every cutting, its refusals, the headers' flags, the keyword errors of
``transcribe_longform(stream_decode="beam")``, and the qualification of the long-stream inputs of
tests/test_hip_rnnt_beam_stream.py's rebase test."""
import itertools
import os
import re

import numpy as np
import pytest

import rnnt_beam_ref as R
import rnnt_beam_stream_ref as SB
import rnnt_head_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lm_spec(text, V):
    import beam_common as BC
    import ctc_lm_ref as CL
    import nbest_inputs as I
    from gigaam_amd import lm as LM
    tok = BC.tokenizer(V)
    classes = [int(c) for c in LM.token_classes(tok)]
    arpa = CL.ArpaLM(text)
    spell = {}
    for w in sorted(arpa.words - {"<s>", "</s>", "<unk>"}):
        ids = LM.word_spelling(tok, w, classes)
        if ids:
            spell[tuple(ids)] = w
    return CL.LMSpec(arpa, classes, spell, I.LM_ALPHA, I.LM_BETA)


def _same(got, want):
    assert got["ids"] == list(want["ids"]) and got["frames"] == list(want["frames"])
    assert got["score"] == want["score"] and got["logp"] == want["logp"]
    assert got["beam"] == want["beam"]


# (head, L, kind, which combinations, which utterances): the sets of the GPU test's one-call comparison.  Every combination and
# utterance on the two small heads.  On the heads of 512 units (F, and A at L = 2) a float64 search takes seconds and a whole set
# up to 20 s (tests/rnnt_head_cases.py), and the suite runs for every later change: there, one short utterance (7 frames) of one
# combination (W = 4, S = 1, with hotwords) per kind -- the twin's frame step does not depend on the head's sizes, which only the
# predictor and the joint see, so these check that it runs on such heads, not new paths of it.
SETS = [("C", 1, "blank", None, None), ("C", 1, "dense", None, None), ("D", 1, "blank", None, None), ("D", 1, "dense", None, None),
        ("F", 1, "blank", [1], [1]), ("F", 1, "dense", [1], [1]), ("A", 2, "blank", [1], [1]), ("A", 2, "dense", [1], [1])]


@pytest.mark.parametrize("name,L,kind,which,utts", SETS)
def test_one_call_of_the_twin_is_the_batch_reference(name, L, kind, which, utts):
    hd = HC.head(name, L, kind)[2]
    for i, c in enumerate(HC.beam_cases(name, L, kind)):
        if which is not None and i not in which:
            continue
        for b in (range(HC.B) if utts is None else utts):
            T = HC.ENC_LEN[b]
            rows = c["encp"][b, :T].astype(np.float64)
            want = R.beam_search(hd, rows, c["W"], c["S"], T, c["phrases"], HC.BETA)
            got, _ = SB.stream(hd, rows, [], c["W"], c["S"], c["phrases"], HC.BETA)
            _same(got, want)
            assert got["margins"] == want["margins"] and got["final_margin"] == want["final_margin"]
            # and what the file of stored references holds for the GPU test
            ref = c["refs"][b]
            assert got["ids"] == ref["ids"] and got["frames"] == ref["frames"] and got["score"] == pytest.approx(ref["score"], abs=1e-9)


@pytest.mark.parametrize("name,L,which,utts", [("C", 1, None, None), ("A", 2, [1], [1])])
def test_one_call_of_the_twin_with_the_lm(name, L, which, utts):
    """The LM sets of the GPU test: every combination and utterance of ("C", 1); of ("A", 2), a head of 512 units, one short utterance
    of one combination (W = 4, S = 1, order 3, with hotwords), for the runtime reason above."""
    hd = HC.head(name, L, "dense")[2]
    V = HC.sizes(name)[0]
    for i, c in enumerate(HC.lm_cases(name, L)):
        if which is not None and i not in which:
            continue
        spec = _lm_spec(c["arpa"], V)
        for b in (range(HC.B) if utts is None else utts):
            T = HC.ENC_LEN[b]
            rows = c["encp"][b, :T].astype(np.float64)
            want = R.beam_search(hd, rows, c["W"], c["S"], T, c["phrases"], HC.BETA, lm=spec)
            got, _ = SB.stream(hd, rows, [], c["W"], c["S"], c["phrases"], HC.BETA, lm=spec)
            _same(got, want)
            assert got["lm"] == want["lm"]


def _cuttings(T):
    """Every cutting of T rows into non-empty calls, then some with empty calls."""
    for k in range(T):
        for cuts in itertools.combinations(range(1, T), k):
            yield list(cuts), False
    for cuts in ([0], [T], [0, 0, 4, 4, 4, T, T], [3, 3], list(range(1, T))):
        yield cuts, False
        yield cuts, True


@pytest.mark.parametrize("kind,with_lm", [("dense", False), ("blank", False), ("dense", True)])
def test_every_cutting_of_a_ten_frame_stream_gives_the_uncut_result(kind, with_lm):
    """Head D (the LM case: head C), W = 4, S = 1 with hotwords (combination 1), utterance 0: 512 cuttings into non-empty calls, cuttings
    with empty calls, END alone.  The carried beam is all the twin keeps, so this is the proof that the record's entry fields suffice."""
    if with_lm:
        c = HC.lm_cases("C", 1)[1]
        hd, lm = HC.head("C", 1, "dense")[2], I_small_lm(c)
    else:
        c = HC.beam_cases("D", 1, kind)[1]
        hd, lm = HC.head("D", 1, kind)[2], None
    rows = c["encp"][0, :HC.T].astype(np.float64)
    want = R.beam_search(hd, rows, c["W"], c["S"], HC.T, c["phrases"], HC.BETA, lm=lm)
    assert c["phrases"] and len(want["ids"]) > 0
    n = 0
    for cuts, end_alone in _cuttings(HC.T):
        if with_lm and len(cuts) > 2 and cuts != list(range(1, HC.T)):
            continue
        got, rec = SB.stream(hd, rows, cuts, c["W"], c["S"], c["phrases"], HC.BETA, lm, end_alone=end_alone)
        _same(got, want)
        assert got["margins"] == want["margins"] and rec["next"] == HC.T
        n += 1
    assert n >= (40 if with_lm else 512)
    # a stream that starts at another frame: the same tokens, frames shifted
    got, _ = SB.stream(hd, rows, [3], c["W"], c["S"], c["phrases"], HC.BETA, lm, t0=1000)
    assert got["ids"] == want["ids"] and got["frames"] == [f + 1000 for f in want["frames"]] and got["score"] == want["score"]


def I_small_lm(c):
    return _lm_spec(c["arpa"], HC.sizes("C")[0])


def test_what_the_twin_refuses():
    c = HC.beam_cases("D", 1, "dense")[1]
    hd = HC.head("D", 1, "dense")[2]
    other = HC.head("C", 1, "dense")[2]
    rows = c["encp"][0].astype(np.float64)
    W, S = c["W"], c["S"]
    rec = SB.new_record()
    assert SB.call(hd, rec, rows[:5], 0, 0, W, S) == 0 and rec == SB.new_record()                       # not begun
    assert SB.call(hd, rec, rows[:5], 7, SB.BEGIN, W, S, max_frames=9, gens=(3, 4)) == 1 and rec["next"] == 12
    before = {k: v for k, v in rec.items() if k != "pred"}
    kw = dict(max_frames=9, gens=(3, 4))
    assert SB.call(hd, rec, rows[5:9], 11, 0, W, S, **kw) == 0                                          # a frame given twice
    assert SB.call(hd, rec, rows[5:9], 13, 0, W, S, **kw) == 0                                          # a frame skipped
    assert SB.call(hd, rec, rows[5:9], 12, 0, W + 1, S, **kw) == 0                                      # another W
    assert SB.call(hd, rec, rows[5:9], 12, 0, W, S + 1, **kw) == 0                                      # another S
    assert SB.call(other, rec, rows[5:9], 12, 0, W, S, **kw) == 0                                       # another head
    assert SB.call(hd, rec, rows[5:9], 12, 0, W, S, max_frames=9, gens=(4, 4)) == 0                     # set_hotwords since BEGIN
    assert SB.call(hd, rec, rows[5:9], 12, 0, W, S, max_frames=9, gens=(3, 5)) == 0                     # set_lm since BEGIN
    assert SB.call(hd, rec, rows[5:10], 12, 0, W, S, **kw) == 0                                         # rows beyond max_frames
    assert SB.call(hd, rec, rows[5:9], 12, 0, W, S, max_frames=8, gens=(3, 4)) == 0                     # a smaller pool than BEGIN saw
    assert {k: v for k, v in rec.items() if k != "pred"} == before
    assert SB.call(hd, rec, rows[5:9], 12, SB.END, W, S, **kw) == 1 and rec["result"]["frames"] == sorted(rec["result"]["frames"])
    assert SB.call(hd, rec, None, 16, 0, W, S, **kw) == 0                                               # ended
    # with or without BEGIN: more rows than the pool holds, frames at 2^31
    rec2 = SB.new_record()
    assert SB.call(hd, rec2, rows[:10], 0, SB.BEGIN, W, S, max_frames=9) == 0 and rec2 == SB.new_record()
    assert SB.call(hd, rec2, rows[:2], 2 ** 31 - 2, SB.BEGIN, W, S) == 0 and rec2 == SB.new_record()
    assert SB.call(hd, rec2, rows[:1], 2 ** 31 - 2, SB.BEGIN | SB.END, W, S) == 1 and rec2["result"]["frames"] in ([], [2 ** 31 - 2] * len(rec2["result"]["ids"]))
    # a stream without a frame
    rec3 = SB.new_record()
    assert SB.call(hd, rec3, None, 5, SB.BEGIN | SB.END, W, S) == 1
    assert (rec3["result"]["ids"], rec3["result"]["score"], rec3["result"]["logp"]) == ([], 0.0, 0.0)


def test_the_kernel_header_agrees_with_the_public_header():
    src = open(os.path.join(ROOT, "gigaam_amd", "csrc", "gam_rnnt_beam.h")).read()
    header = open(os.path.join(ROOT, "include", "gigaam_hip.h")).read()
    from gigaam_amd.engine import HipEngine, RnntBeamStream
    for f, v in (("BEGIN", SB.BEGIN), ("END", SB.END)):
        assert int(re.search(r"#define GAM_RB_F_" + f + r"\s+(\d+)", src).group(1)) == v
        assert int(re.search(r"#define GAM_RNNT_STREAM_" + f + r"\s+(\d+)", header).group(1)) == v
        assert getattr(RnntBeamStream, f) == v
    period = int(re.search(r"#define GAM_RB_STREAM_REBASE\s+(\d+)", src).group(1))
    assert period == SB.REBASE == HipEngine.RNNT_BEAM_STREAM_REBASE and period & (period - 1) == 0
    assert int(re.search(r"#define GAM_ABI_VERSION\s+(\d+)", header).group(1)) == 1


def test_stream_decode_beam_keyword_errors_need_no_gpu():
    import gigaam_amd
    from gigaam_amd import synth
    ctc = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=1, n_layers=1), "cpu")
    rnnt = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_rnnt", seed=1, n_layers=1), "cpu")
    path = "no-such-file.wav"       # (every error below is raised before the file is opened)
    # the checks stream_decode=True makes apply to "beam" unchanged
    for kw in (dict(), dict(speech_regions=[(0.0, 1.0)]), dict(vad="energy")):
        with pytest.raises(ValueError, match='decodes the stitched stream of vad="windows"'):
            rnnt.transcribe_longform(path, stream_decode="beam", **kw)
    with pytest.raises(TypeError, match="stream_decode needs an RNN-T head"):
        ctc.transcribe_longform(path, vad="windows", stream_decode="beam")
    for model in (ctc, rnnt):
        with pytest.raises(ValueError, match="a call takes one of them"):
            model.transcribe_longform(path, vad="windows", stream_search=True, stream_decode="beam", beam_size=4)
    for kw in (dict(beam_size=4), dict(hotwords=["да"]), dict(lm="missing.arpa")):
        with pytest.raises(TypeError, match="beam search needs a CTC head"):
            rnnt.transcribe_longform(path, vad="windows", stream_decode="beam", **kw)
    # "beam" with the greedy decoding object; any other string
    with pytest.raises(ValueError, match=r"select one with set_decoding\(beam_size=\.\.\.\)"):
        rnnt.transcribe_longform(path, vad="windows", stream_decode="beam")
    for bad in ("greedy", "Beam"):
        with pytest.raises(ValueError, match="stream_decode="):
            rnnt.transcribe_longform(path, vad="windows", stream_decode=bad)
    # a beam decoding object: True still raises what it raised, "beam" passes the keyword checks and segmentation keywords still fail
    rnnt.set_decoding(beam_size=4, hotwords=["да"])
    with pytest.raises(ValueError, match="RNN-T beam kernel stops at 8192 frames"):
        rnnt.transcribe_longform(path, vad="windows", stream_decode=True)
    with pytest.raises(ValueError, match="stream_decode="):
        rnnt.transcribe_longform(path, vad="windows", stream_decode="nbest")
    for kw in (dict(speech_regions=[(0.0, 1.0)]), dict(max_duration=20.0)):
        with pytest.raises(ValueError, match='vad="windows" takes no segmentation keywords'):
            rnnt.transcribe_longform(path, vad="windows", stream_decode="beam", **kw)
    with pytest.raises(Exception) as e:      # nothing left to refuse: the route itself starts, and a CPU model has no engine to plan with
        rnnt.transcribe_longform(path, vad="windows", stream_decode="beam")
    assert not isinstance(e.value, (ValueError, TypeError)) and "stream_decode" not in str(e.value)
    rnnt.set_decoding()
    with pytest.raises(TypeError, match="windowed longform needs a CTC head"):
        rnnt.transcribe_longform(path, vad="windows")


# ---- the long-stream inputs of the GPU test's rebase cases
LONG_CASES = [("blank", None), ("blank", 0), ("dense", None)]      # (kind, LM seed or None); tests/test_hip_rnnt_beam_stream.py runs these


@pytest.mark.parametrize("kind,lm_seed", LONG_CASES)
def test_the_long_stream_inputs_qualify(kind, lm_seed):
    """Head D, T = 2 periods + 40, W = 4, S = 3, six hotwords from the plain decode, boost 1.5, encp = 3 N(0, 1): the float64
    reference's smallest decision margin exceeds bar = max(HC.MARGIN, 8 x the fp32 ulp at the largest term the rebase-emulating twin
    reports).  The seed is the first from 0 up that qualifies; the LM seed likewise.  Measured here: blank seed 0 margin 1.9e-3, bar
    1.0e-4 (largest term 108; 202 without the rebase); dense seed 0 margin 4.92e-4, bar 4.88e-4 (largest term 649; without the rebase
    1358, where the bar would be 9.8e-4 and the input would not qualify: the rebase is what lets this stream be compared)."""
    seed, (ok, margin, bar, peak, res) = SB.first_seed(kind=kind)
    assert seed == SB.LONG_SEEDS[kind]
    hd, encp, phrases = SB.long_input(seed, kind)
    assert SB.LONG_T == 2 * SB.REBASE + 40 and len(phrases) == 6
    if lm_seed is not None:
        for s in range(lm_seed + 1):
            ok, margin, bar, peak, res = SB.long_qualifies(hd, encp, phrases, SB.long_lm(seed, hd, encp, s)[1])
            assert ok == (s == lm_seed)
        assert res["lm"] != 0.0
    print(f"kind {kind} seed {seed} lm {lm_seed}: margin {margin:.3e}, bar {bar:.3e}, largest term {peak:.1f}, {len(res['ids'])} tokens, "
          f"committed bonus {res['score'] - res['logp'] - res['lm']:.1f}")
    assert ok and margin > bar >= HC.MARGIN
    assert len(res["ids"]) > 100 and res["score"] - res["logp"] > 100.0      # the sums the rebase is for did grow
    # one call, and a cutting across both rebase frames, give the same result with the same bookkeeping
    cut, rec = SB.stream(hd, encp.astype(np.float64), [SB.REBASE - 1, SB.REBASE, SB.REBASE + 1, 2 * SB.REBASE], SB.LONG_W, SB.LONG_S, phrases,
                         HC.BETA, None if lm_seed is None else SB.long_lm(seed, hd, encp, lm_seed)[1], rebase=SB.REBASE)
    _same(cut, res)
    assert rec["peak"] == peak
