"""Host: the resumable RNN-T greedy decode without a GPU -- the float64 twin of tests/rnnt_stream_ref.py against
``R.greedy_trace`` at every cut (the record suffices; no symbol count has to be carried), the keyword errors of
``transcribe_longform(stream_decode=True)``, the word rule where one frame carries several tokens, and the two headers' flags."""
import os
import re

import pytest

import rnnt_beam_ref as R
import rnnt_cluster_cases as K
import rnnt_stream_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_MARGIN = 1.2e-2      # the smallest margin of the cluster matrix's heads (tests/rnnt_cluster_cases.py HEADS): the L = 2 case must not be closer


@pytest.mark.parametrize("name", ["C", "D"])
def test_every_cut_of_every_utterance_equals_the_uncut_decode(name):
    """The stream cut in two at EVERY position p in [0, T] (p = 0 and p = T: an empty call) carries only the record's fields and
    gives ``R.greedy_trace``'s ids and frames; the count after the first call is the reference's prefix count."""
    _, sd, encoded, lengths = K.inputs(name)
    head = R.head_from_state_dict(sd, 1)
    ref = K.reference(name)
    emitted_at_cut = capped_before_cut = 0
    for b, T in enumerate(lengths):
        want = ref[b]
        for p in range(T + 1):
            got = SR.decode_cut(head, encoded[b], T, K.MAX_SYMBOLS, [p])
            assert (got["ids"], got["frames"]) == (want["ids"], want["frames"]), (name, b, p)
            assert got["counts"] == [sum(want["per_frame"][:p]), len(want["ids"])], (name, b, p)
            emitted_at_cut += p < T and want["per_frame"][p] > 0
            capped_before_cut += p > 0 and want["per_frame"][p - 1] == K.MAX_SYMBOLS
    # the cuts that matter were among them: before an emitting frame, and behind a frame that stopped at max_symbols
    assert emitted_at_cut > 0 and capped_before_cut > 0


def test_many_cuts_and_empty_calls():
    _, sd, encoded, lengths = K.inputs("C")
    head = R.head_from_state_dict(sd, 1)
    want = K.reference("C")[0]
    T = lengths[0]
    for cuts in (list(range(1, T)), [0, 0, 20, 20, 20, T, T], [15, 16, 17, 32, 33]):
        got = SR.decode_cut(head, encoded[0], T, K.MAX_SYMBOLS, cuts)
        assert (got["ids"], got["frames"]) == (want["ids"], want["frames"]), cuts
        assert got["counts"] == [sum(want["per_frame"][:p]) for p in cuts + [T]]


def test_what_the_twin_refuses():
    _, sd, encoded, lengths = K.inputs("D")
    head = R.head_from_state_dict(sd, 1)
    encp = R.encoder_projection(head, encoded[0])
    S, cap = K.MAX_SYMBOLS, 60 * K.MAX_SYMBOLS
    ids, frames, rec = [0] * cap, [0] * cap, SR.new_record()
    assert SR.call(head, rec, encp[:5], 0, 0, S, ids, frames, cap) == 0 and rec == SR.new_record()       # not begun
    assert SR.call(head, rec, encp[:5], 7, SR.BEGIN, S, ids, frames, cap) == 1 and rec["next"] == 12
    before = dict(rec)
    assert SR.call(head, rec, encp[5:9], 11, 0, S, ids, frames, cap) == 0                               # a frame given twice
    assert SR.call(head, rec, encp[5:9], 13, 0, S, ids, frames, cap) == 0                               # a frame skipped
    assert SR.call(head, rec, encp[5:9], 12, 0, S + 1, ids, frames, cap) == 0                           # max_symbols changed
    assert SR.call(head, rec, encp[5:9], 12, 0, S, ids, frames, rec["count"] + 4 * S - 1) == 0          # could overflow cap
    assert rec == before
    assert SR.call(head, rec, encp[5:9], 12, SR.END, S, ids, frames, rec["count"] + 4 * S) == 1
    assert SR.call(head, rec, None, 16, 0, S, ids, frames, cap) == 0                                    # ended


def test_head_c_with_two_layers_is_decided_by_a_wide_margin():
    """The L = 2 case of the GPU test: its margins by the float64 reference allow exact ids, it emits, and it caps frames."""
    _, _, _, lengths, ref = SR.l2_case()
    for b, r in enumerate(ref[:5]):
        assert r["margin"] >= MIN_MARGIN, (b, r["margin"])
    assert sum(len(r["ids"]) for r in ref) > 20 and any(n == K.MAX_SYMBOLS for n in ref[0]["per_frame"])
    print("head C, L = 2: smallest margin", min(r["margin"] for r in ref[:5]))


def test_the_kernel_header_agrees_with_the_public_header():
    src = open(os.path.join(ROOT, "gigaam_amd", "csrc", "gam_rnnt_stream.h")).read()
    header = open(os.path.join(ROOT, "include", "gigaam_hip.h")).read()
    from gigaam_amd.engine import RnntGreedyStream
    for f, v in (("BEGIN", SR.BEGIN), ("END", SR.END)):
        assert int(re.search(r"#define GAM_RNNT_F_" + f + r"\s+(\d+)", src).group(1)) == v
        assert int(re.search(r"#define GAM_RNNT_STREAM_" + f + r"\s+(\d+)", header).group(1)) == v
        assert getattr(RnntGreedyStream, f) == v
    assert int(re.search(r"#define GAM_ABI_VERSION\s+(\d+)", header).group(1)) == 1


def test_stream_decode_keyword_errors_need_no_gpu():
    import gigaam_amd
    from gigaam_amd import synth
    ctc = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=1, n_layers=1), "cpu")
    rnnt = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_rnnt", seed=1, n_layers=1), "cpu")
    path = "no-such-file.wav"       # (every error below is raised before the file is opened)
    # without vad="windows"
    for kw in (dict(), dict(speech_regions=[(0.0, 1.0)]), dict(vad="energy")):
        with pytest.raises(ValueError, match='stream_decode=True decodes the stitched stream of vad="windows"'):
            rnnt.transcribe_longform(path, stream_decode=True, **kw)
    # a CTC head
    with pytest.raises(TypeError, match="stream_decode needs an RNN-T head"):
        ctc.transcribe_longform(path, vad="windows", stream_decode=True)
    # a beam decoding object selected by set_decoding
    rnnt.set_decoding(beam_size=4)
    with pytest.raises(ValueError, match="8192"):
        rnnt.transcribe_longform(path, vad="windows", stream_decode=True)
    rnnt.set_decoding(hotwords=["да"])
    with pytest.raises(ValueError, match="RNN-T beam kernel stops at 8192 frames"):
        rnnt.transcribe_longform(path, vad="windows", stream_decode=True)
    rnnt.set_decoding()
    # per-call beam options on an RNN-T model: the TypeError they always raise
    for kw in (dict(beam_size=4), dict(hotwords=["да"]), dict(lm="missing.arpa")):
        with pytest.raises(TypeError, match="beam search needs a CTC head"):
            rnnt.transcribe_longform(path, vad="windows", stream_decode=True, **kw)
        with pytest.raises(TypeError, match="beam search needs a CTC head"):
            rnnt.transcribe_longform(path, speech_regions=[(0.0, 1.0)], **kw)
    # both resumable decoders at once
    for model in (ctc, rnnt):
        with pytest.raises(ValueError, match="a call takes one of them"):
            model.transcribe_longform(path, vad="windows", stream_search=True, stream_decode=True, beam_size=4)
    # segmentation keywords beside vad="windows"
    for kw in (dict(speech_regions=[(0.0, 1.0)]), dict(max_duration=20.0)):
        with pytest.raises(ValueError, match='vad="windows" takes no segmentation keywords'):
            rnnt.transcribe_longform(path, vad="windows", stream_decode=True, **kw)
    # without stream_decode everything raises what it raised: the two pinned TypeErrors
    with pytest.raises(TypeError, match="windowed longform needs a CTC head"):
        rnnt.transcribe_longform(path, vad="windows")
    with pytest.raises(TypeError, match="windowed longform needs a CTC head"):
        rnnt.transcribe_longform(path, vad="windows", stream_search=True, beam_size=4)
    with pytest.raises(TypeError, match="windowed longform needs a CTC head"):
        rnnt.transcribe_longform(path, vad="windows", stream_decode=False)


def test_words_of_a_stream_whose_frame_holds_three_tokens():
    """``_windows_result`` on RNN-T ids / frames: a word starts at its first token's frame and ends one frame shift behind its last
    token's frame, each in the window it was kept from; the tokens a frame emitted beyond its first share that frame, so a word
    spelt inside ONE frame is one frame shift long, and a word that ends in a frame where the next begins overlaps nothing."""
    import gigaam_amd
    from gigaam_amd import synth
    from gigaam_amd.windows import plan_windows
    rnnt = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_rnnt", seed=1, n_layers=1), "cpu")
    tok = rnnt.decoding.tokenizer
    frame = 640                                            # 40 ms frames
    plan = plan_windows(10 * 16000, frame, lambda n: n // frame, 4.0, 1.0)      # windows of 100 frames, 25 dropped at inner edges
    assert len(plan.windows) >= 3 and plan.t_total == 250
    chars = {tok.id_to_str(i): i for i in range(len(synth.CHAR_VOCAB))}
    a, b, sp = chars["а"], chars["б"], chars[" "]
    # frame 10 holds three tokens ("аб" and the space), frames 80 / 81 (window 1) a word and its space, frame 140 (window 2) three
    # tokens that spell one word inside one frame
    ids = [a, b, sp, b, a, sp, a, a, b]
    frames = [10, 10, 10, 80, 80, 81, 140, 140, 140]
    res = rnnt._windows_result(plan, ids, frames, True, 1.0, 22.0)
    wins, local, times = plan.locate(frames)
    assert (wins[0], wins[3], wins[6]) == (0, 1, 2)
    sh = [plan.windows[k].shift for k in wins]
    want = [("аб", round(times[0], 3), round(plan.windows[0].start_s + (local[1] + 1) * sh[1], 3)),
            ("ба", round(times[3], 3), round(plan.windows[1].start_s + (local[4] + 1) * sh[4], 3)),
            ("ааб", round(times[6], 3), round(plan.windows[2].start_s + (local[8] + 1) * sh[8], 3))]
    assert [(w.text, w.start, w.end) for w in res.words] == want
    assert want[0][2] - want[0][1] == pytest.approx(0.04, abs=1e-3) and want[2][2] - want[2][1] == pytest.approx(0.04, abs=1e-3)
    # pauses of more than a second between the words: three segments
    assert [s.text for s in res.segments] == ["аб", "ба", "ааб"]
    plain = rnnt._windows_result(plan, ids, frames, False, 1.0, 22.0)
    assert [(s.text, s.start, s.end, s.words) for s in plain.segments] == [(t, s0, e0, None) for t, s0, e0 in want]
