"""GPU: the detector-free longform paths -- ``transcribe_longform(vad="windows")`` and ``align_longform(vad="windows")`` -- on synthetic
2-layer CTC models.  The expectation is composed here from public pieces: the planner's windows go through ``BatchFeeder``, ``_encode``
and ``ctc_head`` in the same batches, are stitched in numpy by the planner's table, decoded by the numpy greedy reference and turned
into words and segments by the documented rules.  The same batches give the same log-prob bits, so every comparison is exact."""
import math

import numpy as np
import pytest
import torch

from ctc_greedy_long_ref import greedy_ref
from test_hip_ctc_align import _wav_file

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _model(name):
    import gigaam_amd
    from gigaam_amd import synth
    return gigaam_amd.model_from_checkpoint(synth.make_checkpoint(name, seed=1, n_layers=2), DEV)


def _plan(model, path, chunk_s, stride_s):
    from gigaam_amd.preprocess import load_audio
    from gigaam_amd.windows import plan_windows
    eng = model.head.engine
    audio = load_audio(path, 16000)
    frame = int(eng.cfg.hop_length) * int(eng.cfg.subsampling_factor)
    return audio, plan_windows(int(audio.shape[0]), frame, lambda n: eng.enc_frames(eng.feat_frames(n)), chunk_s, stride_s)


def _stitched(model, audio, plan, batch):
    """The test's own stream: the windows in the same feeder batches through ``_encode`` and ``ctc_head``, stitched in numpy."""
    from gigaam_amd.feeder import BatchFeeder
    eng = model.head.engine
    parts, k = [], 0
    with torch.inference_mode():
        feeder = BatchFeeder([audio[w.start:w.stop] for w in plan.windows], batch, torch.device(DEV))
        for wav, lens in feeder:
            enc, elen = model._encode(wav, lens, feeder.host_lengths)
            lp, elen = eng.ctc_head(enc).cpu().numpy(), elen.cpu().tolist()
            for b in range(lp.shape[0]):
                w = plan.windows[k]
                assert w.hi <= elen[b] == eng.enc_frames(eng.feat_frames(w.stop - w.start))     # the host formula is the device's
                parts.append(lp[b, w.lo:w.hi].copy())
                k += 1
    stream = np.concatenate(parts)
    assert k == len(plan.windows) and stream.shape[0] == plan.t_total
    return stream


def _words(model, plan, ids, frames):
    """``frames_to_words``' rule on file times: start at the first token's frame time, end one frame shift behind the last token's
    frame time, each in the window the frame was kept from, rounded to 3 decimals."""
    from gigaam_amd.timestamps_utils import word_token_groups
    tok = model.decoding.tokenizer
    wins, local, times = plan.locate(frames)
    out = []
    for g in word_token_groups(tok, ids):
        a, b = g[0], g[-1]
        wb = plan.windows[wins[b]]
        text = "".join(tok.id_to_str(ids[i]) for i in g).replace("▁", "").strip()
        out.append((text, round(times[a], 3), round(wb.start_s + (local[b] + 1) * wb.shift, 3)))
    return out


def _segments(words, pause_s=1.0, max_segment_s=22.0):
    segs = []
    for w in words:
        if segs and w[1] - segs[-1][-1][2] < pause_s and w[2] - segs[-1][0][1] <= max_segment_s:
            segs[-1].append(w)
        else:
            segs.append([w])
    return [(" ".join(w[0] for w in s), s[0][1], s[-1][2], s) for s in segs]


def _as_tuples(words):
    return [(w.text, w.start, w.end) for w in words]


def _compare_transcription(model, path, chunk_s, stride_s, batch, pause_s):
    audio, plan = _plan(model, path, chunk_s, stride_s)
    stream = _stitched(model, audio, plan, batch)
    ids, frames = greedy_ref(stream)
    assert len(ids) > 20
    want_words = _words(model, plan, ids, frames)
    want = _segments(want_words, pause_s=pause_s)
    kw = dict(vad="windows", chunk_length_s=chunk_s, stride_length_s=stride_s, fr_batch_size=batch, pause_s=pause_s)
    res = model.transcribe_longform(path, word_timestamps=True, **kw)
    assert _as_tuples(res.words) == want_words
    assert [(s.text, s.start, s.end, _as_tuples(s.words)) for s in res.segments] == want
    plain = model.transcribe_longform(path, **kw)
    assert [(s.text, s.start, s.end, s.words) for s in plain.segments] == [(t, a, b, None) for t, a, b, _ in want]
    return audio, plan, stream, ids, frames, want


@pytest.fixture(scope="module")
def v2():
    return _model("v2_ctc")


@pytest.fixture(scope="module")
def long_case(v2, tmp_path_factory):
    """(b): 23.3 s, 6 s chunks with 1 s strides, feeder batches of 2 -- several windows, several batches; shared with (d)."""
    path = _wav_file(tmp_path_factory.mktemp("windows"), 23.3, 41)
    # a pause threshold of 0.3 s: the synthetic model's word gaps then give more than one segment
    audio, plan, stream, ids, frames, want = _compare_transcription(v2, path, 6.0, 1.0, 2, 0.3)
    assert len(plan.windows) >= 5 and (plan.chunk_frames, plan.stride_frames) == (150, 25)
    return path, plan, stream, ids, frames, want


def test_a_short_file_gives_the_words_of_transcribe(v2, tmp_path):
    path = _wav_file(tmp_path, 7.0, 17)
    want = v2.transcribe(path, word_timestamps=True)
    res = v2.transcribe_longform(path, word_timestamps=True, vad="windows")
    assert len(want.words) >= 2
    assert _as_tuples(res.words) == [(w.text, round(w.start, 3), round(w.end, 3)) for w in want.words]
    assert " ".join(w.text for w in res.words) == " ".join(want.text.split())


def test_several_windows_in_several_batches_match_the_composed_expectation(long_case):
    path, plan, stream, ids, frames, want = long_case
    assert len(want) >= 1
    # the seams are really crossed: tokens were kept from every window
    wins, _, times = plan.locate(frames)
    assert set(wins) == set(range(len(plan.windows)))
    assert all(b > a for a, b in zip(times, times[1:]))


def test_the_conv1d_uncentred_e2e_model(tmp_path):
    model = _model("v3_e2e_ctc")
    assert model.head.engine.cfg.num_classes == 257 and not model.head.engine.cfg.center
    path = _wav_file(tmp_path, 12.0, 43)
    _, plan, _, _, _, _ = _compare_transcription(model, path, 6.0, 1.0, 2, 0.3)
    assert len(plan.windows) >= 2


def test_windowed_alignment_of_the_greedy_ids(v2, long_case):
    path, plan, stream, ids, frames, _ = long_case
    eng = v2.head.engine
    kw = dict(vad="windows", chunk_length_s=6.0, stride_length_s=1.0, fr_batch_size=2)
    ref = eng.op_ctc_align_long(torch.from_numpy(stream), ids).host()
    assert ref["status"] == 1
    res = v2.align_longform(path, ids, **kw)
    assert res.feasible and res.token_ids == ids
    assert res.score == ref["score"] and res.log_likelihood == ref["loglik"]
    want_seg, want_local, want_times = plan.locate(ref["tok_first"].tolist())
    assert (res.token_segments, res.token_frames, res.token_times) == (want_seg, want_local, want_times)
    for k, j, t in zip(res.token_segments, res.token_frames, res.token_times):
        w = plan.windows[k]
        assert w.lo <= j < w.hi and t == w.start_s + j * w.shift
    # one Segment per window over its kept frames: they tile the file, and hold the words that start there
    segs = res.segments
    assert len(segs) == len(plan.windows) and segs[0].start == 0.0 and segs[-1].end == pytest.approx(23.3, abs=1e-3)
    assert all(a.end == b.start for a, b in zip(segs, segs[1:])) and all(s.end > s.start for s in segs)
    assert [w for s in segs for w in s.words] == res.words
    assert all(s.start - 1e-3 <= w.start < s.end + 1e-3 for s in segs for w in s.words)
    assert _as_tuples(res.words) == _words(v2, plan, ids, want_local_to_global(plan, want_seg, want_local))
    # a partial transcript: the middle third of the ids behind one wildcard comes back as one gap
    a, b = len(ids) // 3, 2 * len(ids) // 3
    wid = v2.wildcard_id
    part = ids[:a] + [wid] + ids[b:]
    star = eng.ctc_star_row(torch.from_numpy(stream).to(DEV), None, math.log(2))
    ref = eng.op_ctc_align_long(torch.from_numpy(stream), part, star=star).host()
    res = v2.align_longform(path, part, wildcard="*", **kw)
    assert res.token_ids == part and res.score == ref["score"] and res.log_likelihood == ref["loglik"]
    assert res.token_times == plan.locate(ref["tok_first"].tolist())[2]
    assert len(res.gaps) == 1
    gap = res.gaps[0]
    k0, j0, t0 = (x[0] for x in plan.locate([int(ref["tok_first"][a])]))
    k1, j1, _ = (x[0] for x in plan.locate([int(ref["tok_last"][a])]))
    w1 = plan.windows[k1]
    assert (gap.segment, gap.start_frame, gap.end_segment, gap.end_frame) == (k0, j0, k1, j1)
    assert (gap.start, gap.end) == (round(t0, 3), round(w1.start_s + (j1 + 1) * w1.shift, 3)) and gap.end > gap.start


def want_local_to_global(plan, wins, local):
    return [plan.windows[k].dst + j - plan.windows[k].lo for k, j in zip(wins, local)]


def test_what_the_windowed_route_refuses(v2, tmp_path):
    path = _wav_file(tmp_path, 3.0, 5)
    for kw in (dict(beam_size=4), dict(hotwords=["да"]), dict(lm="missing.arpa")):
        with pytest.raises(ValueError, match="8192"):
            v2.transcribe_longform(path, vad="windows", **kw)
    with pytest.raises(ValueError, match="speech_regions"):
        v2.transcribe_longform(path, vad="windows", speech_regions=[(0.0, 1.0)])
    with pytest.raises(ValueError, match="speech_regions"):
        v2.align_longform(path, "а", vad="windows", speech_regions=[(0.0, 1.0)])
    with pytest.raises(ValueError):
        v2.transcribe_longform(path, vad="windows", chunk_length_s=30.0)
    with pytest.raises(ValueError):
        v2.transcribe_longform(path, vad="windows", chunk_length_s=6.0, stride_length_s=3.0)
    rnnt = _model("v2_rnnt")
    with pytest.raises(TypeError, match="windowed longform needs a CTC head"):
        rnnt.transcribe_longform(path, vad="windows")
    with pytest.raises(TypeError, match="windowed longform needs a CTC head"):
        rnnt.align_longform(path, [1, 2], vad="windows")
