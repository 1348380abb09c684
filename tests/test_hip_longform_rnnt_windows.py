"""GPU: the detector-free longform route of the RNN-T heads -- ``transcribe_longform(vad="windows", stream_decode=True)`` -- on a
synthetic 2-layer ``v2_rnnt``.  The expectation is composed here from public pieces: the planner's windows go through ``BatchFeeder``,
``_encode`` and ``rnnt_encp`` in the same batches, their kept rows are stitched in numpy by the planner's table, ``op_rnnt_greedy``
decodes that stream as ONE utterance at cluster size 0 (the one-workgroup arithmetic, which the resumable kernel shares), and the
words and segments follow the documented rules.  The same batches give the same encp bits, so every comparison is exact.

The checkpoint is ``beam_common.small_rnnt_model``'s (seed 1, blank bias 12, the one the other RNN-T model tests use): its stream of
583 frames emits 340 tokens (asserted: more than 20), several in many a frame.  This synthetic head never emits the space, so the
transcript is ONE word from the first token's frame to the last token's: the word and segment rules are exercised on several words in
tests/test_rnnt_stream_host.py, and here every token still decides the compared text."""
import numpy as np
import pytest
import torch

from test_hip_ctc_align import _wav_file
from test_hip_longform_windows import _as_tuples, _plan, _segments, _words

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KW = dict(vad="windows", stream_decode=True, chunk_length_s=6.0, stride_length_s=1.0, fr_batch_size=2, pause_s=0.3)


@pytest.fixture(scope="module")
def rnnt():
    import gigaam_amd
    from gigaam_amd import synth
    return gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_rnnt", seed=1, n_layers=2, rnnt_blank_bias=12.0), DEV)


@pytest.fixture
def cluster0(rnnt):
    eng = rnnt.head.engine
    before = getattr(eng, "_rnnt_cluster_user", -1)
    eng.set_rnnt_cluster(0)
    yield eng
    eng.set_rnnt_cluster(before)


def _stitched_encp(model, audio, plan, batch):
    """The test's own stream: the windows in the same feeder batches through ``_encode`` and ``rnnt_encp``, stitched in numpy."""
    from gigaam_amd.feeder import BatchFeeder
    eng = model.head.engine
    parts, k = [], 0
    with torch.inference_mode():
        feeder = BatchFeeder([audio[w.start:w.stop] for w in plan.windows], batch, torch.device(DEV))
        for wav, lens in feeder:
            enc, elen = model._encode(wav, lens, feeder.host_lengths)
            rows, elen = eng.rnnt_encp(enc).cpu().numpy(), elen.cpu().tolist()
            for b in range(rows.shape[0]):
                w = plan.windows[k]
                assert w.hi <= elen[b] == eng.enc_frames(eng.feat_frames(w.stop - w.start))
                parts.append(rows[b, w.lo:w.hi].copy())
                k += 1
    stream = np.concatenate(parts)
    assert k == len(plan.windows) and stream.shape == (plan.t_total, int(eng.cfg.joint_hidden))
    return stream


@pytest.fixture(scope="module")
def long_case(rnnt, tmp_path_factory):
    """23.3 s, 6 s chunks with 1 s strides, feeder batches of 2; the stream decoded by ``op_rnnt_greedy`` at cluster size 0."""
    from gigaam_amd.engine import HipEngine
    path = _wav_file(tmp_path_factory.mktemp("rnnt_windows"), 23.3, 41)
    eng = rnnt.head.engine
    before = getattr(eng, "_rnnt_cluster_user", -1)
    eng.set_rnnt_cluster(0)
    try:
        audio, plan = _plan(rnnt, path, 6.0, 1.0)
        stream = _stitched_encp(rnnt, audio, plan, 2)
        dec = eng.op_rnnt_greedy(torch.from_numpy(stream)[None], torch.tensor([plan.t_total], dtype=torch.int32),
                                 int(rnnt.decoding.max_symbols))
        assert eng.rnnt_last_decode() == (0, -1, False)
        (ids, frames), = HipEngine.collect(dec)[0]
    finally:
        eng.set_rnnt_cluster(before)
    assert len(plan.windows) >= 5 and (plan.chunk_frames, plan.stride_frames) == (150, 25)
    print(f"RNN-T windows: {len(ids)} tokens over {plan.t_total} frames, {len(plan.windows)} windows")
    return path, plan, ids, frames


def test_the_stream_emits_and_crosses_every_seam(long_case):
    _, plan, ids, frames = long_case
    assert len(ids) > 20
    wins, _, times = plan.locate(frames)
    assert set(wins) == set(range(len(plan.windows)))
    assert all(b >= a for a, b in zip(times, times[1:]))        # (a frame may carry several tokens)


@pytest.mark.parametrize("overlap", ["1", "0"])
def test_several_windows_in_several_batches_match_the_composed_expectation(rnnt, long_case, overlap, monkeypatch):
    path, plan, ids, frames = long_case
    monkeypatch.setenv("GAM_RNNT_STREAM_OVERLAP", overlap)
    want_words = _words(rnnt, plan, ids, frames)
    want = _segments(want_words, pause_s=KW["pause_s"])
    assert len(want_words) >= 1 and sum(len(w[0]) for w in want_words) > 20
    res = rnnt.transcribe_longform(path, word_timestamps=True, **KW)
    assert _as_tuples(res.words) == want_words
    assert [(s.text, s.start, s.end, _as_tuples(s.words)) for s in res.segments] == want
    plain = rnnt.transcribe_longform(path, **KW)
    assert [(s.text, s.start, s.end, s.words) for s in plain.segments] == [(t, a, b, None) for t, a, b, _ in want]


def test_a_short_file_gives_the_words_of_transcribe(rnnt, cluster0, tmp_path):
    path = _wav_file(tmp_path, 7.0, 17)
    want = rnnt.transcribe(path, word_timestamps=True)
    assert cluster0.rnnt_last_decode() == (0, -1, False)
    res = rnnt.transcribe_longform(path, word_timestamps=True, vad="windows", stream_decode=True)
    assert len(want.words) >= 1 and len(want.text) > 20
    assert _as_tuples(res.words) == [(w.text, round(w.start, 3), round(w.end, 3)) for w in want.words]
    assert " ".join(w.text for w in res.words) == " ".join(want.text.split())
