"""GPU: the detector-free longform route of an RNN-T model in beam mode -- ``transcribe_longform(vad="windows",
stream_decode="beam")`` -- on ``beam_common.small_rnnt_model`` (a synthetic 2-layer ``v2_rnnt``, blank bias 12).  The expectation is
composed from public pieces: the planner's windows go through ``BatchFeeder``, ``_encode`` and ``rnnt_encp``, their kept rows are
stitched in numpy by the planner's table, ONE BEGIN | END call of ``op_rnnt_beam_stream`` searches that stream, and the words and
segments follow the documented rules.  A file of one window with fewer frames than a rebase period is ``transcribe``'s own result."""
import numpy as np
import pytest
import torch

import beam_common as BC
from test_hip_ctc_align import _wav_file
from test_hip_longform_rnnt_windows import _stitched_encp
from test_hip_longform_windows import _as_tuples, _plan, _segments, _words

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KW = dict(vad="windows", stream_decode="beam", pause_s=0.3)


@pytest.fixture(scope="module")
def rnnt():
    return BC.small_rnnt_model()[0]


def _op_stream(model, rows, W):
    """ids, frames of the stitched rows by one call of the op."""
    from gigaam_amd.engine import BeamStreamDecoded
    eng = model.head.engine
    S, n = int(model.decoding.max_symbols), int(rows.shape[0])
    nbytes = int(eng.lib.gam_rnnt_beam_stream_bytes(eng._h, W, S, n))
    state = torch.zeros((nbytes // 4,), dtype=torch.int32, device=DEV)
    out = BeamStreamDecoded.empty(torch.device(DEV), n * S)
    with torch.cuda.device(torch.device(DEV)):
        eng.op_rnnt_beam_stream(torch.from_numpy(rows).to(DEV), 0, 3, W, S, state, nbytes, out)
        h = eng._finish(out, False).host()
    return h["ids"].tolist(), h["frames"].tolist()


def _result(res):
    return [(s.text, s.start, s.end, _as_tuples(s.words)) for s in res.segments]


def test_a_short_file_gives_the_words_of_transcribe(rnnt, tmp_path):
    from gigaam_amd.engine import HipEngine
    path = _wav_file(tmp_path, 7.0, 17)
    rnnt.set_decoding(beam_size=4)
    try:
        want = rnnt.transcribe(path, word_timestamps=True)
        res = rnnt.transcribe_longform(path, word_timestamps=True, vad="windows", stream_decode="beam")
        audio, plan = _plan(rnnt, path, 20.0, None)
        assert len(plan.windows) == 1 and plan.t_total < HipEngine.RNNT_BEAM_STREAM_REBASE
        assert len(want.words) >= 1 and len(want.text) > 20
        assert _as_tuples(res.words) == [(w.text, round(w.start, 3), round(w.end, 3)) for w in want.words]
        assert " ".join(w.text for w in res.words) == " ".join(want.text.split())
        # the ids and frames: ``transcribe`` returns none, so its own decode (``decode_beam``: the batch kernel) of the same audio
        from gigaam_amd.feeder import BatchFeeder
        ids, frames = _op_stream(rnnt, _stitched_encp(rnnt, audio, plan, 1), 4)
        with torch.inference_mode():
            feeder = BatchFeeder([audio], 1, torch.device(DEV))
            for wav, lens in feeder:
                enc, elen = rnnt._encode(wav, lens, feeder.host_lengths)
                (text, bids, bframes, _, _), = rnnt.decoding.decode_beam(rnnt.head, enc, elen)
        assert (ids, frames) == (list(bids), list(bframes)) and len(ids) > 20
        assert text.strip() == want.text.strip()
    finally:
        rnnt.set_decoding()


def test_three_windows_give_one_result_however_they_are_batched(rnnt, tmp_path, monkeypatch):
    from gigaam_amd.engine import HipEngine
    path = _wav_file(tmp_path, 45.0, 41)
    greedy_before = _result(rnnt.transcribe_longform(path, word_timestamps=True, vad="windows", stream_decode=True, pause_s=0.3))
    rnnt.set_decoding(beam_size=4)
    try:
        audio, plan = _plan(rnnt, path, 20.0, None)
        assert len(plan.windows) == 3 and plan.t_total > 4 * HipEngine.RNNT_BEAM_STREAM_REBASE
        ids, frames = _op_stream(rnnt, _stitched_encp(rnnt, audio, plan, 16), 4)
        print(f"RNN-T beam windows: {len(ids)} tokens over {plan.t_total} frames, {len(plan.windows)} windows")
        assert len(ids) > 20 and set(plan.locate(frames)[0]) == {0, 1, 2}
        want_words = _words(rnnt, plan, ids, frames)
        want = _segments(want_words, pause_s=KW["pause_s"])
        default = _result(rnnt.transcribe_longform(path, word_timestamps=True, **KW))
        assert default == want
        assert _result(rnnt.transcribe_longform(path, word_timestamps=True, fr_batch_size=1, **KW)) == want
        assert _result(rnnt.transcribe_longform(path, word_timestamps=True, fr_batch_size=16, **KW)) == want
        monkeypatch.setenv("GAM_RNNT_STREAM_OVERLAP", "0")
        assert _result(rnnt.transcribe_longform(path, word_timestamps=True, **KW)) == want
        monkeypatch.delenv("GAM_RNNT_STREAM_OVERLAP")
        plain = rnnt.transcribe_longform(path, **KW)
        assert [(s.text, s.start, s.end, s.words) for s in plain.segments] == [(t, a, b, None) for t, a, b, _ in want]
        # hotwords through set_decoding: phrases of the plain result, boosted -- the search with them is the op's with them
        tok = rnnt.decoding.tokenizer
        text = tok.decode(ids).replace(" ", "")
        phrases = [text[10:13], text[40:42], text[-9:-6]]
        rnnt.set_decoding(beam_size=4, hotwords=phrases, hotword_boost=1.5)
        boosted = _result(rnnt.transcribe_longform(path, word_timestamps=True, **KW))
        hids, hframes = _op_stream(rnnt, _stitched_encp(rnnt, audio, plan, 16), 4)      # (the engine holds the set the route uploaded)
        assert boosted == _segments(_words(rnnt, plan, hids, hframes), pause_s=KW["pause_s"])
        # set_decoding() restores greedy, and stream_decode=True gives what it gave
        rnnt.set_decoding()
        assert _result(rnnt.transcribe_longform(path, word_timestamps=True, vad="windows", stream_decode=True, pause_s=0.3)) == greedy_before
        with pytest.raises(ValueError, match="set_decoding"):
            rnnt.transcribe_longform(path, **KW)
    finally:
        rnnt.set_decoding()
        rnnt.head.engine.set_hotwords([])
        rnnt.head.engine.set_lm(None)
