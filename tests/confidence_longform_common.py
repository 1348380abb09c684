"""Helpers of tests/test_hip_confidence_longform.py: synthetic two-layer models, a synthetic recording as a WAV file, the window plan
of a file and the test's own stitched stream -- as tests/test_hip_longform_windows.py builds them (copied, so that file stays as it is)."""
import numpy as np
import torch

DEV = "cuda:0"


def model(name):
    import gigaam_amd
    from gigaam_amd import synth
    return gigaam_amd.model_from_checkpoint(synth.make_checkpoint(name, seed=1, n_layers=2), DEV)


def wav_file(tmp_path, seconds, seed):
    import wave
    from gigaam_amd import synth
    wav, _ = synth.synth_audio(1, seconds, seed=seed)
    pcm = (wav[0].numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16)
    p = str(tmp_path / f"clip{seed}.wav")
    with wave.open(p, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(16000)
        wf.writeframes(pcm.tobytes())
    return p


def plan_of(m, path, chunk_s, stride_s):
    from gigaam_amd.preprocess import load_audio
    from gigaam_amd.windows import plan_windows
    eng = m.head.engine
    audio = load_audio(path, 16000)
    frame = int(eng.cfg.hop_length) * int(eng.cfg.subsampling_factor)
    return audio, plan_windows(int(audio.shape[0]), frame, lambda n: eng.enc_frames(eng.feat_frames(n)), chunk_s, stride_s)


def stitched(m, audio, plan, batch):
    """The test's own stream: the windows in the same feeder batches through ``_encode`` and ``ctc_head``, stitched in numpy."""
    from gigaam_amd.feeder import BatchFeeder
    eng = m.head.engine
    parts, k = [], 0
    with torch.inference_mode():
        feeder = BatchFeeder([audio[w.start:w.stop] for w in plan.windows], batch, torch.device(DEV))
        for wav, lens in feeder:
            enc, elen = m._encode(wav, lens, feeder.host_lengths)
            lp, elen = eng.ctc_head(enc).cpu().numpy(), elen.cpu().tolist()
            for b in range(lp.shape[0]):
                w = plan.windows[k]
                assert w.hi <= elen[b] == eng.enc_frames(eng.feat_frames(w.stop - w.start))
                parts.append(lp[b, w.lo:w.hi].copy())
                k += 1
    stream = np.concatenate(parts)
    assert k == len(plan.windows) and stream.shape[0] == plan.t_total
    return stream


def stream_frames(plan, wins, local):
    """(window, local frame) of each token -> its frame in the stitched stream."""
    return [plan.windows[k].dst + j - plan.windows[k].lo for k, j in zip(wins, local)]


def as_tuples(words):
    return [(w.text, w.start, w.end) for w in words]


def region_batch(m, path, **kw):
    """The chunks of the speech-region routes as ONE collated batch: (wav [B, L] zero padded, lengths [B] on the host, boundaries)."""
    from gigaam_amd.feeder import collate
    from gigaam_amd.vad_utils import segment_audio_file
    segments, boundaries = segment_audio_file(path, 16000, device=torch.device(DEV), **kw)
    wav, lens = collate([s.cpu() for s in segments])
    return wav, lens, boundaries
