"""Files at other rates and in other sample formats through the public surface, under the native audio backend: a WAV goes through
read_wav -> gam_op_resample -> the model, with the small synthetic v2_ctc model of __graft_entry__.smoke."""
import struct

import numpy as np
import pytest
import torch

import gigaam_amd
import resample_ref as R
from gigaam_amd import synth
from test_hip_resample import K_RS, bar_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def riff(tag, channels, rate, bits, payload):
    block = channels * bits // 8
    fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * block, block, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(payload)) + bytes(payload)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def alaw_encode(x):
    """fp32 in [-1, 1) -> the nearest A-law code, by search over the 256 decoded values (a test needs no fast encoder)."""
    levels = R.alaw_decode(np.arange(256, dtype=np.uint8)).astype(np.float32) / 32768.0
    order = np.argsort(levels)
    idx = np.clip(np.searchsorted(levels[order], x), 1, 255)
    lo, hi = levels[order][idx - 1], levels[order][idx]
    return order[np.where(x - lo < hi - x, idx - 1, idx)].astype(np.uint8)


@pytest.fixture(scope="module")
def model():
    return gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=1, n_layers=2), DEV)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (path, rate, format, channels, raw bytes): 3 s of synthetic speech-like audio at 8 k (stereo A-law, the channels two
    different utterances), 44.1 k (mono PCM24) and 48 k (float32)."""
    d = tmp_path_factory.mktemp("audio")
    out = {}
    two, _ = synth.synth_audio(2, 3.0, seed=5, sample_rate=8000)
    raw = alaw_encode(two.numpy().T.reshape(-1).clip(-1, 1))
    out["alaw8k"] = (8000, "alaw", 2, raw, riff(6, 2, 8000, 8, raw))
    one, _ = synth.synth_audio(1, 3.0, seed=6, sample_rate=44100)
    v = np.round(one[0].numpy().clip(-1, 1).astype(np.float64) * 8388607).astype(np.int64) & 0xFFFFFF
    raw = np.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], 1).astype(np.uint8).reshape(-1)
    out["pcm24_44k"] = (44100, "i24", 1, raw, riff(1, 1, 44100, 24, raw))
    one, _ = synth.synth_audio(1, 3.0, seed=7, sample_rate=48000)
    raw = one[0].numpy().astype("<f4").view(np.uint8)
    out["f32_48k"] = (48000, "f32", 1, raw, riff(3, 1, 48000, 32, raw))
    res = {}
    for name, (rate, fmt, channels, raw, blob) in out.items():
        p = str(d / (name + ".wav"))
        with open(p, "wb") as fh:
            fh.write(blob)
        res[name] = (p, rate, fmt, channels, raw)
    return res


@pytest.fixture()
def native_backend():
    prev = gigaam_amd.set_audio_backend("native")
    yield
    gigaam_amd.set_audio_backend(prev)


@pytest.mark.parametrize("name", ["alaw8k", "pcm24_44k", "f32_48k"])
def test_file_and_tensor_routes_agree(model, files, native_backend, name):
    path, rate, fmt, channels, raw = files[name]
    wav = gigaam_amd.decode_audio(path, device=DEV)
    n_out = R.out_len(rate, 16000, raw.size // (channels * R.BYTES[fmt]))
    assert wav.shape == (n_out,) and wav.dtype == torch.float32 and wav.device.type == "cuda"
    assert bar_ratio(wav.cpu().numpy(), R.decode_ref(raw, fmt, channels), (rate, 16000), "file_" + name) <= K_RS
    assert torch.equal(gigaam_amd.load_audio(path), wav.cpu())                     # load_audio: the same samples, on the CPU
    text = model.transcribe(path).text
    assert text == model.transcribe_batch(wav[None], torch.tensor([n_out], device=DEV))[0][0]
    assert isinstance(text, str)


def test_longform_on_an_8k_file(model, files, native_backend):
    res = model.transcribe_longform(files["alaw8k"][0], speech_regions=[(0.0, 3.0)])
    assert len(res.segments) == 1 and isinstance(res.text, str)


def test_resample_rows_equal_decode_audio_per_channel(files):
    path, rate, fmt, channels, raw = files["alaw8k"]
    x = R.decode_samples(raw, fmt).reshape(-1, channels)
    L = x.shape[0]
    lens = [L, L - 1234]
    batch = torch.from_numpy(np.ascontiguousarray(x.T)).to(DEV)
    out, out_len = gigaam_amd.resample(batch, 8000, 16000, lengths=torch.tensor(lens))
    assert out_len.tolist() == [2 * n for n in lens] and out.shape == (2, 2 * L)
    c0 = gigaam_amd.decode_audio(path, channel=0, device=DEV)
    c1 = gigaam_amd.decode_audio(path, channel=1, device=DEV)
    assert torch.equal(out[0], c0)
    assert not torch.equal(c0, c1) and float((c0 - c1).abs().max()) > 1e-2     # the channels hold different utterances
    assert bool((out[1, 2 * lens[1]:] == 0).all())
    # the shortened row: the same as its own samples alone; identical to the whole file's channel well before the cut
    alone = gigaam_amd.resample(batch[1, :lens[1]], 8000, 16000)
    assert torch.equal(out[1, :2 * lens[1]], alone) and torch.equal(alone[:2 * lens[1] - 64], c1[:2 * lens[1] - 64])
    mean = gigaam_amd.decode_audio(path, device=DEV)
    assert bar_ratio(mean.cpu().numpy(), R.downmix(x), (8000, 16000), "file_alaw8k_mean") <= K_RS
