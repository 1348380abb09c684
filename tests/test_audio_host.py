"""CPU: the audio-ingest contract without a GPU -- the fp64 helper (tests/resample_ref.py) against a second formulation, the host entries
gam_resample_plan / _table / _out_len against the helper, the RIFF/WAVE reader, the G.711 decoders, decode_audio's host path and the
backends of load_audio."""
import ctypes as C
import math
import os
import re
import shutil
import struct
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from common import ROOT

import gigaam_amd
import resample_ref as R
from gigaam_amd import _lib, audio
from gigaam_amd.preprocess import load_audio

# (rate_in, rate_out): (N, O, K)
PLANS = {(48000, 16000): (1, 3, 37), (8000, 16000): (2, 1, 13), (44100, 16000): (160, 441, 34), (24000, 16000): (2, 3, 19),
         (22050, 16000): (320, 441, 17), (96000, 16000): (1, 6, 73), (11025, 16000): (640, 441, 13), (32000, 16000): (1, 2, 25),
         (12000, 16000): (4, 3, 13), (16000, 8000): (1, 2, 25)}
HAVE_FFMPEG = shutil.which("ffmpeg") is not None


def torchaudio_formulation(x, orig, new, width_l=6, rolloff=0.99):
    """torchaudio.functional.resample (sinc_interp_hann) restated in fp64 torch: one kernel of 2 width + orig taps per output phase,
    the input padded by width on the left and width + orig on the right, a conv1d of stride orig."""
    g = math.gcd(orig, new)
    orig, new = orig // g, new // g
    base = min(orig, new) * rolloff
    width = math.ceil(width_l * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = (torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx) * base
    t = t.clamp(-width_l, width_l)
    window = torch.cos(t * math.pi / width_l / 2) ** 2
    t = t * math.pi
    kernels = torch.where(t == 0, torch.ones_like(t), t.sin() / torch.where(t == 0, torch.ones_like(t), t)) * window * (base / orig)
    n = x.shape[-1]
    y = F.conv1d(F.pad(x[None, None], (width, width + orig)), kernels, stride=orig)
    return y.transpose(1, 2).reshape(-1)[:-((-new * n) // orig)]


@pytest.mark.parametrize("rates", sorted(PLANS))
def test_helper_agrees_with_the_torchaudio_formulation(rates):
    for n in (1, 5, 1000):
        x = np.random.default_rng(n).standard_normal(n)
        want = torchaudio_formulation(torch.from_numpy(x), *rates).numpy()
        got = R.resample_ref(x, *rates)
        assert got.shape == want.shape == (R.out_len(*rates, n),)
        assert np.abs(got - want).max() <= 1e-12
    # the fp32 evaluation stays where fp32 arithmetic puts it
    x = np.random.default_rng(0).standard_normal(1000).astype(np.float32)
    assert np.abs(R.resample_ref32(x, *rates) - R.resample_ref(x, *rates)).max() < 5e-6


def _lib_plan(rates):
    lib = _lib.load_library()
    up, down, taps = C.c_int(), C.c_int(), C.c_int()
    rc = lib.gam_resample_plan(rates[0], rates[1], C.byref(up), C.byref(down), C.byref(taps))
    return rc, (up.value, down.value, taps.value)


@pytest.mark.parametrize("rates", sorted(PLANS) + [(1000, 1001), (16000, 16000), (384000, 8000)])
def test_plan_and_table_match_the_helper(rates):
    lib = _lib.load_library()
    rc, (N, O, K) = _lib_plan(rates)
    assert rc == 0
    if rates in PLANS:
        assert (N, O, K) == PLANS[rates]
    O_r, N_r, K_r, first_r = R.plan(*rates)
    assert (N, O, K) == (N_r, O_r, K_r)
    assert audio.resample_plan(*rates) == (N, O, K)
    coeff, first = np.empty(N * K, np.float32), np.empty(N, np.int32)
    assert lib.gam_resample_table(rates[0], rates[1], C.c_void_p(coeff.ctypes.data), C.c_void_p(first.ctypes.data)) == 0
    assert np.array_equal(first, first_r)
    want = R.table(*rates)[0].astype(np.float32).reshape(-1)
    assert np.all(np.abs(coeff - want) <= np.spacing(np.abs(want)))            # within one fp32 ulp
    assert np.abs(coeff.reshape(N, K).astype(np.float64).sum(1) - 1.0).max() < 1e-3
    for n in (0, 1, 2, 999, 2 ** 31 + 4099, 10 ** 12):
        assert lib.gam_resample_out_len(rates[0], rates[1], n) == R.out_len(*rates, n) == -((-N * n) // O)
    tile, form = C.c_int(), C.c_int()
    assert lib.gam_resample_tile(rates[0], rates[1], C.byref(tile), C.byref(form)) == 0
    assert tile.value >= 1 and form.value == (0 if N == 1 else 1 if tile.value >= N else 2)


def test_plan_errors():
    lib = _lib.load_library()
    for rates in ((0, 16000), (16000, 0), (384001, 16000), (16000, 384001), (-8000, 16000)):
        assert _lib_plan(rates)[0] == -1
        assert lib.gam_resample_out_len(rates[0], rates[1], 10) == -1
        with pytest.raises(ValueError):
            audio.resample_plan(*rates)
    assert _lib_plan((383999, 16000))[0] == -2                                   # N K = 16000 x 291 entries > 2**18
    with pytest.raises(ValueError, match="2\\*\\*18"):
        audio.resample_plan(383999, 16000)
    assert _lib_plan((384000, 16000))[0] == 0


# ------------------------------------------------------------------------------------------------------------ RIFF/WAVE
def riff(tag, channels, rate, bits, payload, extensible=False, before=b"", data_size=None, after=b""):
    block = channels * bits // 8
    fmt = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * block, block, bits)
    if extensible:
        fmt += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + bytes.fromhex("000000001000800000aa00389b71")
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + before
    body += b"data" + struct.pack("<I", len(payload) if data_size is None else data_size) + bytes(payload) + after
    return b"RIFF" + struct.pack("<I", len(body)) + body


def write(tmp_path, name, blob):
    p = str(tmp_path / name)
    with open(p, "wb") as fh:
        fh.write(blob)
    return p


WAVE_FMT = {1: "u8", 2: "i16", 3: "i24", 4: "i32"}


@pytest.mark.parametrize("width", [1, 2, 3, 4])
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_read_wav_reads_what_stdlib_wave_writes(tmp_path, width, channels):
    raw = R.random_raw(WAVE_FMT[width], 333, channels, seed=width * 10 + channels)
    p = str(tmp_path / "w.wav")
    with wave.open(p, "wb") as wf:
        wf.setnchannels(channels); wf.setsampwidth(width); wf.setframerate(22050); wf.writeframes(raw.tobytes())
    w = gigaam_amd.read_wav(p)
    assert (w.fmt, w.channels, w.rate, w.frames) == (WAVE_FMT[width], channels, 22050, 333)
    assert w.data.dtype == np.uint8 and np.array_equal(w.data, raw)


def test_read_wav_hand_built_files(tmp_path):
    f32 = R.random_raw("f32", 50, 2, 1)
    f64 = np.random.default_rng(2).standard_normal(40).astype("<f8").view(np.uint8)
    g711 = R.random_raw("alaw", 77, 1, 3)
    i24 = R.random_raw("i24", 31, 3, 4)
    i16 = R.random_raw("i16", 25, 1, 5)
    odd_list = b"LIST" + struct.pack("<I", 5) + b"INFOx" + b"\0"                 # odd size 5 + its pad byte
    cases = [
        (riff(3, 2, 48000, 32, f32), ("f32", 2, 48000, 50), f32),
        (riff(3, 1, 8000, 64, f64), ("f64", 1, 8000, 40), f64),
        (riff(6, 1, 8000, 8, g711), ("alaw", 1, 8000, 77), g711),
        (riff(7, 1, 8000, 8, g711), ("mulaw", 1, 8000, 77), g711),
        (riff(1, 3, 44100, 24, i24, extensible=True), ("i24", 3, 44100, 31), i24),
        (riff(3, 2, 48000, 32, f32, extensible=True), ("f32", 2, 48000, 50), f32),
        (riff(1, 1, 16000, 16, i16, before=odd_list), ("i16", 1, 16000, 25), i16),
        (riff(1, 1, 16000, 16, i16, data_size=0xFFFFFFFF), ("i16", 1, 16000, 25), i16),
        (riff(1, 1, 16000, 16, i16, data_size=0), ("i16", 1, 16000, 25), i16),
        (riff(1, 1, 16000, 16, i16, data_size=1000), ("i16", 1, 16000, 25), i16),                         # past the end of the file
        (riff(1, 2, 16000, 16, bytes(i16) + b"\x01\x02\x03", data_size=1000), ("i16", 2, 16000, 13), bytes(i16) + b"\x01\x02"),   # whole frames only
        (riff(1, 1, 16000, 16, i16, after=b"LIST" + struct.pack("<I", 4) + b"INFO"), ("i16", 1, 16000, 25), i16),
        (riff(1, 1, 16000, 16, b""), ("i16", 1, 16000, 0), i16[:0]),
    ]
    for i, (blob, meta, payload) in enumerate(cases):
        w = gigaam_amd.read_wav(write(tmp_path, f"c{i}.wav", blob))
        assert (w.fmt, w.channels, w.rate, w.frames) == meta, i
        assert np.array_equal(w.data, np.frombuffer(bytes(payload), np.uint8)), i


def test_read_wav_refusals(tmp_path):
    pcm = R.random_raw("i16", 10, 1, 0)
    ok = riff(1, 1, 16000, 16, pcm)
    bad = {
        "not_riff": b"RIFX" + ok[4:],
        "not_wave": ok[:8] + b"AVI " + ok[12:],
        "short": ok[:10],
        "empty": b"",
        "tag": riff(2, 1, 16000, 4, pcm),                      # ADPCM
        "mp3": riff(0x55, 1, 16000, 16, pcm),
        "width": riff(1, 1, 16000, 12, pcm),
        "float16": riff(3, 1, 16000, 16, pcm),
        "alaw16": riff(6, 1, 8000, 16, pcm),
        "channels": riff(1, 0, 16000, 16, pcm),
        "rate": riff(1, 1, 0, 16, pcm),
        "no_data": ok[:ok.index(b"data")],
        "data_first": b"RIFF" + struct.pack("<I", 4 + 8 + len(pcm)) + b"WAVE" + b"data" + struct.pack("<I", len(pcm)) + bytes(pcm),
        "ext_short": b"RIFF" + struct.pack("<I", 100) + b"WAVE" + b"fmt " + struct.pack("<I", 18) + struct.pack("<HHIIHHH", 0xFFFE, 1, 16000, 32000, 2, 16, 0)
                     + b"data" + struct.pack("<I", len(pcm)) + bytes(pcm),
    }
    for name, blob in bad.items():
        with pytest.raises(RuntimeError, match="^Failed to load audio$"):
            gigaam_amd.read_wav(write(tmp_path, name + ".wav", blob))
    for fn in (gigaam_amd.read_wav, gigaam_amd.decode_audio, lambda p: load_audio(p, backend="native")):
        with pytest.raises(RuntimeError, match="^Failed to load audio$"):
            fn(str(tmp_path / "missing.wav"))


# ------------------------------------------------------------------------------------------------------------ G.711
def test_g711_pins_and_all_codes():
    assert not re.search(r"^\s*(import|from)\s+audioop", open(R.__file__).read(), re.M)
    mu = R.mulaw_decode(np.arange(256, dtype=np.uint8))
    al = R.alaw_decode(np.arange(256, dtype=np.uint8))
    assert (mu[0xFF], mu[0x80], mu[0x00]) == (0, 32124, -32124)
    assert (al[0xD5], al[0x55], al[0xAA], al[0x2A]) == (8, -8, 32256, -32256)
    # an independent statement of both laws: segment / mantissa tables of ITU-T G.711
    for b in range(256):
        u = ~b & 0xFF
        mag = ((((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4)) - 0x84
        assert mu[b] == (-mag if u & 0x80 else mag)
        a = b ^ 0x55
        seg, man = (a & 0x70) >> 4, a & 0x0F
        mag = (man << 4) + 8 if seg == 0 else ((man << 4) + 0x108) << (seg - 1)
        assert al[b] == (mag if a & 0x80 else -mag)
    # the product's host decoders, all 256 codes of each law
    codes = np.arange(256, dtype=np.uint8)
    assert np.array_equal(audio._mulaw(codes), mu) and np.array_equal(audio._alaw(codes), al)
    assert len(set(mu.tolist())) == 255 and len(set(al.tolist())) == 256        # (mu-law has +0 and -0)


# ------------------------------------------------------------------------------------------------------------ decode_audio on the host
HOST_FORMATS = [("u8", 1, 8), ("i16", 1, 16), ("i24", 1, 24), ("i32", 1, 32), ("f32", 3, 32), ("f64", 3, 64), ("alaw", 6, 8), ("mulaw", 7, 8)]


@pytest.mark.parametrize("fmt,tag,bits", HOST_FORMATS)
def test_decode_audio_cpu_at_the_files_own_rate(tmp_path, fmt, tag, bits):
    for channels in (1, 2, 3):
        if fmt == "f64":
            raw = np.random.default_rng(7).standard_normal(101 * channels).astype("<f8").view(np.uint8)
            x = raw.view("<f8").astype(np.float32).reshape(-1, channels)
        else:
            raw = R.random_raw(fmt, 101, channels, seed=7 + channels)
            x = R.decode_samples(raw, fmt).reshape(-1, channels)
        p = write(tmp_path, f"{fmt}{channels}.wav", riff(tag, channels, 8000, bits, raw))
        for channel in [None, 0, 1][:1 + min(channels, 2)]:
            got = gigaam_amd.decode_audio(p, sample_rate=8000, channel=channel, device="cpu")
            assert got.dtype == torch.float32 and got.device.type == "cpu"
            assert np.array_equal(got.numpy().view(np.uint32), R.downmix(x, channel).view(np.uint32)), (channels, channel)
        with pytest.raises(ValueError):
            gigaam_amd.decode_audio(p, sample_rate=8000, channel=channels, device="cpu")
        with pytest.raises(_lib.GigaAMHipError):                          # anything that needs the filter: no CPU path
            gigaam_amd.decode_audio(p, sample_rate=16000, device="cpu")
    with pytest.raises(ValueError):
        gigaam_amd.decode_audio(p, sample_rate=383999, device="cpu")


def test_resample_has_no_cpu_path():
    with pytest.raises(_lib.GigaAMHipError):
        gigaam_amd.resample(torch.zeros(100), 8000)


# ------------------------------------------------------------------------------------------------------------ load_audio
def _pcm16_file(tmp_path, name, channels, rate, frames=1600):
    pcm = (np.sin(np.arange(frames * channels) / 7.0) * 12000).astype(np.int16)
    pcm[:2] = [-32768, 32767]
    p = str(tmp_path / name)
    with wave.open(p, "wb") as wf:
        wf.setnchannels(channels); wf.setsampwidth(2); wf.setframerate(rate); wf.writeframes(pcm.tobytes())
    return p, pcm


@pytest.mark.parametrize("backend", ["auto", "ffmpeg", "native"])
def test_load_audio_mono_pcm16_is_unchanged_under_every_backend(tmp_path, backend):
    if backend == "ffmpeg" and not HAVE_FFMPEG:
        pytest.skip("no ffmpeg on this machine")
    p, pcm = _pcm16_file(tmp_path, "m.wav", 1, 16000)
    want = torch.from_numpy(pcm.astype(np.float32)) / 32768.0
    x = load_audio(p, backend=backend)
    assert x.dtype == torch.float32 and x.device.type == "cpu" and torch.equal(x, want)
    prev = gigaam_amd.set_audio_backend(backend)
    try:
        assert audio.get_audio_backend() == backend
        assert torch.equal(gigaam_amd.load_audio(p), want)
    finally:
        assert gigaam_amd.set_audio_backend(prev) == backend
    with pytest.raises(ValueError):
        gigaam_amd.set_audio_backend("sox")
    with pytest.raises(ValueError):
        load_audio(p, backend="sox")


def test_load_audio_auto_takes_the_native_path_where_today_refuses(tmp_path):
    if HAVE_FFMPEG:
        pytest.skip("ffmpeg is installed: auto means ffmpeg")
    p, pcm = _pcm16_file(tmp_path, "s.wav", 2, 16000)
    x = load_audio(p, backend="auto")
    want = R.downmix(pcm.astype(np.float32).reshape(-1, 2) / np.float32(32768.0))
    assert x.device.type == "cpu" and np.array_equal(x.numpy().view(np.uint32), want.view(np.uint32))
    if not torch.cuda.is_available():
        p8, _ = _pcm16_file(tmp_path, "t.wav", 1, 8000)
        with pytest.raises(_lib.GigaAMHipError):
            load_audio(p8, backend="auto")


def test_new_names_are_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "gigaam_hip.h")).read()
    for name in ("gam_resample_plan", "gam_resample_tile", "gam_resample_table", "gam_resample_out_len", "gam_op_resample"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES
    assert "#define GAM_ABI_VERSION 1" in header
    for name in ("decode_audio", "resample", "read_wav", "set_audio_backend", "load_audio"):
        assert name in gigaam_amd.__all__ and callable(getattr(gigaam_amd, name))
