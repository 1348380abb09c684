"""Audio ingest without ffmpeg: a RIFF/WAVE reader and the GPU sample-format conversion / downmix / resampling stage in front of
``gam_frontend`` (gam_op_resample, gigaam_amd/csrc/gam_resample.h; the contract is in include/gigaam_hip.h, "audio ingest").

The reference decodes every file with an ffmpeg subprocess (gigaam/preprocess.py:12-40).  ``decode_audio`` does the same job for WAV
files -- PCM 8/16/24/32, float 32/64, G.711 A-law / mu-law, any channel count, any rate up to 384 kHz -- by uploading the raw bytes and
running one kernel; ``resample`` is the route for callers who hold tensors at another rate.  The filter is torchaudio's
(``sinc_interp_hann``, width 6, rolloff 0.99), not swresample's, and the result is fp32 rather than 16-bit: it differs numerically from
the ffmpeg path except for files that need no conversion.  As everywhere in this package there is no CPU path for the kernel's work:
only a file already at the target rate is converted on the host (numpy, bit-identical to the kernel's identity filter).
"""
from __future__ import annotations

import ctypes as C
import os
import struct
from typing import Dict, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._lib import GigaAMHipError

SAMPLE_RATE = 16000
BACKENDS = ("auto", "ffmpeg", "native")
_FMT_CODE = {"u8": _lib.RS_U8, "i16": _lib.RS_I16, "i24": _lib.RS_I24, "i32": _lib.RS_I32, "f32": _lib.RS_F32, "mulaw": _lib.RS_MULAW,
             "alaw": _lib.RS_ALAW}
_FMT_BYTES = {"u8": 1, "i16": 2, "i24": 3, "i32": 4, "f32": 4, "f64": 8, "mulaw": 1, "alaw": 1}
# WAVE format tag -> {bits per sample: format}
_WAVE_TAGS = {1: {8: "u8", 16: "i16", 24: "i24", 32: "i32"}, 3: {32: "f32", 64: "f64"}, 6: {8: "alaw"}, 7: {8: "mulaw"}}


def _check_backend(name: str) -> str:
    if name not in BACKENDS:
        raise ValueError(f"audio backend must be one of {BACKENDS}, not {name!r}")
    return name


_backend = _check_backend(os.environ.get("GAM_AUDIO_BACKEND", "auto"))


def set_audio_backend(name: str) -> str:
    """How ``load_audio`` decodes a file; returns the previous setting.  ``"auto"`` (the initial value unless ``GAM_AUDIO_BACKEND`` says
    otherwise): ffmpeg when it is installed; without it a mono PCM16 WAV at the target rate is read on the host and any other WAV goes
    through ``decode_audio``.  ``"ffmpeg"``: always the subprocess.  ``"native"``: always ``decode_audio``."""
    global _backend
    prev, _backend = _backend, _check_backend(name)
    return prev


def get_audio_backend() -> str:
    return _backend


class WavData(NamedTuple):
    """``data``: the raw interleaved frames as a uint8 array of ``frames * channels * bytes-per-sample`` bytes; ``fmt``: one of u8, i16,
    i24, i32, f32, f64, mulaw, alaw; ``rate`` in Hz."""
    data: np.ndarray
    fmt: str
    channels: int
    rate: int
    frames: int


def _parse_wav(path: str) -> WavData:
    size = os.path.getsize(path)
    with open(path, "rb") as fh:
        head = fh.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError("not RIFF/WAVE")
        fmt = None
        channels = rate = 0
        pos = 12
        while True:
            fh.seek(pos)
            ck = fh.read(8)
            if len(ck) < 8:
                raise ValueError("no data chunk")
            cid, csize = ck[:4], struct.unpack("<I", ck[4:])[0]
            pos += 8
            if cid == b"fmt ":
                body = fh.read(min(csize, 40))
                tag, channels, rate, _, _, bits = struct.unpack("<HHIIHH", body[:16])
                if tag == 0xFFFE:                      # WAVE_FORMAT_EXTENSIBLE: the tag is the first two bytes of the sub-format GUID
                    tag = struct.unpack("<H", body[24:26])[0]
                fmt = _WAVE_TAGS.get(tag, {}).get(bits)
                if fmt is None or channels < 1 or rate < 1:
                    raise ValueError("unsupported format")
            elif cid == b"data":
                if fmt is None:
                    raise ValueError("data before fmt")
                avail = size - pos
                n = avail if csize in (0, 0xFFFFFFFF) else min(csize, avail)     # (0 / 0xFFFFFFFF: a piped writer never patched the size)
                frame = channels * _FMT_BYTES[fmt]
                frames = n // frame
                data = np.fromfile(fh, dtype=np.uint8, count=frames * frame, offset=0) if frames else np.zeros(0, np.uint8)
                if data.size != frames * frame:
                    raise ValueError("short read")
                return WavData(data, fmt, channels, rate, frames)
            pos += csize + (csize & 1)                  # chunks are word-aligned: an odd size is followed by a pad byte


def read_wav(path: str) -> WavData:
    """Parse a RIFF/WAVE file: format tags 1 (PCM 8/16/24/32), 3 (float 32/64), 6 (A-law), 7 (mu-law) and 0xFFFE (extensible); unknown
    chunks before ``data`` are skipped; a ``data`` size of 0 or 0xFFFFFFFF reads to the end of the file, one past the end takes the whole
    frames present.  Anything else raises the reference's ``RuntimeError("Failed to load audio")``."""
    try:
        return _parse_wav(os.fspath(path))
    except (OSError, ValueError, struct.error, IndexError) as exc:
        raise RuntimeError("Failed to load audio") from exc


# ------------------------------------------------------------------------------------------------------------ host conversion
def _mulaw(b: np.ndarray) -> np.ndarray:
    u = (~b).astype(np.int32) & 0xFF
    mag = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84
    return np.where(u & 0x80, -mag, mag)


def _alaw(b: np.ndarray) -> np.ndarray:
    a = (b.astype(np.int32) ^ 0x55) & 0xFF
    e, m = (a >> 4) & 7, a & 15
    mag = np.where(e > 0, ((m << 4) + 0x108) << np.maximum(e - 1, 0), (m << 4) + 8)
    return np.where(a & 0x80, mag, -mag)


def _to_f32(data: np.ndarray, fmt: str) -> np.ndarray:
    """The kernel's conversions (include/gigaam_hip.h) in numpy; every scale is a power of two, so the results are bit-identical."""
    if fmt == "u8":
        return (data.astype(np.int32) - 128).astype(np.float32) * np.float32(1.0 / 128.0)
    if fmt == "i16":
        return data.view("<i2").astype(np.float32) * np.float32(1.0 / 32768.0)
    if fmt == "i24":
        b = data.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2].astype(np.int8).astype(np.int32) << 16)
        return v.astype(np.float32) * np.float32(1.0 / 8388608.0)
    if fmt == "i32":
        return data.view("<i4").astype(np.float32) * np.float32(2.0 ** -31)
    if fmt == "f32":
        return data.view("<f4").astype(np.float32)
    if fmt == "f64":
        return data.view("<f8").astype(np.float32)
    dec = _mulaw if fmt == "mulaw" else _alaw
    return dec(data).astype(np.float32) * np.float32(1.0 / 32768.0)


def _downmix(x: np.ndarray, channel: Optional[int]) -> np.ndarray:
    if channel is not None:
        return np.ascontiguousarray(x[:, channel])
    s = x[:, 0].copy()
    for c in range(1, x.shape[1]):
        s += x[:, c]
    return s * (np.float32(1.0) / np.float32(x.shape[1]))


# ------------------------------------------------------------------------------------------------------------ the kernel
class _Table(NamedTuple):
    up: int
    down: int
    taps: int
    coeff: Tensor
    first: Tensor


_tables: Dict[Tuple[int, int, str], _Table] = {}


def resample_plan(rate_in: int, rate_out: int) -> Tuple[int, int, int]:
    """(N, O, K): output and input samples per period and taps per output.  ``ValueError`` for a rate outside 1..384000 or a filter table
    of more than 2**18 entries (rates with a tiny common divisor)."""
    lib = _lib.load_library()
    up, down, taps = C.c_int(), C.c_int(), C.c_int()
    rc = lib.gam_resample_plan(int(rate_in), int(rate_out), C.byref(up), C.byref(down), C.byref(taps))
    if rc == -1:
        raise ValueError(f"sample rates must lie in 1..384000 Hz (got {rate_in} -> {rate_out})")
    if rc != 0:
        raise ValueError(f"resampling {rate_in} -> {rate_out} Hz needs a filter table of more than 2**18 entries; convert through a rate "
                         "that shares a larger divisor")
    return up.value, down.value, taps.value


def _out_len(rate_in: int, rate_out: int, n: int) -> int:
    return int(_lib.load_library().gam_resample_out_len(int(rate_in), int(rate_out), int(n)))


def _table(rate_in: int, rate_out: int, device: torch.device) -> _Table:
    key = (int(rate_in), int(rate_out), str(device))
    t = _tables.get(key)
    if t is None:
        up, down, taps = resample_plan(rate_in, rate_out)
        coeff = np.empty(up * taps, np.float32)
        first = np.empty(up, np.int32)
        rc = _lib.load_library().gam_resample_table(int(rate_in), int(rate_out), C.c_void_p(coeff.ctypes.data), C.c_void_p(first.ctypes.data))
        if rc != 0:
            raise GigaAMHipError(f"gam_resample_table failed ({rc})")
        t = _tables[key] = _Table(up, down, taps, torch.from_numpy(coeff).to(device), torch.from_numpy(first).to(device))
    return t


def _cuda_device(device: Union[str, torch.device, None], what: str) -> torch.device:
    dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if dev.type != "cuda":
        raise GigaAMHipError(f"{what} runs on the GPU (gam_op_resample); there is no CPU path")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _run(src: Tensor, fmt: str, channels: int, channel: Optional[int], len_in: Optional[Tensor], B: int, frames: int, rate_in: int,
         rate_out: int, L_out: int, want_len: bool) -> Tuple[Tensor, Optional[Tensor]]:
    dev = src.device
    tab = _table(rate_in, rate_out, dev)
    out = torch.empty((B, L_out), dtype=torch.float32, device=dev)
    len_out = torch.empty((B,), dtype=torch.int64, device=dev) if want_len else None
    with torch.cuda.device(dev):
        rc = _lib.load_library().gam_op_resample(
            C.c_void_p(src.data_ptr()), _FMT_CODE[fmt], channels, -1 if channel is None else int(channel),
            C.c_void_p(0 if len_in is None else len_in.data_ptr()), B, frames, int(rate_in), int(rate_out),
            C.c_void_p(tab.coeff.data_ptr()), C.c_void_p(tab.first.data_ptr()), C.c_void_p(out.data_ptr()), L_out,
            C.c_void_p(0 if len_out is None else len_out.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise GigaAMHipError(f"gam_op_resample failed ({rc})")
    return out, len_out


def decode_audio(path: str, sample_rate: int = SAMPLE_RATE, channel: Optional[int] = None,
                 device: Union[str, torch.device, None] = None) -> Tensor:
    """A WAV file as mono fp32 ``[n]`` at ``sample_rate`` on ``device`` (default: the GPU when there is one).  ``channel=None`` takes the
    mean of the channels (an fp32 sum in channel order times ``1 / C`` -- for more than two channels this is not ffmpeg's layout-aware
    matrix); ``channel=k`` takes channel k, e.g. one speaker of a two-channel call.  The raw bytes are uploaded and converted, downmixed
    and resampled by one kernel.  On a CPU device only a file already at ``sample_rate`` is converted (numpy, bit-identical to the
    kernel); anything that needs the filter raises ``GigaAMHipError``."""
    wav = read_wav(path)
    if channel is not None and not 0 <= int(channel) < wav.channels:
        raise ValueError(f"channel {channel} of a file with {wav.channels} channel(s)")
    resample_plan(wav.rate, sample_rate)        # ValueError for a refused rate pair, before any device work
    data, fmt = wav.data, wav.fmt
    dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if dev.type == "cpu":
        if wav.rate != sample_rate:
            raise GigaAMHipError(f"resampling {wav.rate} -> {sample_rate} Hz runs on the GPU (gam_op_resample); there is no CPU path")
        return torch.from_numpy(_downmix(_to_f32(data, fmt).reshape(wav.frames, wav.channels), channel))
    dev = _cuda_device(dev, "decode_audio")
    if fmt == "f64":                             # the one conversion done on the host: the kernel has no fp64 input
        data, fmt = data.view("<f8").astype(np.float32).view(np.uint8), "f32"
    n_out = _out_len(wav.rate, sample_rate, wav.frames)
    if n_out == 0:
        return torch.zeros(0, dtype=torch.float32, device=dev)
    src = torch.from_numpy(data).to(dev)
    out, _ = _run(src, fmt, wav.channels, channel, None, 1, wav.frames, wav.rate, sample_rate, n_out, False)
    return out[0]


def resample(wav: Tensor, orig_rate: int, new_rate: int = SAMPLE_RATE, lengths: Optional[Tensor] = None):
    """Resample an fp32 device tensor ``[L]`` or ``[B, L]`` from ``orig_rate`` to ``new_rate``.  With ``lengths`` (``[B]``: the valid
    samples of each row; what lies behind them is ignored) returns ``(out, out_lengths)`` with ``out`` zero behind each row's
    ``out_lengths[b] = ceil(N lengths[b] / O)``; without, returns ``out``."""
    if wav.dim() not in (1, 2):
        raise ValueError("resample takes a [L] or [B, L] tensor")
    dev = _cuda_device(wav.device, "resample")
    resample_plan(orig_rate, new_rate)
    x = wav.to(torch.float32).contiguous()
    x2 = x[None] if x.dim() == 1 else x
    B, L = x2.shape
    len_in = None
    if lengths is not None:
        len_in = torch.as_tensor(lengths).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        if len_in.numel() != B:
            raise ValueError("lengths must hold one entry per row")
    L_out = _out_len(orig_rate, new_rate, L)
    if B == 0 or L_out == 0:
        out, len_out = torch.zeros((B, L_out), dtype=torch.float32, device=dev), torch.zeros((B,), dtype=torch.int64, device=dev)
    else:
        out, len_out = _run(x2, "f32", 1, None, len_in, B, L, orig_rate, new_rate, L_out, lengths is not None)
    out = out[0] if wav.dim() == 1 else out
    return (out, len_out) if lengths is not None else out
