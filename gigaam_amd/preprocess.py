"""``cfg.preprocessor`` slot: FeatureExtractor on the HIP frontend.

Mirrors reference gigaam/preprocess.py:12-98 (same constructor kwargs, call
contract ``(wav [B,L], len [B]) -> (feat [B,n_mels,T], len i64 [B])`` and
``out_len``); the compute is gam_frontend in libgigaam_hip.so.
"""
from __future__ import annotations

import shutil
import subprocess
import wave
from typing import Any, Dict, Mapping, Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from . import audio
from .engine import HipEngine, build_config

SAMPLE_RATE = 16000


def _ffmpeg_pcm16(audio_path: str, sample_rate: int) -> np.ndarray:
    cmd = ["ffmpeg", "-nostdin", "-threads", "0", "-i", audio_path, "-f", "s16le", "-ac", "1",
           "-acodec", "pcm_s16le", "-ar", str(sample_rate), "-"]
    try:
        raw = subprocess.run(cmd, capture_output=True, check=True).stdout
    except (subprocess.CalledProcessError, OSError) as exc:
        raise RuntimeError("Failed to load audio") from exc
    return np.frombuffer(raw, dtype=np.int16)


def _plain_pcm16(audio_path: str, sample_rate: int) -> Optional[np.ndarray]:
    """The samples of a mono PCM16 WAV at ``sample_rate`` (stdlib ``wave``), or None for any other file."""
    try:
        with wave.open(audio_path, "rb") as wf:
            if wf.getnchannels() == 1 and wf.getsampwidth() == 2 and wf.getframerate() == sample_rate:
                return np.frombuffer(wf.readframes(wf.getnframes()), dtype=np.int16)
    except (wave.Error, OSError, EOFError):
        pass
    return None


def load_audio(audio_path: str, sample_rate: int = SAMPLE_RATE, backend: Optional[str] = None) -> Tensor:
    """A file as mono fp32 at ``sample_rate`` on the CPU.  ``backend`` (default: ``audio.set_audio_backend`` / ``GAM_AUDIO_BACKEND``):

    ``"ffmpeg"``  decode to mono ``sample_rate`` PCM16 and scale by 1/32768 (reference preprocess.py:12-40 pipes the file through ffmpeg);
    ``"native"``  ``audio.decode_audio``: our WAV reader and the GPU conversion / downmix / resampling kernel (a file already at the rate
                  needs no GPU);
    ``"auto"``    ffmpeg where it is installed; without it a PCM16 mono WAV at the right rate is read with the stdlib ``wave`` module
                  -- identical samples, no resampling -- and every other file goes the native way.

    What cannot be read raises the reference's ``RuntimeError("Failed to load audio")``."""
    backend = audio.get_audio_backend() if backend is None else audio._check_backend(backend)
    if backend == "ffmpeg" or (backend == "auto" and shutil.which("ffmpeg") is not None):
        pcm: Optional[np.ndarray] = _ffmpeg_pcm16(audio_path, sample_rate)
    else:
        pcm = _plain_pcm16(audio_path, sample_rate) if backend == "auto" else None
    if pcm is None:
        return audio.decode_audio(audio_path, sample_rate).cpu()
    return torch.from_numpy(pcm.astype(np.float32)) / 32768.0


class _EngineModule(nn.Module):
    """Base of the operator shims: holds the cfg of its slot and a (possibly shared)
    HipEngine.  ``_anchor`` is the one real parameter the reference's
    ``_device``/``_dtype`` properties need (gigaam/model.py:39-45)."""

    _prefix = ""

    def __init__(self) -> None:
        super().__init__()
        self._anchor = nn.Parameter(torch.zeros(1), requires_grad=False)
        self._engine: Optional[HipEngine] = None
        self._pending: Dict[str, Tensor] = {}

    # weights live inside the library, not in torch parameters
    def load_state_dict(self, state_dict: Mapping[str, Tensor], strict: bool = True, assign: bool = False):  # type: ignore[override]
        self._pending = {self._prefix + k: v for k, v in state_dict.items() if isinstance(v, Tensor)}
        self._engine = None
        return nn.modules.module._IncompatibleKeys([], [])

    def attach(self, engine: HipEngine) -> None:
        self._engine = engine
        self._pending = {}

    def _cfg_trees(self) -> Tuple[Any, Any, Any]:
        raise NotImplementedError

    @property
    def engine(self) -> HipEngine:
        if self._engine is None:
            pre, enc, head = self._cfg_trees()
            self._engine = HipEngine(build_config(pre, enc, head), self._pending, self._anchor.device)
        return self._engine

    def half(self):
        """``model.encoder.half()`` (reference gigaam/__init__.py:188-189, fp16_encoder=True on a GPU): the storage
        contract follows -- ``_dtype`` becomes float16 (the anchor parameter is converted like any other), inputs
        arrive as float16 and ``encoded`` leaves as float16 -- while the kernels keep computing in fp32."""
        return super().half()


class FeatureExtractor(_EngineModule):
    _prefix = "preprocessor."

    def __init__(self, sample_rate: int, features: int, **kwargs: Any):
        super().__init__()
        self.sample_rate = sample_rate
        self.features = features
        self.hop_length = kwargs.get("hop_length", sample_rate // 100)
        self.win_length = kwargs.get("win_length", sample_rate // 40)
        self.n_fft = kwargs.get("n_fft", sample_rate // 40)
        self.center = kwargs.get("center", True)

    def _cfg_trees(self):
        pre = {"sample_rate": self.sample_rate, "features": self.features, "hop_length": self.hop_length,
               "win_length": self.win_length, "n_fft": self.n_fft, "center": self.center}
        return pre, None, None

    def out_len(self, input_lengths: Tensor) -> Tensor:
        if self.center:
            return input_lengths.div(self.hop_length, rounding_mode="floor").add(1).long()
        return (input_lengths - self.win_length).div(self.hop_length, rounding_mode="floor").add(1).long()

    def forward(self, input_signal: Tensor, length: Tensor) -> Tuple[Tensor, Tensor]:
        return self.engine.frontend(input_signal, length)
