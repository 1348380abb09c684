"""Model assembly with the reference's public surface (gigaam/model.py:16-259):
``GigaAM.forward / embed_audio / prepare_wav``, ``GigaAMASR.transcribe /
transcribe_longform``.  The four cfg slots are instantiated by class path exactly
like ``hydra.utils.instantiate`` does in the reference (model.py:24-25,93-94), but
resolve to the HIP-backed operators of this package, which share ONE library
handle per model.
"""
from __future__ import annotations

import os
from contextlib import contextmanager
from typing import Any, Callable, Dict, List, Mapping, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

from . import decoder as _decoder
from . import decoding as _decoding
from . import encoder as _encoder
from . import preprocess as _preprocess
from . import wildcard as _wildcard
from ._lib import GigaAMHipError
from .engine import HipEngine, build_config
from .preprocess import SAMPLE_RATE, load_audio
from .types import (AlignmentResult, ConfidenceResult, Hypothesis, KeywordSearchResult, LongformAlignmentResult, LongformConfidenceResult,
                    LongformTranscriptionResult, NBestResult, ScoredWord, Segment, TranscriptionResult, Word, nbest_posteriors)

LONGFORM_THRESHOLD = 25 * SAMPLE_RATE

_TARGETS = {
    "FeatureExtractor": _preprocess.FeatureExtractor,
    "ConformerEncoder": _encoder.ConformerEncoder,
    "CTCHead": _decoder.CTCHead,
    "RNNTHead": _decoder.RNNTHead,
    "Linear": _decoder.EmoHead,   # cfg.head of the emotion model (torch.nn.Linear)
    "CTCGreedyDecoding": _decoding.CTCGreedyDecoding,
    "RNNTGreedyDecoding": _decoding.RNNTGreedyDecoding,
    "RNNTBeamDecoding": _decoding.RNNTBeamDecoding,
}


def _node(cfg: Any, key: str) -> Any:
    return cfg[key] if isinstance(cfg, Mapping) else getattr(cfg, key)


def _plain(x: Any) -> Any:
    """A cfg node as plain dict / list / scalar.  The reference's checkpoints hold omegaconf containers
    (``DictConfig`` is a ``MutableMapping``, ``ListConfig`` a ``Sequence``, both also attribute-style); anything with
    the mapping or sequence PROTOCOL is accepted, by interface, not by class name."""
    if isinstance(x, Mapping) or (hasattr(x, "keys") and hasattr(x, "__getitem__")):
        return {k: _plain(x[k]) for k in x.keys()}
    if isinstance(x, (str, bytes)):
        return x
    if isinstance(x, Sequence):
        return [_plain(v) for v in x]
    return x


def instantiate(node: Any) -> Any:
    """``_target_`` class-path instantiation; 'gigaam.encoder.ConformerEncoder' and
    'gigaam_amd.encoder.ConformerEncoder' both resolve here."""
    kw = dict(_plain(node))
    target = kw.pop("_target_")
    cls = _TARGETS.get(target.rsplit(".", 1)[-1])
    if cls is None:
        raise ValueError(f"no MI355X implementation for {target}")
    return cls(**kw)


@contextmanager
def _f32_mode(eng: HipEngine):
    """The engine under GAM_GEMM_F32 for the block; the mode it had comes back whatever the block does."""
    mode = eng.gemm_mode
    eng.set_gemm_mode("f32")
    try:
        yield
    finally:
        eng.set_gemm_mode(mode)


def _pipeline(batches, launch: Callable[[int, Any], Any], emit: Callable[[Any], None]) -> None:
    """The one-batch software pipeline of the chunked longform routes: ``launch(n, batch)`` (device work, no host sync) runs BEFORE
    ``emit`` brings what ``launch`` returned for batch n - 1 to the host; the last batch is emitted after the loop."""
    pending: List[Any] = []
    for n, batch in enumerate(batches):
        pending.append(launch(n, batch))
        if len(pending) > 1:
            emit(pending.pop(0))
    for handle in pending:
        emit(handle)


class GigaAM(nn.Module):
    _check_range = True   # forward() reads the split-fp16 range flag (one 4-byte D2H + sync) and falls back to fp32

    def __init__(self, cfg: Any):
        super().__init__()
        self.cfg = cfg
        self.preprocessor = instantiate(_node(cfg, "preprocessor"))
        self.encoder = instantiate(_node(cfg, "encoder"))

    def _head_cfg(self) -> Any:
        return None

    def load_state_dict(self, state_dict: Mapping[str, Tensor], strict: bool = True, assign: bool = False):  # type: ignore[override]
        """Hand every tensor to the library once (re-laid out there) and share the handle."""
        self._state = {k: v for k, v in state_dict.items() if isinstance(v, Tensor)}
        self._build_engine()
        return nn.modules.module._IncompatibleKeys([], [])

    def _build_engine(self) -> None:
        dev = self._device
        if dev.type != "cuda" or getattr(self, "_state", None) is None:
            return  # built on .to(device)
        conf = build_config(_node(self.cfg, "preprocessor"), _node(self.cfg, "encoder"), self._head_cfg())
        eng = HipEngine(conf, self._state, dev)
        self._state = None
        for m in (self.preprocessor, self.encoder, getattr(self, "head", None)):
            if m is not None:
                m.attach(eng)

    def _apply(self, fn, recurse=True):  # .to(device) / .cuda()
        out = super()._apply(fn, recurse)
        self._build_engine()
        return out

    def forward(self, features: Tensor, feature_lengths: Tensor) -> Tuple[Tensor, Tensor]:
        """wav [B,L], len [B] -> encoded [B,d_model,T'], len i32 [B]  (model.py:27-37;
        the reference wraps the encoder in fp16 autocast on GPU, this path stays fp32).  The public call checks the
        split-fp16 range flag itself (one 4-byte D2H + sync: the caller is about to read the tensor anyway); the
        transcribe paths read the flag together with the decode counts instead (``_encode`` + decoding.finish)."""
        host = self._host_feat_lengths(feature_lengths)     # (lengths given on the CPU: a ragged batch runs on its valid frames only)
        features, feature_lengths = self.preprocessor(features, feature_lengths)
        out = self.encoder(features, feature_lengths, host) if host is not None else self.encoder(features, feature_lengths)
        eng = getattr(self.encoder, "engine", None)
        if self._check_range and eng is not None and eng.gemm_mode != "f32" and eng.range_flag():
            # an activation outside fp16's range reached a split-fp16 GEMM operand (include/gigaam_hip.h,
            # gam_range_flag): the batch is repeated on the exact-fp32 MFMA path, which has no such limit
            self._warn_range("this batch was")
            with _f32_mode(eng):
                out = self.encoder(features, feature_lengths, host) if host is not None else self.encoder(features, feature_lengths)
        return out

    def _host_feat_lengths(self, wav_lengths) -> Optional[list]:
        """Feature-frame counts on the host when the caller's sample counts are on the host (no sync is ever made to get them)."""
        eng = getattr(self.encoder, "engine", None)
        if eng is None or not hasattr(eng, "host_feat_lengths"):
            return None
        return eng.host_feat_lengths(wav_lengths)

    def set_arithmetic(self, mode: str) -> None:
        """Arithmetic of the dense contractions (include/gigaam_hip.h, gam_set_gemm_mode): "f16x3" -- the default, a
        three-term fp16 split with fp32 accumulation, fp32-equivalent (what every parity claim of this package is made in);
        "f32" -- exact fp32 MFMA; "f16" -- OPT-IN speed mode, one fp16 MFMA per product: the contract of the reference's
        own GPU default (fp16 autocast, gigaam/model.py:34-37), not of its CPU path.  Not part of the reference's API."""
        self.encoder.engine.set_gemm_mode(mode)

    @staticmethod
    def _warn_range(what: str, stacklevel: int = 3) -> None:
        import warnings
        warnings.warn(f"gigaam_amd: activation beyond the split-fp16 GEMM range; {what} recomputed with "
                      "GAM_GEMM_F32 (set GAM_GEMM_MODE=f32 to use that path throughout)", RuntimeWarning, stacklevel=stacklevel)

    def _encode(self, wav: Tensor, lengths: Tensor, host_lengths=None) -> Tuple[Tensor, Tensor]:
        """Internal twin of ``forward`` for the transcribe paths: fp32 in, fp32 out whatever ``fp16_encoder`` says (the
        fp16 storage contract of reference __init__.py:188-189 applies to what ``forward`` / ``embed_audio`` RETURN, not
        to what the head consumes here), no host sync and no range check -- the caller reads the flag with the counts."""
        host = self._host_feat_lengths(lengths if host_lengths is None else host_lengths)
        feat, flen = self.preprocessor(wav.to(torch.float32), lengths)
        return self.encoder.forward_f32(feat, flen, host)

    def _encode_batch(self, wav: Tensor, lengths: Tensor) -> Tuple[Tensor, Tensor]:
        """``_encode`` of a caller's collated batch, moved to the device; as launch_batch: sample counts still on the host (a CPU
        ``lengths``) give a ragged batch packed rows."""
        host = lengths if (isinstance(lengths, Tensor) and not lengths.is_cuda) else None
        return self._encode(wav.to(self._device), lengths.to(self._device), host)

    def _with_f32_fallback(self, fn: Callable[[], Any], what: str, stacklevel: int = 3) -> Any:
        """Run ``fn``; if the decode it collects reports the range flag (decoding.RangeOverflow), warn and run it again
        under GAM_GEMM_F32.  ``stacklevel``: the warning names the frame that many above ``_warn_range`` (3: this method's caller)."""
        try:
            return fn()
        except _decoding.RangeOverflow:
            eng = self.encoder.engine
            self._warn_range(what, stacklevel)
            with _f32_mode(eng):
                return fn()

    def _file_run(self, run: Callable[[], Any]) -> Any:
        """The fp32 rerun protocol of every file-level longform route: ``run`` -- the whole file, raising decoding.RangeOverflow on a
        collected flag -- under ``_with_f32_fallback``.  A flag left behind by earlier direct engine use must not cost the file an
        fp32 rerun: it is read (that clears it) first."""
        eng = getattr(self.encoder, "_engine", None)      # (None: not built yet -- then nothing has run on it either)
        if eng is not None and eng.gemm_mode != "f32":
            eng.range_flag()
        return self._with_f32_fallback(run, "the file was", stacklevel=4)      # (the warning names the route, as it always has)

    @property
    def _device(self) -> torch.device:
        return next(self.parameters()).device

    @property
    def _dtype(self) -> torch.dtype:
        # the reference's first parameter is the encoder's (its FeatureExtractor holds buffers only): model.py:43-45
        return next(self.encoder.parameters()).dtype

    def prepare_wav(self, wav_file: str) -> Tuple[Tensor, Tensor]:
        wav = load_audio(wav_file)
        wav = wav.to(self._device).to(self._dtype).unsqueeze(0)
        length = torch.full([1], wav.shape[-1], device=self._device)
        return wav, length

    def embed_audio(self, wav_file: str) -> Tuple[Tensor, Tensor]:
        wav, length = self.prepare_wav(wav_file)
        return self.forward(wav, length)

    def _prepare_wav_f32(self, wav_file: str) -> Tuple[Tensor, Tensor]:
        """``prepare_wav`` without the cast to ``_dtype``: the transcribe paths feed the fp32 frontend fp32 samples
        (PCM16 / 32768 is exact in fp32; through fp16 it would keep 11 bits)."""
        wav = load_audio(wav_file).to(self._device).unsqueeze(0)
        return wav, torch.full([1], wav.shape[-1], device=self._device)

    def _encode_checked(self, wav: Tensor, lengths: Tensor) -> Tuple[Tensor, Tensor]:
        """``_encode`` + the blocking range check of ``forward`` (for heads that bring no counts to the host)."""
        out = self._encode(wav, lengths)
        eng = self.encoder.engine
        if self._check_range and eng.gemm_mode != "f32" and eng.range_flag():
            self._warn_range("this batch was")
            with _f32_mode(eng):
                out = self._encode(wav, lengths)
        return out


class GigaAMEmo(GigaAM):
    """Emotion recognition model (reference gigaam/model.py:262-285): encoder + time pooling +
    linear head + softmax; ``cfg.id2name`` maps class index -> name."""

    def __init__(self, cfg: Any):
        super().__init__(cfg)
        self.head = instantiate(_node(cfg, "head"))
        self.id2name = _plain(_node(cfg, "id2name"))

    def _head_cfg(self) -> Any:
        return _node(self.cfg, "head")

    def get_probs(self, wav_file: str) -> Dict[str, float]:
        wav, length = self._prepare_wav_f32(wav_file)
        encoded, _ = self._encode_checked(wav, length)
        # the reference pools over the whole T' axis of its single, unpadded file (model.py:278-280)
        probs = self.head.probs(encoded)[0].tolist()
        names = self.id2name
        return {(names[i] if not isinstance(names, dict) else names.get(i, names.get(str(i)))): probs[i] for i in range(len(probs))}

    def get_probs_batch(self, wav: Tensor, lengths: Tensor) -> Tensor:
        """Batched variant: wav [B,L], lengths [B] -> probabilities [B,n_classes]; the mean runs over each
        utterance's valid encoder frames."""
        encoded, enc_len = self._encode_checked(wav.to(self._device), lengths.to(self._device))
        return self.head.probs(encoded, enc_len)


class GigaAMASR(GigaAM):
    def __init__(self, cfg: Any):
        super().__init__(cfg)
        self.head = instantiate(_node(cfg, "head"))
        self.decoding = instantiate(_node(cfg, "decoding"))

    def _head_cfg(self) -> Any:
        return _node(self.cfg, "head")

    def _with_words(self, decoded, wav_lens: Tensor, encoded_len: Tensor, word_timestamps: bool, event=None):
        """``event``: the decode's completion event (``engine.Decoded.event``) when the caller has one -- the lengths are then
        copied on the collect stream behind THAT event; without one the collect stream waits for the current stream (correct
        for any caller, e.g. the reference-style ``_decode(enc_cuda, enc_len_cuda, wav_lens_cpu, word_timestamps=True)``)."""
        if not word_timestamps:
            return [(text, None) for text, _, _ in decoded]
        from .timestamps_utils import compute_frame_shift, frames_to_words

        on_dev = [t for t in (wav_lens, encoded_len) if t.is_cuda]
        if on_dev:
            # on the collect stream: a copy on the launch stream would queue behind the NEXT batch's kernels in the one-batch
            # pipelines.  The ordering is explicit: the decode's own event, or everything enqueued so far
            dev = on_dev[0].device
            side = HipEngine._collect_stream(dev)
            if event is not None:
                side.wait_event(event)
            else:
                side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                wl, el = wav_lens.cpu().tolist(), encoded_len.cpu().tolist()
            for t in on_dev:          # (record_stream is not defined for host tensors)
                t.record_stream(side)
        else:
            wl, el = wav_lens.tolist(), encoded_len.tolist()
        out: List[Tuple[str, Optional[List[Word]]]] = []
        for i, (text, ids, frames) in enumerate(decoded):
            shift = compute_frame_shift(int(wl[i]), int(el[i]))
            out.append((text, frames_to_words(self.decoding.tokenizer, ids, frames, shift)))
        return out

    def _decode(self, encoded: Tensor, encoded_len: Tensor, wav_lens: Tensor,
                word_timestamps: bool = False) -> List[Tuple[str, Optional[List[Word]]]]:
        """reference model.py:96-124"""
        return self._with_words(self.decoding.decode(self.head, encoded, encoded_len), wav_lens, encoded_len, word_timestamps)

    def set_decoding(self, beam_size: Optional[int] = None, hotwords: Optional[Sequence[Union[str, List[int]]]] = None,
                     hotword_boost: float = 2.0, lm=None, lm_weight: float = 0.5, word_bonus: float = 1.0) -> None:
        """RNN-T models: switch the decoding object (``cfg.decoding``'s role; NeMo's ``change_decoding_strategy``).  ``beam_size``
        (1..32), ``hotwords`` (strings in the vocabulary or token ids) and / or ``lm`` (an ``NgramLM`` or a path to an ARPA / ``.npz``
        file: ``lm_weight`` * ln P(word | history) + ``word_bonus`` per word) select ``decoding.RNNTBeamDecoding``; hotwords or an LM
        alone mean ``beam_size=4``.  With none of them, ``RNNTGreedyDecoding`` again.  The vocabulary and ``max_symbols_per_step``
        stay.  Every transcribe path then decodes that way (each longform segment starts its LM history at <s>).  CTC heads take
        the beam options per call instead (TypeError here)."""
        dec = self.decoding
        if not isinstance(dec, _decoding.RNNTGreedyDecoding):
            raise TypeError("set_decoding is for RNN-T heads; CTC heads take beam_size / hotwords per call")
        if beam_size is not None and not 1 <= int(beam_size) <= 32:
            raise ValueError(f"beam_size {beam_size} outside [1, 32]")
        new = _decoding.RNNTGreedyDecoding.__new__(
            _decoding.RNNTGreedyDecoding if beam_size is None and hotwords is None and lm is None else _decoding.RNNTBeamDecoding)
        new.tokenizer, new.blank_id, new.max_symbols = dec.tokenizer, dec.blank_id, dec.max_symbols
        if isinstance(new, _decoding.RNNTBeamDecoding):
            if not 1 <= new.max_symbols <= 16:
                raise ValueError(f"max_symbols_per_step {new.max_symbols} outside [1, 16] for the RNN-T beam search")
            new.beam_size = 4 if beam_size is None else int(beam_size)
            new.hotwords = list(hotwords) if hotwords else []
            new.hotword_boost = float(hotword_boost)
            new.set_lm(lm, lm_weight, word_bonus)
        self.decoding = new

    # ---- the launch / collect pair every transcribe path is built from (public: a driver -- bench.py, shard.run_sharded,
    #      a test -- can interleave them, or replace them to script the decode)
    def _beam_width(self, beam_size: Optional[int], hotwords, lm=None) -> Optional[int]:
        """The beam width of a transcribe call: None (greedy) when no option is given, 8 for hotwords or an LM alone."""
        if beam_size is None and hotwords is None and lm is None:
            return None
        if not isinstance(self.decoding, _decoding.CTCGreedyDecoding):
            raise TypeError("beam search needs a CTC head")
        return 8 if beam_size is None else int(beam_size)

    def launch_batch(self, wav: Tensor, lengths: Tensor, overlap: bool = False, host_lengths=None, *, beam_size: Optional[int] = None,
                     hotwords: Optional[Sequence[Union[str, List[int]]]] = None, hotword_boost: float = 2.0, lm=None,
                     lm_weight: float = 0.5, word_bonus: float = 1.0):
        """Device half of ``transcribe_batch``: frontend + encoder + greedy decode of a collated batch (wav [B,L] zero
        padded, len [B]) launched on the current stream, NO host sync.  Returns an opaque handle for ``collect_batch``.
        ``overlap=True`` says another ``launch_batch`` follows before this one is collected: an RNN-T decode then runs on
        the decode side stream BESIDE the next batch's encoder (decoding.RNNTGreedyDecoding.decode_device).
        ``beam_size`` / ``hotwords`` / ``lm`` (CTC heads only) decode by prefix beam search instead (decoding.decode_beam_device)."""
        width = self._beam_width(beam_size, hotwords, lm)
        # sample counts on the host (given, or ``lengths`` itself still a CPU tensor): a ragged batch then runs on its valid frames only
        host = host_lengths if host_lengths is not None else (lengths if (isinstance(lengths, Tensor) and not lengths.is_cuda) else None)
        wav, lengths = wav.to(self._device), lengths.to(self._device)
        encoded, encoded_len = self._encode(wav, lengths, host)
        if width is not None:
            return (self.decoding.decode_beam_device(self.head, encoded, encoded_len, width, hotwords, hotword_boost, lm, lm_weight, word_bonus),
                    lengths, encoded_len)
        return self.decoding.decode_device(self.head, encoded, encoded_len, overlap=overlap), lengths, encoded_len

    def collect_batch(self, handle, word_timestamps: bool = False) -> List[Tuple[str, Optional[List[Word]]]]:
        """Host half: blocks on the handle's decode, detokenises, builds word timestamps.  Raises
        ``decoding.RangeOverflow`` if the split-fp16 range flag was set (the callers below repeat in fp32)."""
        dev_out, wav_lens, encoded_len = handle
        return self._with_words(self.decoding.finish(dev_out), wav_lens, encoded_len, word_timestamps, event=getattr(dev_out, "event", None))

    @torch.inference_mode()
    def transcribe(self, wav_file: str, word_timestamps: bool = False, *, beam_size: Optional[int] = None,
                   hotwords: Optional[Sequence[Union[str, List[int]]]] = None, hotword_boost: float = 2.0, lm=None,
                   lm_weight: float = 0.5, word_bonus: float = 1.0) -> TranscriptionResult:
        """``beam_size`` (1..32) decodes by CTC prefix beam search; ``hotwords`` (strings in the vocabulary or token ids; alone
        they mean ``beam_size=8``) bias it toward those phrases, ``hotword_boost`` per matched token.  ``lm`` (an ``NgramLM`` or a
        path to an ARPA / ``.npz`` file; alone it means ``beam_size=8``) fuses a word n-gram LM: ``lm_weight`` * ln P(word |
        history) + ``word_bonus`` per word.  CTC heads only (TypeError)."""
        self._beam_width(beam_size, hotwords, lm)
        wav, length = self._prepare_wav_f32(wav_file)
        if length.item() > LONGFORM_THRESHOLD:
            raise ValueError("Too long wav file, use 'transcribe_longform' method.")
        text, words = self.transcribe_batch(wav, length, word_timestamps, beam_size=beam_size, hotwords=hotwords,
                                            hotword_boost=hotword_boost, lm=lm, lm_weight=lm_weight, word_bonus=word_bonus)[0]
        return TranscriptionResult(text=text, words=words)

    @torch.inference_mode()
    def transcribe_batch(self, wav: Tensor, lengths: Tensor, word_timestamps: bool = False, *, beam_size: Optional[int] = None,
                         hotwords: Optional[Sequence[Union[str, List[int]]]] = None, hotword_boost: float = 2.0, lm=None,
                         lm_weight: float = 0.5, word_bonus: float = 1.0):
        """Batched twin of ``transcribe`` on an already collated batch (wav [B,L] zero
        padded, len [B]) -- the unit bench.py and the longform driver iterate."""
        if self._beam_width(beam_size, hotwords, lm) is None:
            return self._with_f32_fallback(lambda: self.collect_batch(self.launch_batch(wav, lengths), word_timestamps), "this batch was")
        kw = dict(beam_size=beam_size, hotwords=hotwords, hotword_boost=hotword_boost, lm=lm, lm_weight=lm_weight, word_bonus=word_bonus)
        return self._with_f32_fallback(lambda: self.collect_batch(self.launch_batch(wav, lengths, **kw), word_timestamps), "this batch was")

    # ---- N-best: the best hypotheses of the final beam instead of the best one (gam_ctc_beam_nbest / gam_rnnt_beam_nbest)
    def _nbest_width(self, n_best: int, beam_size: Optional[int], hotwords, lm) -> int:
        """Check ``n_best`` against the search a ``transcribe_nbest`` call runs; its beam width.  Needs no device."""
        n_best = int(n_best)
        if not 1 <= n_best <= 32:
            raise ValueError(f"n_best {n_best} outside [1, 32]")
        dec = self.decoding
        if isinstance(dec, _decoding.CTCGreedyDecoding):
            width = max(8, n_best) if beam_size is None else int(beam_size)
            if not 1 <= width <= 32:
                raise ValueError(f"beam_size {width} outside [1, 32]")
            if n_best > width:
                raise ValueError(f"n_best {n_best} exceeds beam_size {width}")
            return width
        if beam_size is not None or hotwords is not None or lm is not None:
            raise TypeError("beam search needs a CTC head")       # (as transcribe: RNN-T heads take them through set_decoding)
        if not isinstance(dec, _decoding.RNNTBeamDecoding):
            raise ValueError("N-best needs a beam search: select one with set_decoding(beam_size=...)")
        if n_best > dec.beam_size:
            raise ValueError(f"n_best {n_best} exceeds the beam width {dec.beam_size} that set_decoding(beam_size=...) configured")
        return dec.beam_size

    @torch.inference_mode()
    def transcribe_nbest(self, wav_file: str, n_best: int = 5, word_timestamps: bool = False, *, beam_size: Optional[int] = None,
                         hotwords: Optional[Sequence[Union[str, List[int]]]] = None, hotword_boost: float = 2.0, lm=None,
                         lm_weight: float = 0.5, word_bonus: float = 1.0) -> NBestResult:
        """The ``n_best`` (1..32) best hypotheses of the beam search's final beam for a clip of at most 25 s, best first.  CTC heads:
        the options of ``transcribe``; ``beam_size`` defaults to max(8, ``n_best``) and must not be below ``n_best``.  RNN-T heads:
        the search ``set_decoding`` selected (a beam at least ``n_best`` wide; per-call options are a TypeError as in ``transcribe``).
        ``.best`` is what ``transcribe`` returns under the same options; the list can be shorter than ``n_best`` when the final beam
        holds fewer hypotheses."""
        self._nbest_width(n_best, beam_size, hotwords, lm)
        wav, length = self._prepare_wav_f32(wav_file)
        if length.item() > LONGFORM_THRESHOLD:
            raise ValueError("Too long wav file for transcribe_nbest (at most 25 s).")
        return self.transcribe_nbest_batch(wav, length, n_best, word_timestamps, beam_size=beam_size, hotwords=hotwords,
                                           hotword_boost=hotword_boost, lm=lm, lm_weight=lm_weight, word_bonus=word_bonus)[0]

    @torch.inference_mode()
    def transcribe_nbest_batch(self, wav: Tensor, lengths: Tensor, n_best: int = 5, word_timestamps: bool = False, *,
                               beam_size: Optional[int] = None, hotwords: Optional[Sequence[Union[str, List[int]]]] = None,
                               hotword_boost: float = 2.0, lm=None, lm_weight: float = 0.5, word_bonus: float = 1.0) -> List[NBestResult]:
        """Batched twin of ``transcribe_nbest`` on an already collated batch (wav [B,L] zero padded, len [B])."""
        width = self._nbest_width(n_best, beam_size, hotwords, lm)
        ctc = isinstance(self.decoding, _decoding.CTCGreedyDecoding)

        def run():
            encoded, encoded_len = self._encode_batch(wav, lengths)
            if ctc:
                dev = self.decoding.decode_nbest_device(self.head, encoded, encoded_len, int(n_best), width, hotwords, hotword_boost, lm,
                                                        lm_weight, word_bonus)
            else:
                dev = self.decoding.decode_nbest_device(self.head, encoded, encoded_len, int(n_best))
            return self.decoding.finish_nbest(dev), encoded_len

        rows, encoded_len = self._with_f32_fallback(run, "this batch was")
        out: List[NBestResult] = []
        shifts = None
        if word_timestamps:     # the frames_to_words call of _with_words, per hypothesis
            from .timestamps_utils import compute_frame_shift, frames_to_words
            wl, el = lengths.tolist(), encoded_len.tolist()
            shifts = [compute_frame_shift(int(w), int(e)) for w, e in zip(wl, el)]
        tok = self.decoding.tokenizer
        for b, hyps in enumerate(rows):
            post = nbest_posteriors([h[3] for h in hyps])
            out.append(NBestResult([Hypothesis(text=t, token_ids=i, token_frames=f, score=sc, logp=lp, posterior=post[r],
                                               words=frames_to_words(tok, i, f, shifts[b]) if word_timestamps else None)
                                    for r, (t, i, f, sc, lp) in enumerate(hyps)]))
        return out

    # ---- CTC forced alignment: a KNOWN transcript placed on the audio, and its log-likelihood (gam_ctc_align)
    def _require_ctc(self) -> None:
        if not isinstance(self.decoding, _decoding.CTCGreedyDecoding):
            raise TypeError("forced alignment needs a CTC head")

    @property
    def wildcard_id(self) -> int:
        """The token id of a wildcard in a forced-alignment target: V = the number of classes, one past blank."""
        self._require_ctc()
        return len(self.decoding.tokenizer) + 1

    def _wildcard_setup(self, texts, wildcard: Optional[str], wildcard_penalty: float):
        """(token-id lists, the penalty when wildcards are enabled else None) of an alignment; every error that needs no audio."""
        tok = self.decoding.tokenizer
        enabled = wildcard is not None or wildcard_penalty is not _wildcard.DEFAULT_PENALTY
        penalty = _wildcard.check(tok, wildcard, wildcard_penalty)
        wid = self.wildcard_id
        return [_wildcard.encode(tok, t, wildcard, wid, enabled) for t in texts], (penalty if enabled else None)

    @torch.inference_mode()
    def align(self, wav_file: str, text: Union[str, List[int]], wildcard: Optional[str] = None,
              wildcard_penalty: float = _wildcard.DEFAULT_PENALTY) -> AlignmentResult:
        """Align ``text`` (a string in the model's vocabulary, or token ids) to a clip of at most 25 s.  Words are built as
        ``transcribe(word_timestamps=True)`` builds them, from each token's first frame on the best path.  Raises ``ValueError``
        for a longer clip, for characters outside the vocabulary, or for a text that no alignment can fit into the clip.

        ``wildcard`` (a string the tokenizer cannot spell, e.g. ``"*"``): a PARTIAL transcript -- wherever it stands in ``text``,
        audio the transcript does not cover may pass; each wildcard takes at least one frame and comes back as a ``Gap`` in
        ``gaps``.  ``wildcard_penalty`` (>= 0, default ln 2): the price per frame a wildcard pays against the frame's best label.
        Token-id lists may hold ``model.wildcard_id`` when either keyword is given."""
        self._require_ctc()
        wav, length = self._prepare_wav_f32(wav_file)
        if length.item() > LONGFORM_THRESHOLD:
            raise ValueError("Too long wav file for forced alignment (at most 25 s).")
        res = self.align_batch(wav, length, [text], wildcard=wildcard, wildcard_penalty=wildcard_penalty)[0]
        if not res.feasible:
            raise ValueError(f"the text ({len(res.token_ids)} tokens) cannot be aligned to this audio: too long for it")
        return res

    @torch.inference_mode()
    def align_batch(self, wav: Tensor, lengths: Tensor, texts: Sequence[Union[str, List[int]]], wildcard: Optional[str] = None,
                    wildcard_penalty: float = _wildcard.DEFAULT_PENALTY) -> List[AlignmentResult]:
        """Batched ``align`` on a collated batch (wav [B,L] zero padded, len [B]); ``texts`` holds a ``str`` or token ids per
        utterance.  An utterance no alignment fits gets ``feasible=False`` (empty words, -inf scores) instead of an error.
        ``wildcard`` / ``wildcard_penalty``: as ``align``."""
        self._require_ctc()
        if len(texts) != wav.shape[0]:
            raise ValueError(f"{len(texts)} texts for a batch of {wav.shape[0]}")
        tok = self.decoding.tokenizer
        targets, penalty = self._wildcard_setup(texts, wildcard, wildcard_penalty)

        def run():
            encoded, encoded_len = self._encode_batch(wav, lengths)
            if penalty is None:
                return self.decoding.align(self.head, encoded, encoded_len, targets), encoded_len
            return self.decoding.align(self.head, encoded, encoded_len, targets, star_penalty=penalty), encoded_len

        rows, encoded_len = self._with_f32_fallback(run, "this batch was")
        from .timestamps_utils import compute_frame_shift, frames_to_words

        wl, el = lengths.tolist(), encoded_len.tolist()
        out: List[AlignmentResult] = []
        for i, (ids, first, last, score, loglik, ok) in enumerate(rows):
            if penalty is None:
                words = frames_to_words(tok, ids, first, compute_frame_shift(int(wl[i]), int(el[i]))) if ok else []
                out.append(AlignmentResult(text=tok.decode(ids), words=words, token_ids=ids, token_frames=first, score=score,
                                           log_likelihood=loglik, feasible=ok))
                continue
            wid = self.wildcard_id
            words, gaps = _wildcard.short_result(tok, ids, first, last, compute_frame_shift(int(wl[i]), int(el[i])), wid) if ok else ([], [])
            out.append(AlignmentResult(text=_wildcard.text_of(tok, ids, wid, wildcard), words=words, token_ids=ids, token_frames=first,
                                       score=score, log_likelihood=loglik, feasible=ok, gaps=gaps))
        return out

    # ---- keyword search: does a phrase occur, where, and how sure (gam_ctc_kws)
    def _keyword_setup(self, keywords, threshold, max_hits: int, limit: int = 64):
        """(token-id lists, their text, min_score f32 [K]) of a keyword search; every error that needs no audio is raised here.
        ``limit``: the most ``max_hits`` may be (64 per utterance or speech region, 4096 per file on the windowed route)."""
        if not isinstance(self.decoding, _decoding.CTCGreedyDecoding):
            raise TypeError("keyword search needs a CTC head")
        ids = self.decoding.keyword_ids(keywords)
        if not 1 <= int(max_hits) <= limit:
            raise ValueError(f"max_hits={max_hits} outside [1, {limit}]")
        tok = self.decoding.tokenizer
        texts = [w if isinstance(w, str) else tok.decode(i) for w, i in zip(keywords, ids)]
        return ids, texts, _decoding.keyword_min_scores([len(i) for i in ids], threshold)

    @torch.inference_mode()
    def find_keywords(self, wav_file: str, keywords: Sequence[Union[str, List[int]]], threshold=0.5, max_hits: int = 8) -> KeywordSearchResult:
        """Find every occurrence of each keyword in a clip of at most 25 s.  A keyword is a string in the model's vocabulary
        (``Tokenizer.encode``; nothing is normalised) or token ids, of at most 64 tokens; at most 4096 keywords per call.  An
        occurrence is a stretch of frames on which the keyword's tokens, with optional blanks and repeats, are at most a factor
        away from the greedy path: ``score`` is its log-likelihood ratio against that path (0 where the greedy path spells the
        keyword) and ``confidence`` = exp(score / tokens).  ``threshold`` in (0, 1] (one value or one per keyword) is the lowest
        confidence reported; the default 0.5 is a convention, not a measurement, and the confidence is uncalibrated.  At most
        ``max_hits`` (1..64) occurrences per keyword are returned, the earliest ones; ``truncated`` names the keywords that had more.

        In a char-wise vocabulary a keyword also matches INSIDE longer words; a space in the keyword is the vocabulary's " " token
        and enforces a word boundary there ("кот " does not match "котик").

        Raises ``ValueError`` for a longer clip, characters outside the vocabulary, an empty keyword or list, more than 64 tokens,
        more than 4096 keywords, a threshold outside (0, 1]; ``TypeError`` on RNN-T models."""
        self._keyword_setup(keywords, threshold, max_hits)
        wav, length = self._prepare_wav_f32(wav_file)
        if length.item() > LONGFORM_THRESHOLD:
            raise ValueError("Too long wav file for find_keywords (at most 25 s), use 'find_keywords_longform' method.")
        return self.find_keywords_batch(wav, length, keywords, threshold, max_hits)[0]

    @torch.inference_mode()
    def find_keywords_batch(self, wav: Tensor, lengths: Tensor, keywords: Sequence[Union[str, List[int]]], threshold=0.5,
                            max_hits: int = 8) -> List[KeywordSearchResult]:
        """Batched ``find_keywords`` on a collated batch (wav [B,L] zero padded, len [B]): every keyword is searched in every
        utterance, one result per utterance."""
        ids, texts, min_score = self._keyword_setup(keywords, threshold, max_hits)

        def run():
            encoded, encoded_len = self._encode_batch(wav, lengths)
            dec = self.decoding.find_keywords_device(self.head, encoded, encoded_len, ids, min_score, max_hits)
            return self.decoding.finish_keywords(dec), encoded_len

        h, encoded_len = self._with_f32_fallback(run, "this batch was")
        from .timestamps_utils import compute_frame_shift

        wl, el = lengths.tolist(), encoded_len.tolist()
        out: List[KeywordSearchResult] = []
        for b in range(wav.shape[0]):
            shift = compute_frame_shift(int(wl[b]), int(el[b])) if el[b] else 0.0
            hits, truncated = _decoding.keyword_hits(h, b, ids, texts, shift)
            out.append(KeywordSearchResult(hits=_decoding.sort_keyword_hits(hits), truncated=truncated, keywords=list(texts)))
        return out

    @torch.inference_mode()
    def find_keywords_longform(self, wav_file: str, keywords: Sequence[Union[str, List[int]]], threshold=0.5, max_hits: int = 8,
                               fr_batch_size: int = 16, **kwargs: Any) -> KeywordSearchResult:
        """``find_keywords`` on a recording of any length.  Segmentation keywords as for ``transcribe_longform`` (``speech_regions=``,
        ``vad=``, the pack_regions keywords; the same pyannote / EnergyVAD default and warnings).  Every speech region's chunk is
        searched as one batch entry; hits come in file time (region start + frame x that region's frame shift) with the region's
        index in ``segment`` and the frames counted inside it; ``max_hits`` and ``truncated`` apply per region.  An occurrence that
        straddles two regions is NOT found: the regions are searched independently and nothing is stitched.

        ``vad="windows"`` needs no speech detector and loses nothing at a cut: the recording is cut into overlapping windows
        (keywords ``chunk_length_s=20.0`` / ``stride_length_s=None`` as for ``transcribe_longform``; they belong to this route alone --
        without ``vad="windows"`` they go with the other keywords to the chunk packer, which refuses them as it always has, so such a
        call runs exactly what it ran before), their kept frames are stitched into ONE stream and the
        keywords are searched over that stream, batch by batch beside the next batch's encoder (``_find_keywords_windows``).  There
        ``max_hits`` (1..4096) and ``truncated`` count per keyword over the whole file; a hit's ``segment`` / ``end_segment`` are the
        windows its start and end frames were kept from, ``start_frame`` / ``end_frame`` the local frames inside those windows."""
        if self._windows_route(kwargs, ("chunk_length_s", "stride_length_s")):
            return self._find_keywords_windows(wav_file, keywords, threshold, max_hits, fr_batch_size, kwargs.get("chunk_length_s", 20.0),
                                               kwargs.get("stride_length_s"))
        from .feeder import BatchFeeder
        from .timestamps_utils import compute_frame_shift
        from .vad_utils import segment_audio_file

        ids, texts, min_score = self._keyword_setup(keywords, threshold, max_hits)
        self._default_vad(kwargs, "find_keywords_longform")
        segments, boundaries = segment_audio_file(wav_file, SAMPLE_RATE, device=self._device, **kwargs)
        if not segments:
            return KeywordSearchResult(hits=[], truncated=[], keywords=list(texts))

        # the one-batch pipeline of transcribe_longform: batch n is launched before batch n - 1 is brought to the host
        def run():
            hits, truncated, seg = [], set(), 0

            def emit(pending) -> None:
                nonlocal seg
                dec, encoded_len, lens = pending
                h = self.decoding.finish_keywords(dec)
                for b, (n_wav, n_enc) in enumerate(zip(lens.tolist(), encoded_len.tolist())):
                    shift = compute_frame_shift(int(n_wav), int(n_enc)) if n_enc else 0.0
                    got, trunc = _decoding.keyword_hits(h, b, ids, texts, shift, boundaries[seg][0], seg)
                    hits.extend(got)
                    truncated.update(trunc)
                    seg += 1

            def launch(n, batch):
                wav, lens = batch
                encoded, encoded_len = self._encode(wav, lens, getattr(feeder, "host_lengths", None))
                return self.decoding.find_keywords_device(self.head, encoded, encoded_len, ids, min_score, max_hits), encoded_len, lens

            feeder = BatchFeeder(segments, fr_batch_size, self._device)
            _pipeline(feeder, launch, emit)
            return _decoding.sort_keyword_hits(hits), sorted(truncated)

        hits, truncated = self._file_run(run)
        return KeywordSearchResult(hits=hits, truncated=truncated, keywords=list(texts))

    # ---- transducer forced alignment: the same for RNN-T heads (gam_rnnt_align)
    def _require_rnnt(self) -> None:
        if not isinstance(self.decoding, _decoding.RNNTGreedyDecoding):
            raise TypeError("transducer alignment needs an RNN-T head")

    @torch.inference_mode()
    def rnnt_align(self, wav_file: str, text: Union[str, List[int]]) -> AlignmentResult:
        """``align`` for RNN-T heads: place ``text`` (a string in the model's vocabulary, or token ids) on a clip of at most 25 s by
        transducer forced alignment.  ``token_frames`` are the frames at which the tokens are emitted on the best path, words are
        built from them as ``transcribe(word_timestamps=True)`` builds them; ``log_likelihood`` is log p(text | audio) over all
        alignments (= -rnnt_loss).  ``max_symbols_per_step`` does not bound the lattice, and the result does not depend on
        ``set_decoding``.  Raises ``ValueError`` for a longer clip, for characters outside the vocabulary, for more than 1024
        tokens, or for a text that no alignment can fit into the clip; ``TypeError`` on a CTC model."""
        self._require_rnnt()
        wav, length = self._prepare_wav_f32(wav_file)
        if length.item() > LONGFORM_THRESHOLD:
            raise ValueError("Too long wav file for forced alignment (at most 25 s).")
        res = self.rnnt_align_batch(wav, length, [text])[0]
        if not res.feasible:
            raise ValueError(f"the text ({len(res.token_ids)} tokens) cannot be aligned to this audio")
        return res

    @torch.inference_mode()
    def rnnt_align_batch(self, wav: Tensor, lengths: Tensor, texts: Sequence[Union[str, List[int]]]) -> List[AlignmentResult]:
        """Batched ``rnnt_align`` on a collated batch (wav [B,L] zero padded, len [B]); ``texts`` holds a ``str`` or token ids per
        utterance.  An utterance no alignment fits gets ``feasible=False`` (empty words, -inf scores) instead of an error."""
        self._require_rnnt()
        if len(texts) != wav.shape[0]:
            raise ValueError(f"{len(texts)} texts for a batch of {wav.shape[0]}")
        tok = self.decoding.tokenizer
        targets = [tok.encode(t) if isinstance(t, str) else [int(i) for i in t] for t in texts]

        def run():
            encoded, encoded_len = self._encode_batch(wav, lengths)
            return self.decoding.align(self.head, encoded, encoded_len, targets), encoded_len

        rows, encoded_len = self._with_f32_fallback(run, "this batch was")
        from .timestamps_utils import compute_frame_shift, frames_to_words

        wl, el = lengths.tolist(), encoded_len.tolist()
        out: List[AlignmentResult] = []
        for i, (ids, frames, score, loglik, ok) in enumerate(rows):
            words = frames_to_words(tok, ids, frames, compute_frame_shift(int(wl[i]), int(el[i]))) if ok else []
            out.append(AlignmentResult(text=tok.decode(ids), words=words, token_ids=ids, token_frames=frames, score=score,
                                       log_likelihood=loglik, feasible=ok))
        return out

    # ---- token / word / utterance confidence: a post-pass over a finished decode or alignment (gam_ctc_confidence / gam_rnnt_confidence)
    @torch.inference_mode()
    def confidence(self, wav_file: str, text: Optional[Union[str, List[int]]] = None, *, measure: str = "prob", aggregation: str = "mean",
                   beam_size: Optional[int] = None, hotwords: Optional[Sequence[Union[str, List[int]]]] = None,
                   hotword_boost: float = 2.0, lm=None, lm_weight: float = 0.5, word_bonus: float = 1.0) -> ConfidenceResult:
        """How sure the model is of each token and word of a clip of at most 25 s.  Without ``text`` the clip is decoded as
        ``transcribe`` decodes it (CTC: greedy, or beam search from the per-call options; RNN-T: what ``set_decoding`` selected --
        the per-call beam options are a ``TypeError`` there) and the decode is scored on the same encoder output.  With ``text`` (a
        string in the vocabulary, or token ids) the transcript is first placed by forced alignment (``align`` / ``rnnt_align``) and its
        tokens are scored at the aligned frames: the confidence of a KNOWN transcript (``ValueError`` if it cannot be aligned).
        ``measure``: "prob" -- p(token) under the distribution it was emitted from -- or "entropy" -- 1 - H / ln V;
        ``aggregation``: "mean" | "min" | "prod", over the frames of a CTC token's run, over the tokens of a word and over the
        utterance.  Every number lies in [0, 1]; none is calibrated."""
        HipEngine._confidence_codes(measure, aggregation)
        self._beam_width(beam_size, hotwords, lm)
        wav, length = self._prepare_wav_f32(wav_file)
        if length.item() > LONGFORM_THRESHOLD:
            raise ValueError("Too long wav file for confidence scoring (at most 25 s).")
        res = self.confidence_batch(wav, length, None if text is None else [text], measure=measure, aggregation=aggregation,
                                    beam_size=beam_size, hotwords=hotwords, hotword_boost=hotword_boost, lm=lm, lm_weight=lm_weight,
                                    word_bonus=word_bonus)[0]
        if not res.feasible:
            raise ValueError(f"the text ({len(res.token_ids)} tokens) cannot be aligned to this audio")
        return res

    @torch.inference_mode()
    def confidence_batch(self, wav: Tensor, lengths: Tensor, texts: Optional[Sequence[Union[str, List[int]]]] = None, *,
                         measure: str = "prob", aggregation: str = "mean", beam_size: Optional[int] = None,
                         hotwords: Optional[Sequence[Union[str, List[int]]]] = None, hotword_boost: float = 2.0, lm=None,
                         lm_weight: float = 0.5, word_bonus: float = 1.0) -> List[ConfidenceResult]:
        """Batched ``confidence`` on a collated batch (wav [B,L] zero padded, len [B]).  Text, token ids, token frames and word times
        are those of ``transcribe_batch(word_timestamps=True)`` (without ``texts``) or of ``align_batch`` / ``rnnt_align_batch`` (with
        ``texts``: a ``str`` or token ids per utterance; one that cannot be aligned gets ``feasible=False``).  ONE encoder run: the
        decode or the alignment and the confidence pass read the same encoder output."""
        m_code, a_code = HipEngine._confidence_codes(measure, aggregation)
        width = self._beam_width(beam_size, hotwords, lm)
        is_ctc = isinstance(self.decoding, _decoding.CTCGreedyDecoding)
        tok = self.decoding.tokenizer
        targets = None
        if texts is not None:
            if width is not None:
                raise ValueError("beam search options select a decode; they cannot be combined with a given text")
            if len(texts) != wav.shape[0]:
                raise ValueError(f"{len(texts)} texts for a batch of {wav.shape[0]}")
            targets = [tok.encode(t) if isinstance(t, str) else [int(i) for i in t] for t in texts]

        def run():
            encoded, encoded_len = self._encode_batch(wav, lengths)
            if targets is not None:
                rows = [(tok.decode(r[0]), r[0], r[1], r[-1]) for r in self.decoding.align(self.head, encoded, encoded_len, targets)]
            elif width is not None:
                dev_out = self.decoding.decode_beam_device(self.head, encoded, encoded_len, width, hotwords, hotword_boost, lm, lm_weight,
                                                           word_bonus)
                rows = [(t, i, f, True) for t, i, f in self.decoding.finish(dev_out)]
            else:
                rows = [(t, i, f, True) for t, i, f in self.decoding.finish(self.decoding.decode_device(self.head, encoded, encoded_len))]
            ids = [i if ok else [] for _, i, _, ok in rows]
            frames = [f if ok else [] for _, _, f, ok in rows]
            eng = self.head.engine
            if is_ctc:
                h = eng.ctc_confidence(encoded, encoded_len, ids, frames, measure=measure, aggregation=aggregation).host()
            else:
                h = eng.rnnt_confidence(encoded, encoded_len, ids, frames, measure=measure).host()
            _decoding.check_range(h["flag"])
            return rows, h, encoded_len

        rows, h, encoded_len = self._with_f32_fallback(run, "this batch was")
        from .timestamps_utils import aggregate_confidence, compute_frame_shift, frames_to_words, word_token_groups

        wl, el = lengths.tolist(), encoded_len.tolist()
        out: List[ConfidenceResult] = []
        for i, (text, ids, frames, ok) in enumerate(rows):
            if not ok:
                out.append(ConfidenceResult(text=text, words=[], token_ids=ids, token_frames=[], token_confidence=[], confidence=None,
                                            feasible=False))
                continue
            if not int(h["status"][i]):
                raise GigaAMHipError(f"confidence pass rejected the tokens of utterance {i}")
            conf = [float(c) for c in h["conf"][i, :len(ids)]]
            words = frames_to_words(tok, ids, frames, compute_frame_shift(int(wl[i]), int(el[i])))
            groups = word_token_groups(tok, ids)
            assert len(groups) == len(words)
            scored = [ScoredWord(text=w.text, start=w.start, end=w.end, confidence=aggregate_confidence([conf[k] for k in g], aggregation))
                      for w, g in zip(words, groups)]
            out.append(ConfidenceResult(text=text, words=scored, token_ids=ids, token_frames=frames, token_confidence=conf,
                                        confidence=aggregate_confidence(conf, aggregation), feasible=True))
        return out

    @staticmethod
    def _windows_route(kwargs: Dict[str, Any], allowed: Sequence[str] = (), refuse: bool = True) -> bool:
        """Whether the segmentation keywords of a longform call select ``vad="windows"``; the route takes none but ``allowed`` beside
        ``vad`` (``ValueError``, unless ``refuse`` is off: a caller with earlier errors to raise asks twice)."""
        if not (isinstance(kwargs.get("vad"), str) and kwargs["vad"] == "windows"):
            return False
        more = set(kwargs) - {"vad", *allowed}
        if more and refuse:
            raise ValueError(f'vad="windows" takes no segmentation keywords (got {sorted(more)}): there are no speech '
                             "regions to give or to pack")
        return True

    def _default_vad(self, kwargs: Dict[str, Any], what: str) -> None:
        """The segmentation keywords of the longform calls: ``vad="energy"`` becomes the EnergyVAD stand-in; with neither ``vad`` nor
        ``speech_regions`` the reference's pyannote pipeline is used when importable, else the stand-in, with a warning."""
        from .vad_utils import EnergyVAD

        if kwargs.get("vad") == "energy":   # stand-in detector on the HIP frontend (NOT pyannote)
            kwargs["vad"] = EnergyVAD(self.preprocessor)
        elif kwargs.get("vad") is None and kwargs.get("speech_regions") is None:
            # reference default: pyannote (model.py:212-216 -> vad_utils.py:100-101).  Without that optional
            # third-party package the call still works, on the labelled stand-in, and says so.
            try:
                import pyannote.audio  # noqa: F401
            except ImportError:
                import warnings
                warnings.warn(f"pyannote.audio is not installed: {what}() segments with gigaam_amd's "
                              "EnergyVAD stand-in instead of the reference's pyannote/segmentation-3.0 pipeline "
                              "(chunk boundaries will differ); pass speech_regions= or vad= to control segmentation",
                              RuntimeWarning, stacklevel=3)
                kwargs["vad"] = EnergyVAD(self.preprocessor)

    @torch.inference_mode()
    def transcribe_longform(self, wav_file: str, word_timestamps: bool = False, fr_batch_size: int = 16,
                            fr_num_workers: int = 0, *, beam_size: Optional[int] = None,
                            hotwords: Optional[Sequence[Union[str, List[int]]]] = None, hotword_boost: float = 2.0, lm=None,
                            lm_weight: float = 0.5, word_bonus: float = 1.0, chunk_length_s: float = 20.0,
                            stride_length_s: Optional[float] = None, pause_s: float = 1.0, max_segment_s: float = 22.0,
                            stream_search: bool = False, stream_decode: Union[bool, str] = False,
                            **kwargs: Any) -> LongformTranscriptionResult:
        """Segment -> zero-padded batches of ``fr_batch_size`` -> transcribe -> stitch
        (reference model.py:195-259).  The reference segments with pyannote's VAD
        (gated third-party model, not installable here); pass ``speech_regions=[(s,e),..]``,
        ``vad=callable(wav, sr) -> regions`` or ``vad="energy"`` (vad_utils.EnergyVAD, a labelled
        stand-in) and the reference's own chunk packer
        (vad_utils.pack_regions) does the rest.

        ``fr_num_workers`` is accepted for signature compatibility and ignored: the reference hands it to a
        ``DataLoader`` whose workers only run ``collate`` (model.py:219-229); here that role is the pinned,
        double-buffered ``feeder.BatchFeeder`` (one staging thread is enough to keep the GPU busy).

        ``beam_size`` / ``hotwords`` / ``hotword_boost`` / ``lm`` / ``lm_weight`` / ``word_bonus``: as for ``transcribe`` (CTC prefix
        beam search on every chunk; each chunk starts its own LM history at <s>).

        ``vad="windows"`` (CTC heads) needs no speech detector: the recording is cut into overlapping windows of ``chunk_length_s``
        seconds, ``stride_length_s`` seconds (default: a sixth of the chunk) at each inner window edge are dropped, and what is left is
        decoded as ONE utterance (``_transcribe_windows``); ``pause_s`` / ``max_segment_s`` cut its words into segments.  With
        ``stream_search=True`` and at least one of ``beam_size`` / ``hotwords`` / ``lm`` that utterance is decoded by the resumable
        beam search instead (``_transcribe_windows_beam``): the LM then sees the whole file as ONE history, <s> at its first frame
        and </s> at its end.

        ``vad="windows", stream_decode=True`` (RNN-T heads) is the same detector-free route for a transducer: the windows' encoder
        frames are stitched as the encoder half of the joint, and the resumable greedy kernel walks them in order, carrying its
        predictor state across the seams (``_transcribe_windows_rnnt``): the predictor sees the file as ONE history, where the
        speech-region route starts a new one per chunk.  It decodes greedily: beam options are errors.

        ``vad="windows", stream_decode="beam"`` walks the same stitched rows with the resumable beam search
        (``_transcribe_windows_rnnt_beam``) for a model that ``set_decoding(beam_size= / hotwords= / lm=)`` has put into beam mode:
        the width, the hotwords and the LM are the decoding object's; the predictor and the LM see the file as ONE history."""
        windows = self._windows_route(kwargs, refuse=False)
        search = beam_size is not None or hotwords is not None or lm is not None
        if stream_decode:      # (every error before any audio is read)
            if stream_search:
                raise ValueError("stream_search=True is the CTC heads' resumable beam search, stream_decode=True the RNN-T heads' resumable "
                                 "greedy decode: a call takes one of them")
            if not windows:
                raise ValueError('stream_decode=True decodes the stitched stream of vad="windows"; the other routes decode chunk by chunk')
            if not isinstance(self.decoding, _decoding.RNNTGreedyDecoding):
                raise TypeError("stream_decode needs an RNN-T head")
            self._beam_width(beam_size, hotwords, lm)      # (per-call beam options on an RNN-T model: the TypeError they always raise)
            if isinstance(stream_decode, str):
                if stream_decode != "beam":
                    raise ValueError(f'stream_decode={stream_decode!r}: True (the resumable greedy decode) or "beam" (the resumable beam search)')
                if not isinstance(self.decoding, _decoding.RNNTBeamDecoding):
                    raise ValueError('stream_decode="beam" needs a beam search: select one with set_decoding(beam_size=...)')
                self._windows_route(kwargs)
                return self._transcribe_windows_rnnt_beam(wav_file, word_timestamps, fr_batch_size, chunk_length_s, stride_length_s, pause_s,
                                                          max_segment_s)
            if isinstance(self.decoding, _decoding.RNNTBeamDecoding):
                raise ValueError("stream_decode=True decodes greedily: the RNN-T beam kernel stops at 8192 frames, so the beam decoding "
                                 "selected by set_decoding is not available over the stitched stream (set_decoding() selects greedy again)")
            self._windows_route(kwargs)
            return self._transcribe_windows_rnnt(wav_file, word_timestamps, fr_batch_size, chunk_length_s, stride_length_s, pause_s,
                                                 max_segment_s)
        if stream_search and not windows:
            raise ValueError('stream_search=True searches the stitched stream of vad="windows"; the other routes search chunk by chunk')
        if windows:
            if search and not stream_search:
                raise ValueError('vad="windows" decodes greedily: the beam kernel stops at 8192 frames, so beam_size / hotwords / lm over '
                                 "the stitched stream are not available without stream_search=True (the resumable beam search)")
            if stream_search and not search:
                raise ValueError("stream_search=True needs beam_size, hotwords or lm: there is nothing to search with")
            self._windows_route(kwargs)
            if stream_search:
                return self._transcribe_windows_beam(wav_file, word_timestamps, fr_batch_size, chunk_length_s, stride_length_s, pause_s,
                                                     max_segment_s, beam_size, hotwords, hotword_boost, lm, lm_weight, word_bonus)
            return self._transcribe_windows(wav_file, word_timestamps, fr_batch_size, chunk_length_s, stride_length_s, pause_s,
                                            max_segment_s)
        from .vad_utils import segment_audio_file

        beam_kw = {} if self._beam_width(beam_size, hotwords, lm) is None else dict(beam_size=beam_size, hotwords=hotwords,
                                                                                     hotword_boost=hotword_boost, lm=lm,
                                                                                     lm_weight=lm_weight, word_bonus=word_bonus)

        self._default_vad(kwargs, "transcribe_longform")
        segments, boundaries = segment_audio_file(wav_file, SAMPLE_RATE, device=self._device, **kwargs)
        if not segments:
            return LongformTranscriptionResult(segments=[])
        from .feeder import BatchFeeder

        # One-batch software pipeline: the kernels of batch n are launched (launch_batch: no host sync) BEFORE the
        # decoded ids of batch n-1 are copied back and detokenised (collect_batch), so the D2H wait, the tokenizer and
        # the feeder's staging of the next batch all run while the GPU works.  (The reference syncs per batch:
        # model.py:230-236.)  The range flag of the split-fp16 GEMMs rides on each batch's counts copy; if it ever
        # fires, the file is redone on the fp32 path.
        def run() -> List[Segment]:
            result: List[Segment] = []

            def emit(handle) -> None:
                for text, words in self.collect_batch(handle, word_timestamps):
                    start, end = boundaries[len(result)]
                    if word_timestamps:
                        shifted = [Word(text=w.text, start=round(w.start + start, 3), end=round(w.end + start, 3)) for w in words or []]
                        result.append(Segment(text=text, start=start, end=end, words=shifted))
                    else:
                        result.append(Segment(text=text, start=start, end=end))

            n_batches = (len(segments) + fr_batch_size - 1) // fr_batch_size
            feeder = BatchFeeder(segments, fr_batch_size, self._device)                           # pinned, double-buffered H2D
            _pipeline(feeder, lambda n, batch: self.launch_batch(*batch, overlap=n + 1 < n_batches,      # (RNN-T: decode n beside encoder n+1)
                                                                 host_lengths=getattr(feeder, "host_lengths", None), **beam_kw), emit)
            return result

        return LongformTranscriptionResult(segments=self._file_run(run))

    # ---- longform without a speech detector: overlapping windows stitched on the device (windows.py, gam_stitch.h)
    def _plan_windows(self, wav_file: str, chunk_length_s: float, stride_length_s: Optional[float], rnnt: bool = False):
        """(the file's samples as one CPU tensor, the window plan): every error that needs no GPU work is raised here.  ``rnnt``: the
        caller stitches encoder frames for an RNN-T head (``_transcribe_windows_rnnt``) and has made its own head check."""
        from .windows import plan_windows

        if not rnnt and not isinstance(self.decoding, _decoding.CTCGreedyDecoding):
            raise TypeError("windowed longform needs a CTC head")
        eng = self.head.engine
        audio = load_audio(wav_file, SAMPLE_RATE)
        frame_samples = int(eng.cfg.hop_length) * int(eng.cfg.subsampling_factor)
        return audio, plan_windows(int(audio.shape[0]), frame_samples, lambda n: eng.enc_frames(eng.feat_frames(n)), chunk_length_s,
                                   stride_length_s, SAMPLE_RATE)

    def _stitched_log_probs(self, audio: Tensor, plan, fr_batch_size: int, after_batch: Optional[Callable[[Tensor], None]] = None,
                            head: Optional[Tuple[Callable[[Tensor], Tensor], int]] = None) -> Tuple[Tensor, Tensor]:
        """The windows of ``plan`` (views of ``audio``) through the feeder, the encoder (packed rows: host lengths) and the CTC head,
        batch by batch; each batch's kept frames go straight into one preallocated [T_total, V] buffer (gam_op_ctc_stitch).  The window
        tables are uploaded once, nothing is read back.  Returns (the stream, the stitch statuses i32 [windows]), both on the device.
        ``after_batch(rows)``: called behind each batch's stitch with the rows of the stream that batch added (a view; they are
        contiguous: from the ``dst`` of its first window to the end of its last).  ``head``: (what makes a batch's rows
        [B, T', width] from its encoder output, their width) where they are not the CTC head's log-probs -- the encoder frames are the
        same for either head, only the rows are head-specific (``_transcribe_windows_rnnt``: ``rnnt_encp``, joint_hidden; the stitch
        copies rows of any width)."""
        from .feeder import BatchFeeder

        eng, dev, ws = self.head.engine, self._device, plan.windows
        lo = torch.tensor([w.lo for w in ws], dtype=torch.int32).to(dev)
        hi = torch.tensor([w.hi for w in ws], dtype=torch.int32).to(dev)
        dst = torch.tensor([w.dst for w in ws], dtype=torch.int64).to(dev)
        rows_of, width = (eng.ctc_head, int(eng.cfg.num_classes)) if head is None else head
        out = torch.empty((plan.t_total, width), dtype=torch.float32, device=dev)
        status: List[Tensor] = []
        feeder = BatchFeeder([audio[w.start:w.stop] for w in ws], fr_batch_size, dev)
        o = 0
        for wav, lens in feeder:
            b = wav.shape[0]
            encoded, encoded_len = self._encode(wav, lens, getattr(feeder, "host_lengths", None))
            status.append(eng.op_ctc_stitch(rows_of(encoded), encoded_len, lo[o:o + b], hi[o:o + b], dst[o:o + b], out))
            if after_batch is not None:
                after_batch(out[ws[o].dst:ws[o + b - 1].dst + ws[o + b - 1].hi - ws[o + b - 1].lo])
            o += b
        return out, torch.cat(status)

    @staticmethod
    def _check_stitch(status: Tensor) -> None:
        if not bool(status.cpu().all()):
            raise GigaAMHipError("windowed longform: the host length formula and the device disagree on a window's encoder frames "
                                 f"(stitch statuses {status.cpu().tolist()})")

    def _windows_run(self, audio: Tensor, plan, fr_batch_size: int, whole: Optional[Callable[[Tensor], Dict[str, Any]]] = None,
                     stream=None, overlap: bool = False, ended: Optional[Callable[[Tensor, Any], Dict[str, Any]]] = None,
                     head: Optional[Tuple[Callable[[Tensor], Tensor], int]] = None) -> Dict[str, Any]:
        """One pass of a windowed route over the stitched stream of ``plan`` -> its result on the host.  Either ``whole(stream)`` -- a
        one-shot op on the finished [T_total, V] stream, brought to the host (a dict with ``flag``) -- or ``stream``, a resumable
        search (engine.KeywordStream / BeamStream): ONE push of the rows each batch added behind that batch's stitch (``overlap``: on
        the decode side stream, beside the next batch's frontend and encoder), then the END call and ONE collect -- or, with ``ended``,
        ``ended(stream, result)``: a pass over the finished stream that reads the search's result on the device, and brings both to
        the host.  ``head``: as ``_stitched_log_probs``.  Raises decoding.RangeOverflow on the flag, then checks the stitch statuses."""
        if stream is None:
            lp_all, status = self._stitched_log_probs(audio, plan, fr_batch_size, head=head)
            h = whole(lp_all)
        else:
            lp_all, status = self._stitched_log_probs(audio, plan, fr_batch_size, lambda rows: stream.push(rows, overlap=overlap), head=head)
            out = stream.finish(consume_flag=True)
            h = out.host() if ended is None else ended(lp_all, out)
        _decoding.check_range(h["flag"])
        self._check_stitch(status)
        return h

    def _transcribe_windows(self, wav_file: str, word_timestamps: bool, fr_batch_size: int, chunk_length_s: float,
                            stride_length_s: Optional[float], pause_s: float, max_segment_s: float) -> LongformTranscriptionResult:
        """``transcribe_longform(vad="windows")``: plan -> stitched log-probs -> gam_op_ctc_greedy_long -> ONE collect.  Words follow
        ``frames_to_words``' rule on file times (each time taken in the window its frame was kept from, rounded to 3 decimals);
        segments are runs of words (windows.segment_words).  The defaults of ``stride_length_s``, ``pause_s`` and ``max_segment_s``
        are conventions, not measurements."""
        audio, plan = self._plan_windows(wav_file, chunk_length_s, stride_length_s)
        if not plan.windows:
            return LongformTranscriptionResult(segments=[])
        eng = self.head.engine

        def greedy(lp_all: Tensor) -> Dict[str, Any]:
            rows, flag = HipEngine.collect(eng.op_ctc_greedy_long(lp_all, consume_flag=True))
            return {"rows": rows[0], "flag": flag}

        ids, frames = self._file_run(lambda: self._windows_run(audio, plan, fr_batch_size, greedy)["rows"])
        return self._windows_result(plan, ids, frames, word_timestamps, pause_s, max_segment_s)

    def _windows_result(self, plan, ids: List[int], frames: List[int], word_timestamps: bool, pause_s: float,
                        max_segment_s: float) -> LongformTranscriptionResult:
        """Token ids and their frames of the stitched stream of ``plan`` -> words on file times -> segments."""
        from .timestamps_utils import longform_words
        from .windows import segment_words

        wins, local, _ = plan.locate(frames)
        words, _ = longform_words(self.decoding.tokenizer, ids, wins, local, [(w.start_s, w.start_s) for w in plan.windows],
                                  [w.shift for w in plan.windows])
        return LongformTranscriptionResult(segments=[
            Segment(text=" ".join(w.text for w in run_), start=run_[0].start, end=run_[-1].end, words=run_ if word_timestamps else None)
            for run_ in segment_words(words, pause_s, max_segment_s)])

    def _transcribe_windows_beam(self, wav_file: str, word_timestamps: bool, fr_batch_size: int, chunk_length_s: float,
                                 stride_length_s: Optional[float], pause_s: float, max_segment_s: float, beam_size: Optional[int],
                                 hotwords, hotword_boost: float, lm, lm_weight: float, word_bonus: float) -> LongformTranscriptionResult:
        """``transcribe_longform(vad="windows", stream_search=True)``: the plan and the stitch of ``_transcribe_windows``; behind each
        batch's stitch ONE push of the rows that batch added into a resumable beam search (engine.BeamStream, gam_op_ctc_beam_stream)
        -- on the decode side stream, so that batch n's search runs beside batch n + 1's frontend and encoder
        (GAM_BEAM_STREAM_OVERLAP=0: on the launch stream, the A/B switch) --, then the END call and ONE collect.  The hotwords and
        the LM are set as ``transcribe`` sets them; the LM's history is the whole file's."""
        audio, plan = self._plan_windows(wav_file, chunk_length_s, stride_length_s)
        width = self._beam_width(beam_size, hotwords, lm)
        if not 1 <= width <= HipEngine.MAX_BEAM:
            raise ValueError(f"beam_size {width} outside [1, {HipEngine.MAX_BEAM}]")
        if not plan.windows:
            return LongformTranscriptionResult(segments=[])
        eng, dec = self.head.engine, self.decoding
        overlap = os.environ.get("GAM_BEAM_STREAM_OVERLAP", "1") != "0"

        def run():      # (a rerun under GAM_GEMM_F32 comes here again: a new stream, BEGIN)
            eng.set_hotwords(dec.hotword_ids(hotwords), hotword_boost)
            eng.set_lm(dec.language_model(lm), dec.tokenizer, lm_weight, word_bonus)
            h = self._windows_run(audio, plan, fr_batch_size, stream=eng.beam_stream(width, plan.t_total), overlap=overlap)
            return h["ids"].tolist(), h["frames"].tolist()

        ids, frames = self._file_run(run)
        return self._windows_result(plan, ids, frames, word_timestamps, pause_s, max_segment_s)

    def _transcribe_windows_rnnt(self, wav_file: str, word_timestamps: bool, fr_batch_size: int, chunk_length_s: float,
                                 stride_length_s: Optional[float], pause_s: float, max_segment_s: float) -> LongformTranscriptionResult:
        """``transcribe_longform(vad="windows", stream_decode=True)`` on an RNN-T head: the plan of ``_transcribe_windows``; each feeder
        batch goes through the encoder and the encoder half of the joint (``rnnt_encp``), and its kept frames are stitched into one
        [T_total, joint_hidden] buffer; behind each batch's stitch ONE push of the rows that batch added into a resumable greedy decode
        (engine.RnntGreedyStream, gam_op_rnnt_greedy_stream) -- on the decode side stream, so that batch n's decode runs beside batch
        n + 1's frontend and encoder (GAM_RNNT_STREAM_OVERLAP=0: on the launch stream, the A/B switch) --, then the END call and ONE
        collect.  The predictor's state crosses the seams: the file is ONE history.  Words follow ``_windows_result``'s rule; a frame
        may carry several tokens (up to max_symbols_per_step), which then share its time."""
        audio, plan = self._plan_windows(wav_file, chunk_length_s, stride_length_s, rnnt=True)
        if not plan.windows:
            return LongformTranscriptionResult(segments=[])
        eng = self.head.engine
        overlap = os.environ.get("GAM_RNNT_STREAM_OVERLAP", "1") != "0"

        def run():      # (a rerun under GAM_GEMM_F32 comes here again: a new stream, BEGIN)
            stream = eng.rnnt_greedy_stream(plan.t_total, int(self.decoding.max_symbols))

            def ended(_, out) -> Dict[str, Any]:
                rows, flag = HipEngine.collect(out)
                stream.check()
                return {"rows": rows[0], "flag": flag}

            return self._windows_run(audio, plan, fr_batch_size, stream=stream, overlap=overlap, ended=ended,
                                     head=(eng.rnnt_encp, int(eng.cfg.joint_hidden)))["rows"]

        ids, frames = self._file_run(run)
        return self._windows_result(plan, ids, frames, word_timestamps, pause_s, max_segment_s)

    def _transcribe_windows_rnnt_beam(self, wav_file: str, word_timestamps: bool, fr_batch_size: int, chunk_length_s: float,
                                      stride_length_s: Optional[float], pause_s: float, max_segment_s: float) -> LongformTranscriptionResult:
        """``transcribe_longform(vad="windows", stream_decode="beam")`` on an RNN-T head in beam mode (``set_decoding``): the plan,
        the stitch and the pushes of ``_transcribe_windows_rnnt`` into a resumable beam search (engine.RnntBeamStream,
        gam_op_rnnt_beam_stream) with the decoding object's width, hotwords and LM, set as the RNN-T ``transcribe`` sets them
        (GAM_RNNT_STREAM_OVERLAP=0: pushes on the launch stream, the A/B switch); then the END call and ONE collect.  The predictor
        and the LM see the file as ONE history: <s> at its first frame, </s> at its end."""
        audio, plan = self._plan_windows(wav_file, chunk_length_s, stride_length_s, rnnt=True)
        if not plan.windows:
            return LongformTranscriptionResult(segments=[])
        eng, dec = self.head.engine, self.decoding
        overlap = os.environ.get("GAM_RNNT_STREAM_OVERLAP", "1") != "0"

        def run():      # (a rerun under GAM_GEMM_F32 comes here again: a new stream, BEGIN)
            eng.set_hotwords(dec.hotword_ids(dec.hotwords), dec.hotword_boost)
            eng.set_lm(dec.lm, dec.tokenizer, dec.lm_weight, dec.word_bonus)
            h = self._windows_run(audio, plan, fr_batch_size, stream=eng.rnnt_beam_stream(dec.beam_size, plan.t_total, int(dec.max_symbols)),
                                  overlap=overlap, head=(eng.rnnt_encp, int(eng.cfg.joint_hidden)))
            return h["ids"].tolist(), h["frames"].tolist()

        ids, frames = self._file_run(run)
        return self._windows_result(plan, ids, frames, word_timestamps, pause_s, max_segment_s)

    def _find_keywords_windows(self, wav_file: str, keywords, threshold, max_hits: int, fr_batch_size: int, chunk_length_s: float,
                               stride_length_s: Optional[float]) -> KeywordSearchResult:
        """``find_keywords_longform(vad="windows")``: the plan and the stitch of ``_transcribe_windows``; behind each batch's stitch ONE
        push of the rows that batch added into a resumable search (engine.KeywordStream, gam_op_ctc_kws_stream) -- on the decode side
        stream, so that batch n's search runs beside batch n + 1's frontend and encoder (GAM_KWS_STREAM_OVERLAP=0: on the launch
        stream, the A/B switch) --, then the END call and ONE collect."""
        eng_max = HipEngine.MAX_KEYWORD_STREAM_HITS
        ids, texts, min_score = self._keyword_setup(keywords, threshold, max_hits, eng_max)
        audio, plan = self._plan_windows(wav_file, chunk_length_s, stride_length_s)
        if not plan.windows:
            return KeywordSearchResult(hits=[], truncated=[], keywords=list(texts))
        eng = self.head.engine
        overlap = os.environ.get("GAM_KWS_STREAM_OVERLAP", "1") != "0"

        def run():      # (a rerun under GAM_GEMM_F32 comes here again: a new stream, BEGIN)
            eng.set_keywords(ids, min_score)
            return self._windows_run(audio, plan, fr_batch_size, stream=eng.kws_stream(int(max_hits)), overlap=overlap)

        hits, truncated = _decoding.keyword_stream_hits(self._file_run(run), ids, texts, plan)
        return KeywordSearchResult(hits=_decoding.sort_keyword_hits(hits), truncated=truncated, keywords=list(texts))

    # ---- forced alignment of a whole recording: one stream, two ways to produce it (speech regions / windows), one tail
    def _align_long_setup(self, text: Union[str, List[int]], wildcard: Optional[str], wildcard_penalty: float):
        """(token ids, the penalty when wildcards are enabled else None, the result's text) of ``align_longform``: every error
        that needs no audio."""
        (ids,), penalty = self._wildcard_setup([text], wildcard, wildcard_penalty)
        tok = self.decoding.tokenizer
        return ids, penalty, (tok.decode(ids) if penalty is None else _wildcard.text_of(tok, ids, self.wildcard_id, wildcard))

    def _align_stream(self, lp_all: Tensor, ids: List[int], penalty: Optional[float]) -> Dict[str, Any]:
        """gam_op_ctc_align_long of ``ids`` on a finished [T_total, V] stream (wildcards enabled: with its star row) -> the host dict."""
        eng = self.head.engine
        star = None if penalty is None else eng.ctc_star_row(lp_all, None, penalty)
        return eng.op_ctc_align_long(lp_all, ids, consume_flag=True, star=star).host()

    def _align_long_result(self, ids: List[int], penalty: Optional[float], text_out: str, nothing: Optional[str],
                           run: Optional[Callable[[], tuple]]) -> LongformAlignmentResult:
        """The tail of ``align_longform`` on either route.  ``nothing``: set when there is no frame to align to (it says why) -- an
        empty text then aligns trivially, any other is an error.  Else ``run()`` (under ``_file_run``) produces the stream, aligns it
        and returns (the host dict of ``op_ctc_align_long``, what the text is too long for when it does not fit, ``locate(stream
        frames) -> (segments, local frames, times)``, the segments' time origins, their frame shifts, the time spans that re-time the
        segments or None)."""
        from .timestamps_utils import longform_words

        tok, wid = self.decoding.tokenizer, self.wildcard_id
        if nothing is not None:
            if ids:
                raise ValueError(f"{nothing}: the text ({len(ids)} tokens) cannot be aligned to it")
            return LongformAlignmentResult(text=text_out, words=[], token_ids=ids, token_segments=[], token_frames=[], token_times=[],
                                           score=0.0, log_likelihood=0.0, segments=[], feasible=True)
        try:
            h, too_long_for, locate, origins, shifts, spans = self._file_run(run)
        except GigaAMHipError as e:
            if "gam_set_ctc_align_workspace" in str(e):
                raise ValueError(f"the alignment lattice does not fit the workspace cap: {e}") from e
            raise
        if not h["status"]:
            raise ValueError(f"the text ({len(ids)} tokens) cannot be aligned to this audio: too long for {too_long_for}")
        token_segments, token_frames, token_times = locate(h["tok_first"].tolist())
        more = {}
        if penalty is None:
            words, segs = longform_words(tok, ids, token_segments, token_frames, origins, shifts)
        else:
            last_segments, last_frames, _ = locate(h["tok_last"].tolist())
            words, segs, more["gaps"] = _wildcard.longform_result(tok, ids, token_segments, token_frames, last_segments, last_frames,
                                                                  origins, shifts, wid)
        if spans is not None:
            segs = [Segment(text=sg.text, start=a, end=b, words=sg.words) for sg, (a, b) in zip(segs, spans)]
        return LongformAlignmentResult(text=text_out, words=words, token_ids=ids, token_segments=token_segments,
                                       token_frames=token_frames, token_times=token_times, score=h["score"],
                                       log_likelihood=h["loglik"], segments=segs, feasible=True, **more)

    def _align_windows(self, wav_file: str, text: Union[str, List[int]], fr_batch_size: int, wildcard: Optional[str],
                       wildcard_penalty: float, chunk_length_s: float, stride_length_s: Optional[float],
                       align: Optional[Callable[[Tensor, List[int], Optional[float]], Dict[str, Any]]] = None) -> LongformAlignmentResult:
        """``align_longform(vad="windows")``: the same plan and the same stitch, then gam_op_ctc_align_long on the stream.  A token's
        segment is the window its frame was kept from, its frame the local frame inside that window; ``segments`` holds one Segment
        per window over the time span of its kept frames (they tile the file) with the words that start there.  ``align``: what aligns
        the finished stream in place of ``_align_stream`` (``confidence_longform``: the alignment and the confidence pass behind it)."""
        align = align or self._align_stream
        if not isinstance(self.decoding, _decoding.CTCGreedyDecoding):
            raise TypeError("windowed longform needs a CTC head")
        ids, penalty, text_out = self._align_long_setup(text, wildcard, wildcard_penalty)
        audio, plan = self._plan_windows(wav_file, chunk_length_s, stride_length_s)
        if not plan.windows:
            return self._align_long_result(ids, penalty, text_out, "the recording holds no encoder frame", None)

        def run():
            h = self._windows_run(audio, plan, fr_batch_size, lambda lp_all: align(lp_all, ids, penalty))
            origins = [(w.start_s, w.start_s) for w in plan.windows]      # a local frame's time counts from its window's start
            return (h, f"its {plan.t_total} frames", plan.locate, origins, [w.shift for w in plan.windows],
                    [(round(a, 3), round(b, 3)) for a, b in plan.spans()])

        return self._align_long_result(ids, penalty, text_out, None, run)

    @torch.inference_mode()
    def align_longform(self, wav_file: str, text: Union[str, List[int]], fr_batch_size: int = 16, wildcard: Optional[str] = None,
                       wildcard_penalty: float = _wildcard.DEFAULT_PENALTY, chunk_length_s: float = 20.0,
                       stride_length_s: Optional[float] = None, **kwargs: Any) -> LongformAlignmentResult:
        """Align ``text`` (a string in the model's vocabulary, or token ids) to a recording of any length: forced alignment of the
        WHOLE text against the WHOLE recording (``align`` stops at 25 s and 1024 tokens).  Segmentation keywords as for
        ``transcribe_longform`` (``speech_regions=``, ``vad=``, the pack_regions keywords; the same pyannote / EnergyVAD default).

        The speech regions are encoded in batches of ``fr_batch_size``; the CTC log-probs of every region's valid frames are
        concatenated on the device into one [T_total, V] utterance, which gam_op_ctc_align_long aligns in one go.  So: the
        concatenated speech frames are ONE CTC utterance -- where the text splits between the regions is found by the alignment,
        not given; a token's run may continue across a region boundary; nothing can be placed in non-speech.  A token's time is
        its region's start + its frame inside the region x that region's frame shift; words follow the rule of
        ``transcribe(word_timestamps=True)`` on those file times.

        ``wildcard`` / ``wildcard_penalty``: as ``align`` -- a partial transcript; each wildcard comes back as a ``Gap`` in ``gaps``
        (file times; it may start in one speech region and end in another: ``segment`` / ``end_segment``), and no word spans a gap.

        Raises ``ValueError`` for characters outside the vocabulary, for a text that no alignment fits into the speech found, for a
        non-empty text when no speech was found, and for a lattice beyond the workspace cap (the message carries the needed and
        the allowed bytes; ``HipEngine.set_ctc_align_workspace`` / GAM_CTC_ALIGN_WS raise it); ``TypeError`` on RNN-T models.

        ``vad="windows"``: no speech detector -- the whole recording as overlapping windows of ``chunk_length_s`` / ``stride_length_s``
        (as ``transcribe_longform``), stitched into one stream and aligned in one go (``_align_windows``): a token's segment is then
        the window its frame was kept from, and ``segments`` tile the file."""
        if self._windows_route(kwargs):
            return self._align_windows(wav_file, text, fr_batch_size, wildcard, wildcard_penalty, chunk_length_s, stride_length_s)
        return self._align_regions(wav_file, text, fr_batch_size, wildcard, wildcard_penalty, kwargs)

    def _align_regions(self, wav_file: str, text: Union[str, List[int]], fr_batch_size: int, wildcard: Optional[str], wildcard_penalty: float,
                       kwargs: Dict[str, Any],
                       align: Optional[Callable[[Tensor, List[int], Optional[float]], Dict[str, Any]]] = None) -> LongformAlignmentResult:
        """``align_longform`` over speech regions (its docstring); ``align``: as ``_align_windows``."""
        align = align or self._align_stream
        from .feeder import BatchFeeder
        from .timestamps_utils import compute_frame_shift, concat_frames_to_segments
        from .vad_utils import segment_audio_file

        self._require_ctc()
        ids, penalty, text_out = self._align_long_setup(text, wildcard, wildcard_penalty)
        self._default_vad(kwargs, "align_longform")
        segments, boundaries = segment_audio_file(wav_file, SAMPLE_RATE, device=self._device, **kwargs)
        if not segments:
            return self._align_long_result(ids, penalty, text_out, "no speech found in the recording", None)
        eng = self.head.engine

        def run():
            rows: List[Tensor] = []
            seg_frames: List[Tensor] = []
            feeder = BatchFeeder(segments, fr_batch_size, self._device)
            for wav, lens in feeder:
                encoded, encoded_len = self._encode(wav, lens, getattr(feeder, "host_lengths", None))
                lp = eng.ctc_head(encoded)                                         # [B, T', V] log-probs, on the device
                valid = torch.arange(lp.shape[1], device=lp.device)[None, :] < encoded_len[:, None]
                rows.append(lp[valid])                                             # each utterance's valid rows, utterance after utterance
                seg_frames.append(encoded_len)
            h = align(torch.cat(rows, dim=0), ids, penalty)
            _decoding.check_range(h["flag"])
            n = torch.cat(seg_frames).tolist()
            shifts = [compute_frame_shift(int(seg.shape[0]), int(k)) if k else 0.0 for seg, k in zip(segments, n)]
            starts = [b[0] for b in boundaries]
            return (h, f"the speech found ({sum(n)} frames)", lambda frames: concat_frames_to_segments(frames, n, starts, shifts),
                    boundaries, shifts, None)

        return self._align_long_result(ids, penalty, text_out, None, run)

    # ---- token / word / segment confidence over a whole recording (gam_op_ctc_confidence_long; per chunk: the batch passes)
    @torch.inference_mode()
    def confidence_longform(self, wav_file: str, text: Optional[Union[str, List[int]]] = None, *, measure: str = "prob",
                            aggregation: str = "mean", fr_batch_size: int = 16, wildcard: Optional[str] = None,
                            wildcard_penalty: float = _wildcard.DEFAULT_PENALTY, beam_size: Optional[int] = None,
                            hotwords: Optional[Sequence[Union[str, List[int]]]] = None, hotword_boost: float = 2.0, lm=None,
                            lm_weight: float = 0.5, word_bonus: float = 1.0, stream_search: bool = False, chunk_length_s: float = 20.0,
                            stride_length_s: Optional[float] = None, pause_s: float = 1.0, max_segment_s: float = 22.0,
                            **kwargs: Any) -> LongformConfidenceResult:
        """``confidence`` on a recording of any length: how sure the model is of each token, word and segment.  Words (text, start,
        end), segments, token ids, ``token_segments`` / ``token_frames`` / ``token_times`` and gaps are exactly those of
        ``transcribe_longform(..., word_timestamps=True)`` (without ``text``) or of ``align_longform(...)`` (with ``text``: a KNOWN,
        with ``wildcard=`` partial, transcript) under the same arguments; confidence only adds numbers.  ``measure`` /
        ``aggregation``: as ``confidence``; a wildcard belongs to no word, has ``token_confidence`` None and is left out of every
        aggregate.  Segmentation keywords, ``chunk_length_s`` / ``stride_length_s`` / ``pause_s`` / ``max_segment_s``, the beam keywords
        and ``stream_search``: as ``transcribe_longform``; ``wildcard`` / ``wildcard_penalty``: as ``align_longform``.

        ``vad="windows"`` (CTC heads): the stitched stream is decoded greedily (gam_op_ctc_greedy_long), searched
        (``stream_search=True``: the resumable beam search) or aligned (``text``), and ONE pass over the whole stream
        (gam_op_ctc_confidence_long) scores the tokens where the decode or the alignment left them on the device.  Speech regions with
        ``text`` (CTC heads): the concatenated region stream of ``align_longform``, aligned, then the same pass.  Speech regions
        without ``text`` (CTC and RNN-T heads): each feeder batch is decoded as ``transcribe_longform`` decodes it -- an RNN-T batch on
        the launch stream with full-size clusters, as ``confidence_batch`` decodes it -- and scored on the same encoder output by the
        batch pass of ``confidence_batch``.

        Raises ``ValueError`` for an unknown measure or aggregation (before any audio is read), for beam options together with
        ``text``, and whatever ``transcribe_longform`` / ``align_longform`` raise for the same arguments; ``TypeError`` for
        ``vad="windows"`` or ``text`` on an RNN-T model (there is no long transducer alignment) and for per-call beam options there;
        ``GigaAMHipError`` if the pass rejects the token list."""
        HipEngine._confidence_codes(measure, aggregation)
        search = beam_size is not None or hotwords is not None or lm is not None
        is_ctc = isinstance(self.decoding, _decoding.CTCGreedyDecoding)
        windows = self._windows_route(kwargs, refuse=False)
        if text is not None:
            if search or stream_search:
                raise ValueError("beam search options select a decode; they cannot be combined with a given text")
            if not is_ctc and not windows:
                raise TypeError("confidence_longform with a text needs a CTC head: there is no long transducer alignment")
            return self._confidence_long_text(wav_file, text, measure, aggregation, fr_batch_size, wildcard, wildcard_penalty,
                                              chunk_length_s, stride_length_s, kwargs)
        if wildcard is not None or wildcard_penalty is not _wildcard.DEFAULT_PENALTY:
            raise ValueError("wildcard / wildcard_penalty belong to a given text")
        if stream_search and not windows:
            raise ValueError('stream_search=True searches the stitched stream of vad="windows"; the other routes search chunk by chunk')
        if windows:
            if search and not stream_search:
                raise ValueError('vad="windows" decodes greedily: the beam kernel stops at 8192 frames, so beam_size / hotwords / lm over '
                                 "the stitched stream are not available without stream_search=True (the resumable beam search)")
            if stream_search and not search:
                raise ValueError("stream_search=True needs beam_size, hotwords or lm: there is nothing to search with")
            self._windows_route(kwargs)
            beam = (beam_size, hotwords, hotword_boost, lm, lm_weight, word_bonus) if stream_search else None
            return self._confidence_windows(wav_file, measure, aggregation, fr_batch_size, chunk_length_s, stride_length_s, pause_s,
                                            max_segment_s, beam)
        width = self._beam_width(beam_size, hotwords, lm)
        beam = None if width is None else (width, hotwords, hotword_boost, lm, lm_weight, word_bonus)
        return self._confidence_regions(wav_file, measure, aggregation, fr_batch_size, beam, kwargs)

    def _confidence_host(self, cf, n: int) -> List[float]:
        """The first ``n`` token confidences of a one-row ``engine.Confidence`` on the host; status 0 is an error."""
        h = cf.host()
        if not int(h["status"][0]):
            raise GigaAMHipError("the confidence pass rejected the token list of the recording")
        return [float(c) for c in h["conf"][0, :n]]

    def _confidence_windows(self, wav_file: str, measure: str, aggregation: str, fr_batch_size: int, chunk_length_s: float,
                            stride_length_s: Optional[float], pause_s: float, max_segment_s: float, beam) -> LongformConfidenceResult:
        """``confidence_longform(vad="windows")`` without text: the plan, the stitch and the decode of ``_transcribe_windows`` (``beam``:
        of ``_transcribe_windows_beam``), then gam_op_ctc_confidence_long on the stream the stitch left, fed by the decode's device
        result; the collects come after both."""
        from .timestamps_utils import score_longform

        audio, plan = self._plan_windows(wav_file, chunk_length_s, stride_length_s)
        eng, dec = self.head.engine, self.decoding
        if beam is not None:
            width = self._beam_width(beam[0], beam[1], beam[3])
            if not 1 <= width <= HipEngine.MAX_BEAM:
                raise ValueError(f"beam_size {width} outside [1, {HipEngine.MAX_BEAM}]")
        if not plan.windows:
            return LongformConfidenceResult(text="", segments=[], words=[], token_ids=[], token_segments=[], token_frames=[],
                                            token_times=[], token_confidence=[], confidence=None)

        def greedy(lp_all: Tensor) -> Dict[str, Any]:
            out = eng.op_ctc_greedy_long(lp_all, consume_flag=True)
            cf = eng.op_ctc_confidence_long(lp_all, out, measure=measure, aggregation=aggregation)
            rows, flag = HipEngine.collect(out)
            return {"ids": rows[0][0], "frames": rows[0][1], "flag": flag, "cf": cf}

        def searched(lp_all: Tensor, out) -> Dict[str, Any]:
            cf = eng.op_ctc_confidence_long(lp_all, out, measure=measure, aggregation=aggregation)
            h = out.host()
            return {"ids": h["ids"].tolist(), "frames": h["frames"].tolist(), "flag": h["flag"], "cf": cf}

        def run():
            if beam is None:
                h = self._windows_run(audio, plan, fr_batch_size, greedy)
            else:      # (a rerun under GAM_GEMM_F32 comes here again: a new stream, BEGIN)
                _, hotwords, hotword_boost, lm, lm_weight, word_bonus = beam
                eng.set_hotwords(dec.hotword_ids(hotwords), hotword_boost)
                eng.set_lm(dec.language_model(lm), dec.tokenizer, lm_weight, word_bonus)
                overlap = os.environ.get("GAM_BEAM_STREAM_OVERLAP", "1") != "0"
                h = self._windows_run(audio, plan, fr_batch_size, stream=eng.beam_stream(width, plan.t_total), overlap=overlap,
                                      ended=searched)
            return h["ids"], h["frames"], self._confidence_host(h["cf"], len(h["ids"]))

        ids, frames, conf = self._file_run(run)
        base = self._windows_result(plan, ids, frames, True, pause_s, max_segment_s)
        wins, local, times = plan.locate(frames)
        token_conf, words, segments, total = score_longform(dec.tokenizer, ids, conf, base.words, base.segments, aggregation)
        return LongformConfidenceResult(text=base.text, segments=segments, words=words, token_ids=ids, token_segments=list(wins),
                                        token_frames=list(local), token_times=list(times), token_confidence=token_conf, confidence=total)

    def _confidence_long_text(self, wav_file: str, text: Union[str, List[int]], measure: str, aggregation: str, fr_batch_size: int,
                              wildcard: Optional[str], wildcard_penalty: float, chunk_length_s: float, stride_length_s: Optional[float],
                              kwargs: Dict[str, Any]) -> LongformConfidenceResult:
        """``confidence_longform`` with a text, on either route of ``align_longform``: its alignment, and behind it on the same stream
        gam_op_ctc_confidence_long with the text's ids at ``tok_first`` as the alignment left them on the device (wildcards enabled:
        ``wildcard=`` set); ONE result is assembled from ``align_longform``'s own."""
        from .timestamps_utils import score_longform

        eng = self.head.engine if isinstance(self.decoding, _decoding.CTCGreedyDecoding) else None
        got: Dict[str, Any] = {}

        def align(lp_all: Tensor, ids: List[int], penalty: Optional[float]) -> Dict[str, Any]:
            star = None if penalty is None else eng.ctc_star_row(lp_all, None, penalty)
            al = eng.op_ctc_align_long(lp_all, ids, consume_flag=True, star=star)
            cf = eng.op_ctc_confidence_long(lp_all, ids, frames=al.tok_first, measure=measure, aggregation=aggregation,
                                            wildcard=penalty is not None) if ids else None
            h = al.host()
            got["cf"] = cf if h["status"] else None      # (a text that does not fit: the caller raises; its frames are no token list)
            return h

        if self._windows_route(kwargs):
            base = self._align_windows(wav_file, text, fr_batch_size, wildcard, wildcard_penalty, chunk_length_s, stride_length_s, align)
        else:
            base = self._align_regions(wav_file, text, fr_batch_size, wildcard, wildcard_penalty, kwargs, align)
        ids = base.token_ids
        conf = self._confidence_host(got["cf"], len(ids)) if got.get("cf") is not None else [0.0] * len(ids)
        wid = self.wildcard_id
        token_conf, words, segments, total = score_longform(self.decoding.tokenizer, ids, conf, base.words, base.segments, aggregation, wid)
        return LongformConfidenceResult(text=base.text, segments=segments, words=words, token_ids=ids, token_segments=base.token_segments,
                                        token_frames=base.token_frames, token_times=base.token_times, token_confidence=token_conf,
                                        confidence=total, gaps=base.gaps, score=base.score, log_likelihood=base.log_likelihood)

    def _confidence_regions(self, wav_file: str, measure: str, aggregation: str, fr_batch_size: int, beam: Optional[tuple],
                            kwargs: Dict[str, Any]) -> LongformConfidenceResult:
        """``confidence_longform`` over speech regions without text: the segmentation, the feeder and the one-batch pipeline of
        ``transcribe_longform``; per batch ONE encoder run, the decode, and behind it the batch pass of ``confidence_batch`` on the
        decode's device result.  ``beam``: (width, hotwords, hotword_boost, lm, lm_weight, word_bonus) of a CTC beam search, or None.
        A segment per chunk; a token's segment is its chunk, its frame the chunk's local frame."""
        from .engine import _to_host
        from .feeder import BatchFeeder
        from .timestamps_utils import aggregate_confidence, compute_frame_shift, frames_to_words, score_longform
        from .vad_utils import segment_audio_file

        is_ctc = isinstance(self.decoding, _decoding.CTCGreedyDecoding)
        self._default_vad(kwargs, "confidence_longform")
        segments, boundaries = segment_audio_file(wav_file, SAMPLE_RATE, device=self._device, **kwargs)
        out = LongformConfidenceResult(text="", segments=[], words=[], token_ids=[], token_segments=[], token_frames=[], token_times=[],
                                       token_confidence=[], confidence=None)
        if not segments:
            return out
        eng, tok = self.head.engine, self.decoding.tokenizer

        def run():
            chunks: List[tuple] = []

            def launch(n, batch):
                wav, lens = batch
                encoded, encoded_len = self._encode(wav, lens, getattr(feeder, "host_lengths", None))
                if beam is None:
                    dev_out = self.decoding.decode_device(self.head, encoded, encoded_len)
                else:
                    dev_out = self.decoding.decode_beam_device(self.head, encoded, encoded_len, *beam)
                if is_ctc:
                    cf = eng.ctc_confidence(encoded, encoded_len, dev_out, measure=measure, aggregation=aggregation)
                else:
                    cf = eng.rnnt_confidence(encoded, encoded_len, dev_out, measure=measure)
                return dev_out, cf, list(feeder.host_lengths), encoded_len

            def emit(pending) -> None:
                dev_out, cf, wl, encoded_len = pending
                rows = self.decoding.finish(dev_out)
                h = cf.host()
                _decoding.check_range(h["flag"])
                el = _to_host((encoded_len,), cf.event)[0].tolist()
                for i, (text, ids, frames) in enumerate(rows):
                    if not int(h["status"][i]):
                        raise GigaAMHipError(f"confidence pass rejected the tokens of chunk {len(chunks)}")
                    chunks.append((text, ids, frames, [float(c) for c in h["conf"][i, :len(ids)]], int(wl[i]), int(el[i])))

            feeder = BatchFeeder(segments, fr_batch_size, self._device)
            _pipeline(feeder, launch, emit)
            return chunks

        # chunk by chunk, as transcribe_longform builds its segments: a word never runs from one chunk's tokens into the next's
        for k, (text, ids, frames, conf, wl, el) in enumerate(self._file_run(run)):
            start, end = boundaries[k]
            shift = compute_frame_shift(wl, el) if el else 0.0
            words = [Word(text=w.text, start=round(w.start + start, 3), end=round(w.end + start, 3))
                     for w in frames_to_words(tok, ids, frames, shift)]
            token_conf, scored, (segment,), _ = score_longform(tok, ids, conf, words, [Segment(text=text, start=start, end=end, words=words)],
                                                               aggregation)
            out.segments.append(segment)
            out.words += scored
            out.token_ids += ids
            out.token_segments += [k] * len(ids)
            out.token_frames += frames
            out.token_times += [start + f * shift for f in frames]
            out.token_confidence += token_conf
        out.text = " ".join(sg.text for sg in out.segments)
        out.confidence = aggregate_confidence(out.token_confidence, aggregation)
        return out
