"""HipEngine: one ``gam_handle`` (include/gigaam_hip.h) behind torch tensors.

torch is plumbing here -- device memory, the current HIP stream and (in bench.py)
torch.distributed.  All compute happens in libgigaam_hip.so; there is no eager /
CPU fallback, and every method raises if the library or the GPU call fails.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import math
import os
import threading
from typing import Any, Callable, Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._lib import GamConfig, GigaAMHipError


def _get(cfg: Any, key: str, default: Any = None) -> Any:
    if cfg is None:
        return default
    if isinstance(cfg, Mapping):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def build_config(pre: Any = None, enc: Any = None, head: Any = None) -> GamConfig:
    """POD mirror of the checkpoint's cfg sub-trees.  Defaults follow the reference
    constructors (gigaam/preprocess.py:60-65, gigaam/encoder.py:510-526)."""
    c = GamConfig()
    sr = _get(pre, "sample_rate", 16000)
    c.sample_rate = sr
    c.n_mels = _get(pre, "features", 64)
    c.hop_length = _get(pre, "hop_length", sr // 100)
    c.win_length = _get(pre, "win_length", sr // 40)
    c.n_fft = _get(pre, "n_fft", sr // 40)
    c.center = int(bool(_get(pre, "center", True)))
    c.feat_in = _get(enc, "feat_in", 64)
    c.n_layers = _get(enc, "n_layers", 16)
    c.d_model = _get(enc, "d_model", 768)
    subs = _get(enc, "subsampling", "conv2d")
    assert subs in ("conv1d", "conv2d")  # encoder.py:48
    c.subsampling = _lib.SUBS_CONV2D if subs == "conv2d" else _lib.SUBS_CONV1D
    c.subs_kernel_size = _get(enc, "subs_kernel_size", 3)
    c.subsampling_factor = _get(enc, "subsampling_factor", 4)
    c.ff_expansion_factor = _get(enc, "ff_expansion_factor", 4)
    att = _get(enc, "self_attention_model", "rotary")
    assert att in ("rotary", "rel_pos"), f"Not supported attn = {att}"  # encoder.py:530-533
    c.self_attention_model = _lib.ATT_ROTARY if att == "rotary" else _lib.ATT_REL_POS
    c.n_heads = _get(enc, "n_heads", 16)
    c.pos_emb_max_len = _get(enc, "pos_emb_max_len", 5000)
    norm = _get(enc, "conv_norm_type", "batch_norm")
    assert norm in ("batch_norm", "layer_norm")  # encoder.py:377
    c.conv_norm_type = _lib.NORM_BATCH if norm == "batch_norm" else _lib.NORM_LAYER
    c.conv_kernel_size = _get(enc, "conv_kernel_size", 31)
    c.head_type = _lib.HEAD_NONE
    if head is not None:
        target = str(_get(head, "_target_", ""))
        dec, jn = _get(head, "decoder"), _get(head, "joint")
        if dec is not None and jn is not None or target.endswith("RNNTHead"):
            c.head_type = _lib.HEAD_RNNT
            c.num_classes = _get(dec, "num_classes")
            c.pred_hidden = _get(dec, "pred_hidden")
            c.pred_rnn_layers = _get(dec, "pred_rnn_layers")
            c.joint_hidden = _get(jn, "joint_hidden")
        elif target.endswith("Linear"):   # emotion model: torch.nn.Linear(in_features, out_features)
            c.head_type = _lib.HEAD_EMO
            c.num_classes = _get(head, "out_features")
        else:
            c.head_type = _lib.HEAD_CTC
            c.num_classes = _get(head, "num_classes")
    return c


_DTYPES = {
    torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16,
    torch.float64: _lib.DTYPE_F64, torch.int64: _lib.DTYPE_I64,
}


_I32, _F32, _F64 = torch.int32, torch.float32, torch.float64
_NP_DTYPES = {_I32: np.int32, _F32: np.float32, _F64: np.float64}


class _Layout:
    """The fields of ONE i32 buffer, stated ONCE per class: ``DIMS`` names the dimensions, ``FIELDS`` lists (name, shape, dtype) in buffer
    order -- the shape in names of dimensions or plain ints; the dtype i32, or f32 / f64 whose bits lie in the i32 words (an f64 field
    must start on an even word).  A fourth entry names a dimension: where that is false the field is absent (no words, None).  From
    that one statement come the words to allocate (``words``), the views of the device buffer and the same views of its numpy copy
    on the host (``views``): the three cannot disagree."""
    DIMS: Tuple[str, ...] = ()
    FIELDS: Tuple[tuple, ...] = ()

    @classmethod
    def _dims(cls, *dims) -> Dict[str, int]:
        return dict(zip(cls.DIMS, dims))

    @classmethod
    @functools.lru_cache(maxsize=256)      # (a decode loop asks for the same few dimensions again and again)
    def layout(cls, *dims) -> Tuple[Tuple[tuple, ...], Tuple[int, ...], int]:
        """(((name, first word, words, shape or None, dtype), ...) in buffer order, the words of each, words of the whole buffer)"""
        d, fields, o = cls._dims(*dims), [], 0
        for name, shape, dtype, *present in cls.FIELDS:
            if present and not d[present[0]]:
                fields.append((name, o, 0, None, dtype))
                continue
            shape = tuple(s if isinstance(s, int) else d[s] for s in shape)
            n = math.prod(shape) * (2 if dtype is _F64 else 1)
            if dtype is _F64 and o % 2:
                raise GigaAMHipError(f"{cls.__name__}.{name}: an f64 field must start on an even word, not {o}")
            fields.append((name, o, n, shape, dtype))
            o += n
        return tuple(fields), tuple(f[2] for f in fields), o

    @classmethod
    def words(cls, *dims) -> int:
        return cls.layout(*dims)[2]

    @staticmethod
    def views(layout: tuple, buf) -> Dict[str, Any]:
        """{name: its words of ``buf`` in its dtype and shape} -- ``buf`` the device buffer or its numpy copy on the host."""
        fields, sizes, words = layout
        on_host, out = isinstance(buf, np.ndarray), {}
        if on_host:
            parts = [buf[o: o + n] for _, o, n, _, _ in fields]
        else:       # (ONE split for all the fields: a slice each is a torch call each, and those are what building a result costs)
            parts = (buf if buf.shape[0] == words else buf[:words]).split_with_sizes(sizes)
        for (name, _, _, shape, dtype), v in zip(fields, parts):
            if shape is None:
                out[name] = None
                continue
            if dtype is not _I32:
                v = v.view(_NP_DTYPES[dtype] if on_host else dtype)
            if len(shape) > 1:
                v = v.reshape(shape) if on_host else v.view(shape)
            out[name] = v
        return out


class _Packed(_Layout):
    """A decode result whose outputs are views of ONE i32 device buffer (constructor: the buffer, then ``DIMS``, which become
    attributes), so that it reaches the host in one copy; its flag word is the one-word field ``ext``."""

    @classmethod
    def empty(cls, device, *dims, **kw):
        """Allocate the buffer for ``dims`` on ``device`` and construct the result over it."""
        return cls(torch.empty((cls.words(*dims),), dtype=_I32, device=device), *dims, **kw)

    def flag_word(self) -> Tensor:
        """The device word (i32 [1]) that receives the range flag."""
        return self.ext

    def _bind(self, buf: Tensor, *dims) -> None:
        self._layout = self.layout(*dims)
        self.__dict__.update(zip(self.DIMS, dims))
        self.__dict__.update(self.views(self._layout, buf))

    def _host_fields(self, buf: Tensor, **more: Tensor) -> Dict[str, Any]:
        """One blocking D2H of ``buf`` (and of each tensor of ``more``, a copy each under its own name) -> its fields as numpy views
        of the one host array, with ``flag`` in place of the flag word ``ext``."""
        arr, *rest = _to_host((buf, *more.values()), self.event)
        h = self.views(self._layout, arr)
        flag = HipEngine._flag_of(int(h.pop("ext")[-1]))
        if more:
            h.update(zip(more, rest))
        h["flag"] = flag
        return h


def _to_host(tensors: Sequence[Tensor], event, then: Optional[Callable[[List[np.ndarray]], Sequence[Tensor]]] = None,
             also_record: Sequence[Tensor] = ()) -> List[np.ndarray]:
    """THE device-to-host path of every decode result: blocking copies of ``tensors`` on the device's collect stream
    (``aux_streams``: a queue of its own), which waits for ``event`` -- the result's own completion, not whatever the caller has
    enqueued since (see ``_fetch_flag``) -- or, without one, for the caller's current stream; then ``record_stream`` on each
    (allocated on the launch stream, last read on this one).  ``then(arrays)``: further tensors to copy behind the same wait, for
    a result whose first block tells how much of the rest is worth copying; it runs with the collect stream current, what it
    makes there needs no ``record_stream``, and what it reads there is named in ``also_record``.  CPU tensors are returned as
    they are (``.numpy()``), no stream is touched."""
    if not tensors[0].is_cuda:
        out = [t.numpy() for t in tensors]
        return out + [t.numpy() for t in then(out)] if then else out
    dev = tensors[0].device
    side = HipEngine._collect_stream(dev)
    launch = torch.cuda.current_stream(dev) if event is None else None     # (here: inside the block below the current stream is ``side``)
    with torch.cuda.stream(side):
        if event is not None:
            side.wait_event(event)
        else:
            side.wait_stream(launch)
        out = [t.cpu().numpy() for t in tensors]
        if then:
            out += [t.cpu().numpy() for t in then(out)]
    for t in tensors:
        t.record_stream(side)
    for t in also_record:
        t.record_stream(side)
    return out


def _rows(ids_a: np.ndarray, fr_a: np.ndarray, counts: List[int]) -> List[Tuple[List[int], List[int]]]:
    """[(ids, frames)] host lists of the first ``counts[i]`` columns of row i (numpy row slices convert to lists at half the cost of
    per-row Tensor.tolist(): 0.33 -> 0.17 ms at 32 x 502)."""
    return [(ids_a[i, :c].tolist(), fr_a[i, :c].tolist()) for i, c in enumerate(counts)]


class Decoded(tuple, _Layout):
    """What ``ctc_greedy`` / ``rnnt_greedy`` return.  Unpacks as ``(ids, frames, counts)`` (``+ (dump, dump_count)`` when a
    logits dump was asked for) and carries the decode's two hidden companions as EXPLICIT fields -- they used to hang off the
    ``counts`` view as Python attributes, which any ``torch.cat`` / slice / unpack-and-repack dropped silently (ADVICE r3,
    VERDICT r4 weak #13):

    ``ext``    i32 [B + 1]: ``counts`` is its first B words, the last word receives the split-fp16 range flag
               (gam_range_flag_fetch), so ``collect`` brings both to the host in ONE copy;
    ``event``  recorded on the stream the decode ran on, right behind it: ``collect`` waits for THIS on its side stream, not
               for whatever the caller has enqueued since (the next batch of a launch-n / collect-n-1 pipeline);
    ``stream`` the stream the decode ran on.

    Pass the object itself to ``HipEngine.collect`` / ``shard.range_flag_of``; three bare tensors are accepted too, but then
    nothing is known about a flag or an event (a plain blocking copy on the current stream)."""
    DIMS = ("b", "cap")
    # ids | frames | counts + flag word: the prefix ``collect`` reads, of the greedy decodes' buffer and of ``BeamDecoded``'s
    FIELDS = (("ids", ("b", "cap"), _I32), ("frames", ("b", "cap"), _I32), ("ext", ("b1",), _I32))

    @classmethod
    def _dims(cls, b: int, cap: int) -> Dict[str, int]:
        return {"b": b, "cap": cap, "b1": b + 1}

    def __new__(cls, ids: Tensor, frames: Tensor, counts: Tensor, ext: Optional[Tensor] = None, event=None, stream=None,
                dump: Optional[Tensor] = None, dump_count: Optional[Tensor] = None, whole: Optional[Tensor] = None):
        self = tuple.__new__(cls, (ids, frames, counts) if dump is None else (ids, frames, counts, dump, dump_count))
        self.ext, self.event, self.stream = ext, event, stream
        # ``whole`` (r06): ids | frames | ext are views of ONE i32 buffer [2 B cap + B + 1] -- a small decode (CTC: 128 KB at 32 x 20 s)
        # then reaches the host in ONE blocking copy instead of three (counts first, then the used part of ids and of frames)
        self.whole = whole
        return self

    @staticmethod
    def packed(device, b: int, cap: int) -> "Decoded":
        """A greedy decode's result over ONE new buffer for ``cap`` tokens per utterance (``whole``); no event yet."""
        _, sizes, words = Decoded.layout(b, cap)
        whole = torch.empty((words,), dtype=_I32, device=device)
        ids, frames, ext = whole.split_with_sizes(sizes)      # (FIELDS' three, without ``views``' dict: bench.py's step makes this call)
        return Decoded(ids.view(b, cap), frames.view(b, cap), ext[:b], ext, whole=whole)

    ids = property(lambda self: self[0])
    frames = property(lambda self: self[1])
    counts = property(lambda self: self[2])

    def flag_word(self) -> Optional[Tensor]:
        """The device word (i32 [1]) that received the range flag of this decode, or None."""
        return None if self.ext is None else self.ext[-1:]


class Aligned(_Packed):
    """What ``ctc_align`` / ``op_ctc_align`` return: every output of the alignment kernel as a view of ONE i32 device buffer
    (``whole``) that reaches the host in ONE copy (``host``), like ``Decoded.whole``.  Layout: frame_labels [B, T'] | tok_first
    [B, Umax] | tok_last [B, Umax] | status [B] | score [B] (f32 bits) | loglik [B] (f32 bits) | range flag word."""
    DIMS = ("b", "tp", "umax")
    FIELDS = (("frame_labels", ("b", "tp"), _I32), ("tok_first", ("b", "umax"), _I32), ("tok_last", ("b", "umax"), _I32),
              ("status", ("b",), _I32), ("score", ("b",), _F32), ("loglik", ("b",), _F32), ("ext", (1,), _I32))

    def __init__(self, whole: Tensor, b: int, tp: int, umax: int, event=None, stream=None):
        self.whole, self.event, self.stream = whole, event, stream
        self._bind(whole, b, tp, umax)

    def host(self) -> Dict[str, Any]:
        """One blocking D2H of the whole result, on the collect stream behind the alignment's own completion event -> numpy arrays
        (``frame_labels``, ``tok_first``, ``tok_last``, ``status``, ``score``, ``loglik``) and ``flag`` (the split-fp16
        range flag of the encoder run that produced the log-probs: True = repeat under GAM_GEMM_F32)."""
        return self._host_fields(self.whole)


class KeywordHits(_Packed):
    """What ``ctc_kws`` / ``op_ctc_kws`` return: the hits of every (utterance, keyword) pair as views of ONE i32 device buffer
    (``whole``) that reaches the host in ONE copy (``host``), like ``Aligned``.  Layout: n_hits [B, K] | hit_frames [B, K, H, 2]
    (start, end) | hit_score [B, K, H] (f32 bits) | range flag word.  ``dense_score`` f32 / ``dense_start`` i32 [B, K, T'] (the
    per-frame E_t / S_t of gam_kws.h) are tensors of their own, present only when they were asked for."""
    DIMS = ("b", "k", "max_hits")
    FIELDS = (("n_hits", ("b", "k"), _I32), ("hit_frames", ("b", "k", "h", 2), _I32), ("hit_score", ("b", "k", "h"), _F32),
              ("ext", (1,), _I32))

    @classmethod
    def _dims(cls, b: int, k: int, max_hits: int) -> Dict[str, int]:
        # (max_hits outside [1, 64] is the library's error; the buffers only must not be negative.  The attribute keeps the caller's value)
        return {"b": b, "k": k, "h": max(max_hits, 0)}

    def __init__(self, whole: Tensor, b: int, k: int, max_hits: int, dense_score: Optional[Tensor] = None,
                 dense_start: Optional[Tensor] = None, event=None, stream=None):
        self.whole, self.event, self.stream = whole, event, stream
        self.dense_score, self.dense_start = dense_score, dense_start
        self._bind(whole, b, k, max_hits)

    def host(self) -> Dict[str, Any]:
        """One blocking D2H of the hits, on the collect stream behind the search's own completion event -> numpy arrays ``n_hits``
        [B, K], ``hit_frames`` [B, K, H, 2], ``hit_score`` [B, K, H] and ``flag`` (the split-fp16 range flag of the encoder run that
        produced the log-probs: True = repeat under GAM_GEMM_F32).  With dense outputs: ``dense_score`` / ``dense_start`` too (a
        copy each).  Never the log-probs."""
        if self.dense_score is None:
            return self._host_fields(self.whole)
        return self._host_fields(self.whole, dense_score=self.dense_score, dense_start=self.dense_start)


class KeywordStreamHits(_Packed):
    """What ``KeywordStream.finish`` returns: the hits of every keyword over ONE stream as views of ONE i32 device buffer (``whole``) that
    reaches the host in ONE copy (``host``).  Layout: n_hits [K] | status [K] | hit_frames [K, H, 2] (start, end; stream frames) |
    hit_score [K, H] (f32 bits) | range flag word.  ``n_hits`` counts every hit of the stream (above H: the first H are listed);
    ``status`` is that of the stream's LAST call (gam_op_ctc_kws_stream)."""
    DIMS = ("k", "max_hits")
    FIELDS = (("n_hits", ("k",), _I32), ("status", ("k",), _I32), ("hit_frames", ("k", "h", 2), _I32), ("hit_score", ("k", "h"), _F32),
              ("ext", (1,), _I32))

    @classmethod
    def _dims(cls, k: int, max_hits: int) -> Dict[str, int]:
        return {"k": k, "h": max(max_hits, 0)}

    def __init__(self, whole: Tensor, k: int, max_hits: int, event=None, stream=None):
        self.whole, self.event, self.stream = whole, event, stream
        self._bind(whole, k, max_hits)

    def host(self, check: bool = True) -> Dict[str, Any]:
        """One blocking D2H of the whole result, on the collect stream behind the END call's completion event -> numpy arrays ``n_hits``
        [K], ``status`` [K], ``hit_frames`` [K, H, 2], ``hit_score`` [K, H] and ``flag`` (as ``KeywordHits.host``).  A zero in
        ``status`` -- the library refused a call of this stream for that keyword -- raises ``GigaAMHipError`` unless ``check`` is off."""
        h = self._host_fields(self.whole)
        if check and not h["status"].all():
            raise GigaAMHipError(f"keyword stream: the call was refused for keywords {np.nonzero(h['status'] == 0)[0].tolist()[:8]} (the "
                                 "state was not begun or has ended, a frame was skipped, or set_keywords was called during the stream)")
        return h


class _ResumableStream:
    """One stream of any length fed in pieces to a resumable kernel: the bookkeeping ``KeywordStream`` and ``BeamStream`` share.  Owns
    the state record (``state``) and the result (``out``), counts the frames (``t_next``), adds BEGIN to the first call and refuses a
    call after the END one.  A subclass gives ``NAME`` / ``MAKER`` (for the messages), ``BEGIN`` / ``END``, ``_launch`` (the op),
    ``_empty_v`` (the V of an END call when nothing was pushed) and, if it has one, ``_precheck``."""

    def __init__(self, engine: "HipEngine", state: Tensor, out):
        self.engine, self.state, self.out = engine, state, out
        self.t_next, self.begun, self.ended, self.v = 0, False, False, None

    def _precheck(self) -> None:
        """What must hold before BEGIN and before any launch."""

    def _call(self, log_probs: Optional[Tensor], v: int, flags: int, overlap: bool, **kw):
        eng = self.engine
        if self.ended:
            raise GigaAMHipError(f"{self.NAME}: the stream has ended (finish); make a new one with {self.MAKER}()")
        self._precheck()
        if not self.begun:
            flags |= self.BEGIN
        side = eng._decode_side_stream() if overlap else None
        if overlap:
            side.wait_stream(torch.cuda.current_stream(eng.device))
        with torch.cuda.stream(side) if overlap else torch.cuda.device(eng.device):
            rows = self._launch(log_probs, v, flags, **kw)
            if overlap:      # allocated on the launch stream, last used on the side stream
                for t in (log_probs, self.state, self.out.whole):
                    if t is not None:
                        t.record_stream(side)
        self.begun = True
        self.t_next += 0 if log_probs is None else int(log_probs.shape[0])
        self.ended = bool(flags & self.END)
        return rows

    def push(self, log_probs: Tensor, overlap: bool = False):
        """Enqueue the search of the next ``n`` rows (log_probs f32 [n, V], used as they are; n = 0 is legal); the first call begins
        the stream.  ``overlap``: on the engine's decode SIDE stream, behind everything enqueued on the current stream so far (as
        ``rnnt_greedy(overlap=True)``) -- the caller's next encoder call then runs beside this search; the library orders the
        decode-class calls of a handle whatever streams they run on."""
        return self._push(log_probs, overlap)

    def _push(self, log_probs: Tensor, overlap: bool, **kw):
        log_probs = self.engine._dev(log_probs, torch.float32)
        if log_probs.dim() != 2:
            raise GigaAMHipError(f"{self.NAME}: log_probs must be [n, V], got {tuple(log_probs.shape)}")
        self.v = int(log_probs.shape[1])
        return self._call(log_probs, self.v, 0, overlap, **kw)

    def finish(self, consume_flag: bool = False):
        """The END call (no rows), on the current stream -> the stream's result (``out``).  ``consume_flag``: the rows came from this
        engine's encoder -- move the split-fp16 range flag into the result's flag word."""
        self._call(None, self._empty_v() if self.v is None else self.v, self.END, False)
        with torch.cuda.device(self.engine.device):
            return self.engine._finish(self.out, consume_flag)


class KeywordStream(_ResumableStream):
    """Keyword search over one stream of any length fed in pieces (``HipEngine.kws_stream``; gam_op_ctc_kws_stream): owns the state
    record and the hit arrays of the keyword set that was at hand when it was made.  ``push`` enqueues the next rows, ``finish`` ends the
    stream (the END call emits the open candidate) and returns its ``KeywordStreamHits``; neither synchronises the host."""
    BEGIN, END = 1, 2      # include/gigaam_hip.h GAM_KWS_STREAM_BEGIN / _END
    NAME, MAKER = "keyword stream", "kws_stream"

    def __init__(self, engine: "HipEngine", max_hits: int = 8):
        self.max_hits = int(max_hits)
        self.k = self._set_size(engine)
        nbytes = int(engine.lib.gam_ctc_kws_state_bytes(engine._h))
        if nbytes < 0:
            engine._check(-1, "gam_ctc_kws_state_bytes")
        if nbytes != self.k * engine.KWS_STATE_WORDS * 4:
            raise GigaAMHipError(f"keyword stream: {nbytes} state bytes for {self.k} keywords, expected {engine.KWS_STATE_WORDS * 4} each")
        # (max_hits outside [1, 4096] is the library's error at the first push; the buffers only must not be negative)
        super().__init__(engine, torch.zeros((nbytes // 4,), dtype=_I32, device=engine.device),
                         KeywordStreamHits.empty(engine.device, self.k, self.max_hits))

    @staticmethod
    def _set_size(engine: "HipEngine") -> int:
        key = getattr(engine, "_keywords_key", None)
        return len(key[0]) if key else 0

    def _precheck(self) -> None:      # (before BEGIN and before any launch: see op_ctc_kws_stream)
        at_hand = self._set_size(self.engine)
        if at_hand != self.k:
            raise GigaAMHipError(f"keyword stream: made for {self.k} keywords, the set at hand has {at_hand} "
                                 "(set_keywords was called with another set since kws_stream(); make a new stream)")

    def _launch(self, log_probs: Optional[Tensor], v: int, flags: int, dense: bool = False):
        return self.engine.op_ctc_kws_stream(log_probs, v, self.t_next, flags, self.state, self.out, dense)

    def _empty_v(self) -> int:      # nothing was pushed: any V that the keyword ids fit
        return max((max(p) for p in self.engine._keywords_key[0]), default=0) + 2

    def push(self, log_probs: Tensor, dense: bool = False, overlap: bool = False):
        """``_ResumableStream.push``; ``dense``: returns this call's (dense_score f32, dense_start i32) [K, n], allocated on the stream
        the call ran on."""
        return self._push(log_probs, overlap, dense=dense)


class BeamStreamDecoded(_Packed):
    """What ``BeamStream.finish`` returns: the beam search's result over ONE stream as views of ONE i32 device buffer (``whole``).
    Layout: score (f64 bits, 2 words) | logp (f64 bits, 2 words) | count | status | ids [max_frames] | frames [max_frames] (stream
    frames) | range flag word.  ``status`` is that of the stream's LAST call (gam_op_ctc_beam_stream)."""
    DIMS = ("max_frames",)
    FIELDS = (("score", (1,), _F64), ("logp", (1,), _F64), ("count", (1,), _I32), ("status", (1,), _I32),
              ("ids", ("max_frames",), _I32), ("frames", ("max_frames",), _I32), ("ext", (1,), _I32))
    HEAD_WORDS = 6      # score | logp | count | status: what ``host`` copies first

    @classmethod
    def _dims(cls, max_frames: int) -> Dict[str, int]:
        # (at least one word each: the library takes no NULL ids / frames, and an empty view has no address; the attribute keeps
        # the caller's value)
        return {"max_frames": max(max_frames, 1)}

    def __init__(self, whole: Tensor, max_frames: int, event=None, stream=None):
        self.whole, self.event, self.stream = whole, event, stream
        self._bind(whole, max_frames)

    def host(self, check: bool = True) -> Dict[str, Any]:
        """The result on the host, on the collect stream behind the END call's completion event: the small block and the flag word
        first, then only ``count`` entries of ids and of frames -> ``ids`` / ``frames`` (numpy i32 [count]), ``count`` / ``status``
        (int), ``score`` / ``logp`` (Python floats from the float64 outputs) and ``flag`` (as ``Aligned.host``).  Status 0 -- the
        library refused the stream's last call -- raises ``GigaAMHipError`` unless ``check`` is off (ids / frames are then empty)."""
        hw = self.HEAD_WORDS

        def used(first):
            n = int(first[0][4]) if int(first[0][5]) else 0
            return (self.ids[:n], self.frames[:n])

        head, ext, ids, frames = _to_host((self.whole[:hw], self.ext), self.event, used, also_record=(self.whole,))
        status = int(head[5])
        if check and not status:
            raise GigaAMHipError("beam stream: the call was refused (the state was not begun or has ended, a frame was skipped, the width "
                                 "or V changed, set_hotwords / set_lm was called during the stream, or rows beyond max_frames)")
        return {"ids": ids, "frames": frames, "count": int(ids.shape[0]), "status": status, "score": float(head[:2].view(np.float64)[0]),
                "logp": float(head[2:4].view(np.float64)[0]), "flag": HipEngine._flag_of(int(ext[-1]))}


class BeamStream(_ResumableStream):
    """CTC prefix beam search over one stream of any length fed in pieces (``HipEngine.beam_stream``; gam_op_ctc_beam_stream): owns
    the state record with its node pool and the result.  The hotword set and the LM are those the engine holds at the first ``push``;
    the kernel refuses the calls that follow a later ``set_hotwords`` / ``set_lm``.  ``push`` enqueues the next rows, ``finish`` ends
    the stream (the END call makes the final pick and the backtrack) and returns its ``BeamStreamDecoded``; neither synchronises the host."""
    BEGIN, END = 1, 2      # include/gigaam_hip.h GAM_BEAM_STREAM_BEGIN / _END
    NAME, MAKER = "beam stream", "beam_stream"

    def __init__(self, engine: "HipEngine", beam_size: int, max_frames: int):
        engine._check_beam(beam_size)
        self.beam_size, self.max_frames = int(beam_size), int(max_frames)
        nbytes = int(engine.lib.gam_ctc_beam_stream_bytes(engine._h, self.beam_size, self.max_frames))
        if nbytes < 0:
            engine._check(-1, "gam_ctc_beam_stream_bytes")
        super().__init__(engine, torch.zeros(((nbytes + 3) // 4,), dtype=_I32, device=engine.device),
                         BeamStreamDecoded.empty(engine.device, self.max_frames))
        self.out.whole[:BeamStreamDecoded.HEAD_WORDS].zero_()      # (a stream refused before its END call has status 0, count 0)

    def _launch(self, log_probs: Optional[Tensor], v: int, flags: int) -> None:
        self.engine.op_ctc_beam_stream(log_probs, v, self.t_next, flags, self.beam_size, self.state, self.out)

    def _empty_v(self) -> int:      # nothing was pushed: the V of the LM at hand, else any V the hotword ids fit
        return self.engine._beam_stream_v()


class RnntGreedyStream(_ResumableStream):
    """RNN-T greedy decode over one stream of any length fed in pieces (``HipEngine.rnnt_greedy_stream``;
    gam_op_rnnt_greedy_stream): owns the state record and a one-row packed ``Decoded`` with room for ``max_frames * max_symbols``
    tokens.  ``push`` enqueues the next rows of the encoder projection (``HipEngine.rnnt_encp``), ``finish`` ends the stream and returns
    the ``Decoded``, which ``HipEngine.collect`` reads like any greedy decode (frames are stream frames); neither synchronises the
    host.  ``out.counts`` holds the tokens so far after every accepted call.  ``status`` (i32 [1] on the device) is that of the
    stream's LAST call: 0 = the library refused it (``check`` raises)."""
    BEGIN, END = 1, 2      # include/gigaam_hip.h GAM_RNNT_STREAM_BEGIN / _END
    NAME, MAKER = "RNN-T greedy stream", "rnnt_greedy_stream"

    def __init__(self, engine: "HipEngine", max_frames: int, max_symbols: int):
        self.max_frames, self.max_symbols = int(max_frames), int(max_symbols)
        if self.max_frames < 0 or self.max_symbols < 1 or self.max_frames * self.max_symbols >= 2 ** 31:
            raise GigaAMHipError(f"RNN-T greedy stream: max_frames {max_frames} x max_symbols {max_symbols} outside [0, 2^31)")
        nbytes = int(engine.lib.gam_rnnt_greedy_stream_bytes(engine._h))
        if nbytes < 0:
            engine._check(-1, "gam_rnnt_greedy_stream_bytes")
        self.state_bytes = nbytes
        self.cap = max(self.max_frames * self.max_symbols, 1)      # (at least one word: the library takes no NULL ids / frames)
        # the record, and behind it the status word (one buffer: what a side-stream call must keep alive)
        state = torch.zeros(((nbytes + 3) // 4 + 1,), dtype=_I32, device=engine.device)
        super().__init__(engine, state, Decoded.packed(engine.device, 1, self.cap))
        self.status = state[-1:]
        self.out.whole.zero_()      # (a stream refused at its first call has count 0)

    def _launch(self, encp_rows: Optional[Tensor], v: int, flags: int) -> None:
        self.engine.op_rnnt_greedy_stream(encp_rows, self.t_next, flags, self.max_symbols, self.state, self.state_bytes, self.out,
                                          self.status)

    def _empty_v(self) -> int:
        return int(self.engine.cfg.joint_hidden)

    def push(self, encp_rows: Tensor, overlap: bool = False):
        """``_ResumableStream.push`` of rows of the encoder projection, f32 [n, joint_hidden] (n = 0 is legal)."""
        encp_rows = self.engine._dev(encp_rows, torch.float32)
        if encp_rows.dim() != 2 or int(encp_rows.shape[1]) != self._empty_v():
            raise GigaAMHipError(f"{self.NAME}: encp rows must be [n, {self._empty_v()}], got {tuple(encp_rows.shape)}")
        self.v = self._empty_v()
        return self._call(encp_rows, self.v, 0, overlap)

    def check(self) -> None:
        """Raise ``GigaAMHipError`` if the library refused the stream's last call (one blocking one-word copy)."""
        if not int(_to_host((self.status,), getattr(self.out, "event", None))[0][0]):
            raise GigaAMHipError("RNN-T greedy stream: the call was refused (the state was not begun or has ended, a frame was skipped, "
                                 "max_symbols or the head changed, or more rows than max_frames)")


class RnntBeamStream(_ResumableStream):
    """RNN-T beam search over one stream of any length fed in pieces (``HipEngine.rnnt_beam_stream``; gam_op_rnnt_beam_stream): owns
    the state record -- the beam, the predictor-state slots and the node pool of ``max_frames * max_symbols * beam_size`` nodes -- and
    the result, a ``BeamStreamDecoded`` whose one dimension is ``cap = max_frames * max_symbols`` tokens.  The hotword set and the LM
    are those the engine holds at the first ``push``; the kernel refuses the calls that follow a later ``set_hotwords`` / ``set_lm``.
    ``push`` enqueues the next rows of the encoder projection (``HipEngine.rnnt_encp``), ``finish`` ends the stream (the END call makes
    the final pick and the backtrack) and returns the ``BeamStreamDecoded`` (frames are stream frames); neither synchronises the host."""
    BEGIN, END = 1, 2      # include/gigaam_hip.h GAM_RNNT_STREAM_BEGIN / _END
    NAME, MAKER = "RNN-T beam stream", "rnnt_beam_stream"

    def __init__(self, engine: "HipEngine", beam_size: int, max_frames: int, max_symbols: int):
        engine._check_beam(beam_size, max_symbols)
        self.beam_size, self.max_frames, self.max_symbols = int(beam_size), int(max_frames), int(max_symbols)
        nbytes = int(engine.lib.gam_rnnt_beam_stream_bytes(engine._h, self.beam_size, self.max_symbols, self.max_frames))
        if nbytes < 0:
            engine._check(-1, "gam_rnnt_beam_stream_bytes")
        self.state_bytes = nbytes
        self.cap = self.max_frames * self.max_symbols
        super().__init__(engine, torch.zeros(((nbytes + 3) // 4,), dtype=_I32, device=engine.device),
                         BeamStreamDecoded.empty(engine.device, self.cap))
        self.out.whole[:BeamStreamDecoded.HEAD_WORDS].zero_()      # (a stream refused before its END call has status 0, count 0)

    def _launch(self, encp_rows: Optional[Tensor], v: int, flags: int) -> None:
        self.engine.op_rnnt_beam_stream(encp_rows, self.t_next, flags, self.beam_size, self.max_symbols, self.state, self.state_bytes,
                                        self.out)

    def _empty_v(self) -> int:
        return int(self.engine.cfg.joint_hidden)

    def push(self, encp_rows: Tensor, overlap: bool = False):
        """``_ResumableStream.push`` of rows of the encoder projection, f32 [n, joint_hidden] (n = 0 is legal)."""
        encp_rows = self.engine._dev(encp_rows, torch.float32)
        if encp_rows.dim() != 2 or int(encp_rows.shape[1]) != self._empty_v():
            raise GigaAMHipError(f"{self.NAME}: encp rows must be [n, {self._empty_v()}], got {tuple(encp_rows.shape)}")
        self.v = self._empty_v()
        return self._call(encp_rows, self.v, 0, overlap)


class AlignedLong(_Packed):
    """What ``op_ctc_align_long`` returns: every output of the long-utterance alignment as a view of ONE i32 device buffer (``whole``)
    that reaches the host in ONE copy (``host``), like ``Aligned``.  Layout: score (f64 bits, 2 words) | loglik (f64 bits, 2 words) |
    status | range flag word | frame_labels [T] | tok_first [U] | tok_last [U]."""
    DIMS = ("t", "u")
    FIELDS = (("score", (1,), _F64), ("loglik", (1,), _F64), ("status", (1,), _I32), ("ext", (1,), _I32),
              ("frame_labels", ("t",), _I32), ("tok_first", ("u",), _I32), ("tok_last", ("u",), _I32))

    def __init__(self, whole: Tensor, t: int, u: int, event=None, stream=None):
        self.whole, self.event, self.stream = whole, event, stream
        self._bind(whole, t, u)

    def host(self) -> Dict[str, Any]:
        """One blocking D2H of the whole result, on the collect stream behind the alignment's own completion event -> ``frame_labels``,
        ``tok_first``, ``tok_last`` (numpy i32), ``status`` (int), ``score`` / ``loglik`` (Python floats from the float64 outputs) and
        ``flag`` (as ``Aligned.host``)."""
        h = self._host_fields(self.whole)
        h["score"], h["loglik"], h["status"] = float(h["score"][0]), float(h["loglik"][0]), int(h["status"][0])
        return h


class RnntAligned(_Packed):
    """What ``rnnt_align`` / ``op_rnnt_align`` / ``op_rnnt_lattice_align`` return: every output of the transducer alignment as a view of
    ONE i32 device buffer (``whole``) that reaches the host in ONE copy (``host``), like ``Aligned``.  Layout: tok_frame [B, Umax] |
    status [B] | score [B] (f32 bits) | loglik [B] (f32 bits) | range flag word.  ``lattice`` (``op_rnnt_align(want_lattice=True)``):
    the (log P(blank), log P(next token)) lattice f32 [B, T', Umax + 1, 2] on the device."""
    DIMS = ("b", "umax")
    FIELDS = (("tok_frame", ("b", "umax"), _I32), ("status", ("b",), _I32), ("score", ("b",), _F32), ("loglik", ("b",), _F32),
              ("ext", (1,), _I32))

    def __init__(self, whole: Tensor, b: int, umax: int, event=None, stream=None):
        self.whole, self.event, self.stream = whole, event, stream
        self.lattice: Optional[Tensor] = None
        self._bind(whole, b, umax)

    def host(self) -> Dict[str, Any]:
        """One blocking D2H of the whole result, on the collect stream behind the alignment's own completion event -> numpy arrays
        (``tok_frame``, ``status``, ``score``, ``loglik``) and ``flag`` (the split-fp16 range flag, as ``Aligned.host``)."""
        return self._host_fields(self.whole)


class Confidence(_Packed):
    """What ``ctc_confidence`` / ``op_ctc_confidence`` / ``rnnt_confidence`` / ``op_rnnt_confidence`` return: the token confidences of a
    finished decode as views of ONE i32 device buffer (``whole``) that reaches the host in ONE copy (``host``), like ``Aligned``.
    Layout: conf [B, cap] (f32 bits) | span [B, cap] (CTC only) | status [B] | range flag word."""
    DIMS = ("b", "cap", "has_span")
    FIELDS = (("conf", ("b", "cap"), _F32), ("span", ("b", "cap"), _I32, "has_span"), ("status", ("b",), _I32), ("ext", (1,), _I32))

    def __init__(self, whole: Tensor, b: int, cap: int, has_span: bool, event=None, stream=None):
        self.whole, self.event, self.stream = whole, event, stream
        self._bind(whole, b, cap, has_span)

    def host(self) -> Dict[str, Any]:
        """One blocking D2H of the whole result, on the collect stream behind the pass's own completion event -> numpy arrays
        (``conf`` f32 [B, cap], ``span`` i32 [B, cap] or None, ``status`` i32 [B]) and ``flag`` (the split-fp16 range flag, as
        ``Aligned.host``)."""
        return self._host_fields(self.whole)


class BeamDecoded(Decoded, _Packed):
    """What ``ctc_beam`` / ``op_ctc_beam`` / ``rnnt_beam`` / ``op_rnnt_beam`` return: a ``Decoded`` (ids, frames, counts + range flag word: ``collect``, ``finish`` and the
    word builder take it as they take a greedy decode) whose buffer goes on with ``score`` and ``logp`` f32 [B] (``buf``: ids [B, cap] |
    frames [B, cap] | counts [B] | flag word | score bits [B] | logp bits [B]).  ``host`` brings all of it to the host in ONE copy."""
    FIELDS = Decoded.FIELDS + (("score", ("b",), _F32), ("logp", ("b",), _F32))

    def __new__(cls, buf: Tensor, b: int, tp: int, event=None, stream=None):
        # (tp: the width of ids / frames -- T' for CTC, T' * max_symbols for RNN-T)
        layout = cls.layout(b, tp)
        v = cls.views(layout, buf)
        self = Decoded.__new__(cls, v["ids"], v["frames"], v["ext"][:b], v["ext"], event, stream, whole=buf[: Decoded.words(b, tp)])
        self.buf, self.score, self.logp, self._layout = buf, v["score"], v["logp"], layout
        return self

    def host(self) -> Dict[str, Any]:
        """One blocking D2H of the whole result, on the collect stream behind the beam search's own completion event -> ``rows``
        [(ids, frames)] host lists, ``score`` / ``logp`` numpy f32 [B] and ``flag`` (the split-fp16 range flag, as ``collect``)."""
        arr, = _to_host((self.buf,), self.event)
        h = self.views(self._layout, arr)
        n = h["ext"].tolist()
        flag = HipEngine._flag_of(n.pop())
        return {"rows": _rows(h["ids"], h["frames"], n), "score": h["score"].copy(), "logp": h["logp"].copy(), "flag": flag}


class NBestDecoded(_Packed):
    """What ``ctc_beam_nbest`` / ``op_ctc_beam_nbest`` / ``rnnt_beam_nbest`` / ``op_rnnt_beam_nbest`` return: the ``n`` best hypotheses
    of each final beam, on the device.  ``ids`` / ``frames`` i32 [B, n, cap]; the small block ``small`` is ONE i32 buffer: n_hyp [B] |
    counts [B, n] | score bits [B, n] | logp bits [B, n] | range flag word.  Row 0 of every utterance is the 1-best search's result."""
    DIMS = ("b", "n")
    FIELDS = (("n_hyp", ("b",), _I32), ("counts", ("b", "n"), _I32), ("score", ("b", "n"), _F32), ("logp", ("b", "n"), _F32),
              ("ext", (1,), _I32))

    def __init__(self, tok: Tensor, small: Tensor, event=None, stream=None):
        # (tok: i32 [2, B, n, cap], ids | frames)
        _, b, n, cap = tok.shape
        self.tok, self.ids, self.frames, self.small, self.cap = tok, tok[0], tok[1], small, cap
        self.event, self.stream = event, stream
        self._bind(small, b, n)
        self.copied_bytes = 0     # what the last ``host()`` brought over

    @classmethod
    def empty(cls, device, b: int, n: int, cap: int) -> "NBestDecoded":
        return cls(torch.empty((2, b, n, cap), dtype=_I32, device=device), torch.empty((cls.words(b, n),), dtype=_I32, device=device))

    def host(self) -> Dict[str, Any]:
        """At most TWO blocking D2H copies, on the collect stream behind the search's own completion event: the small block, then
        columns [0, longest hypothesis) of ids | frames ([B, n, cap] can be tens of MB for RNN-T and is never copied whole) ->
        ``rows`` [b][r] = (ids, frames) host lists for r < n_hyp[b], ``score`` / ``logp`` numpy f32 [B, n] (-inf past n_hyp),
        ``n_hyp`` numpy i32 [B] and ``flag`` (the split-fp16 range flag, as ``collect``)."""
        h: Dict[str, Any] = {}

        def used_columns(arrs: List[np.ndarray]) -> List[Tensor]:
            h.update(self.views(self._layout, arrs[0]))
            m = int(h["counts"].max()) if h["counts"].size else 0
            return [self.tok[..., :m].contiguous()] if m > 0 else []

        arr, *tok = _to_host((self.small,), self.event, then=used_columns, also_record=(self.tok,))
        tok = tok[0] if tok else None
        self.copied_bytes = arr.nbytes + (0 if tok is None else tok.nbytes)
        n_hyp, counts = h["n_hyp"].copy(), h["counts"].tolist()      # (lists: a numpy scalar per index costs more than the row it cuts)
        rows = [[(tok[0, i, r, :c].tolist(), tok[1, i, r, :c].tolist()) if c else ([], []) for r, c in enumerate(counts[i][:nh])]
                for i, nh in enumerate(n_hyp.tolist())]
        return {"rows": rows, "score": h["score"].copy(), "logp": h["logp"].copy(), "n_hyp": n_hyp,
                "flag": HipEngine._flag_of(int(h["ext"][0]))}


def _ptr(t: Optional[Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


class HipEngine:
    """Owns one library handle on one GPU."""

    def __init__(self, config: GamConfig, state_dict: Mapping[str, Tensor], device: torch.device):
        self.lib = _lib.load_library()
        device = torch.device(device)
        if device.type != "cuda":
            raise GigaAMHipError(f"gigaam_amd runs on a ROCm GPU only (device={device}); there is no CPU path")
        if not torch.cuda.is_available():
            raise GigaAMHipError("no ROCm GPU visible to torch")
        self.device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        self.cfg = config
        self._h = C.c_void_p()
        rc = self.lib.gam_create(C.byref(config), self.device.index, C.byref(self._h))
        self._check(rc, "gam_create")
        for key, val in state_dict.items():
            if not isinstance(val, Tensor):
                continue
            t = val.detach().to("cpu").contiguous()
            if t.dtype not in _DTYPES:
                t = t.to(torch.float32)
            shape = (C.c_int64 * max(1, t.dim()))(*t.shape)
            rc = self.lib.gam_set_weight(self._h, key.encode(), C.c_void_p(t.data_ptr()), _DTYPES[t.dtype], shape, t.dim())
            self._check(rc, f"gam_set_weight({key})")
        self._check(self.lib.gam_finalize(self._h), "gam_finalize")
        # the cluster size in force outside an overlapped decode: what gam_create read from the environment (clamped like it does), then
        # whatever the caller set through set_rnnt_cluster -- an overlapped decode restores THIS, not the environment's value
        self._rnnt_cluster_user = max(-1, min(8, int(os.environ.get("GAM_RNNT_CLUSTER", "-1"))))

    # ------------------------------------------------------------------ utils
    def _check(self, rc: int, what: str) -> None:
        if rc != 0:
            msg = self.lib.gam_last_error(self._h)
            raise GigaAMHipError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")

    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, t: Tensor, dtype: torch.dtype) -> Tensor:
        return t.to(device=self.device, dtype=dtype).contiguous()

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.gam_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_gemm_mode(self, mode: str) -> None:
        """"f32" (exact fp32 MFMA), "f16x3" (three-term split-fp16 MFMA, fp32-equivalent; the default) or "f16" (OPT-IN speed
        mode: one fp16 MFMA per product, fp32 accumulation -- the reference's GPU autocast contract, not its CPU one)."""
        m = {"f32": _lib.GEMM_F32, "f16x3": _lib.GEMM_F16X3, "f16": _lib.GEMM_F16}[mode]
        self._check(self.lib.gam_set_gemm_mode(self._h, m), "gam_set_gemm_mode")

    @property
    def gemm_mode(self) -> str:
        return {_lib.GEMM_F32: "f32", _lib.GEMM_F16X3: "f16x3", _lib.GEMM_F16: "f16"}[self.lib.gam_get_gemm_mode(self._h)]

    def range_flag(self) -> bool:
        """True if, since the last call, an unscaled split-fp16 GEMM operand left fp16's range (gam_range_flag);
        synchronises the current stream and clears the flag.  NOTE: ``ctc_greedy`` / ``rnnt_greedy`` CONSUME the flag (they
        move it into the hidden tail word of the counts buffer they return, which ``collect`` reads): after a decode call
        this method reports 0 -- read the flag from the ``Decoded`` object they return (``.flag_word()``) or through ``collect``."""
        out = C.c_int(0)
        with torch.cuda.device(self.device):
            self._check(self.lib.gam_range_flag(self._h, C.byref(out), self._stream()), "gam_range_flag")
        return self._flag_of(out.value)

    def _fetch_flag(self, word: Tensor):
        """Move the range flag into ``word`` (the result's ``flag_word()``, i32 [1]) and record "this decode is complete" on the
        stream it ran on; returns (event, stream) for the result object.  ``collect`` waits for the event on a side stream, so a caller
        that has already launched the next batch (model.transcribe_longform, shard.run_sharded, bench.py configs 4 / 5) is not
        held until that next batch has finished too -- a ``.cpu()`` on the launch stream is ordered behind everything enqueued
        there, which made the "launch n, then collect n-1" pipelines wait for batch n (measured: +3.9 ms per 33 ms step)."""
        rc = self.lib.gam_range_flag_fetch(self._h, _ptr(word), self._stream())
        self._check(rc, "gam_range_flag_fetch")
        st = torch.cuda.current_stream(self.device)
        evt = torch.cuda.Event()
        evt.record(st)
        return evt, st

    def _finish(self, out, consume_flag: bool):
        """The tail of every decode-class call but the overlapped ``rnnt_greedy``: fill the result's flag word and set its completion
        ``event`` / ``stream``, on the current stream.  ``consume_flag``: the call ran the encoder's GEMMs -- move the range flag into
        the word (``_fetch_flag``); otherwise (an ``op_*`` call: no encoder ran) the word is 0.  No kernel writes that word, so where
        in the call's own stream order it is filled does not matter."""
        word = out.flag_word()
        if consume_flag:
            out.event, out.stream = self._fetch_flag(word)
        else:
            word.zero_()
            out.stream = torch.cuda.current_stream(self.device)
            out.event = torch.cuda.Event()
            out.event.record(out.stream)
        return out

    # the three forms a decode-class call takes its input in -> the device tensors and the dimensions
    def _in_encoded(self, encoded: Tensor, enc_len: Optional[Tensor]):
        """encoded f32 [B, d_model, T'], enc_len i32 [B] (or None) -> (encoded, enc_len, B, T')"""
        encoded = self._dev(encoded, torch.float32)
        b, _, tp = encoded.shape
        return encoded, None if enc_len is None else self._dev(enc_len, torch.int32), b, tp

    def _in_log_probs(self, log_probs: Tensor, enc_len: Tensor):
        """log_probs f32 [B, T', V], enc_len i32 [B] -> (log_probs, enc_len, B, T', V)"""
        log_probs = self._dev(log_probs, torch.float32)
        return (log_probs, self._dev(enc_len, torch.int32), *log_probs.shape)

    def _in_encp(self, encp: Tensor, enc_len: Tensor):
        """encp f32 [B, T', joint_hidden], enc_len i32 [B] -> (encp, enc_len, B, T')"""
        encp = self._dev(encp, torch.float32)
        b, tp, jh = encp.shape
        if jh != self.cfg.joint_hidden:
            raise GigaAMHipError(f"encp must be [B, T', {self.cfg.joint_hidden}], got {tuple(encp.shape)}")
        return encp, self._dev(enc_len, torch.int32), b, tp

    _aux_streams: Dict[int, Tuple["torch.cuda.Stream", "torch.cuda.Stream", "torch.cuda.Stream"]] = {}
    _aux_lock = threading.Lock()
    ONE_COPY_BYTES = int(os.environ.get("GAM_ONE_COPY_BYTES", str(256 * 1024)))   # decodes up to this size reach the host in one copy (collect); 0: A/B switch

    @classmethod
    def aux_streams(cls, device: torch.device) -> Tuple["torch.cuda.Stream", "torch.cuda.Stream", "torch.cuda.Stream"]:
        """(decode side stream, collect stream, host-to-device copy stream) of a device: three HIGH-priority streams taken from torch's pool in
        one go.  Why (tools/queue_probe.py, profiles/r06_queue_probe.txt): HIP maps streams onto four hardware queues per priority level, round
        robin in creation order, and two streams on one queue SERIALISE -- one normal-priority stream in four lands on the null stream's queue,
        where an "overlapped" decode, the ids' D2H copy or the next batch's H2D copy silently queues behind the encoder it was meant to run
        beside (both / one = 2.00 instead of 1.00).  High-priority streams have their own four queues (never the launch stream's, whatever
        the caller created before), and three taken consecutively are on three different ones.  Same-box A/B of the priority alone: neutral."""
        key = device.index if device.index is not None else torch.cuda.current_device()
        st = cls._aux_streams.get(key)
        if st is None:
            with cls._aux_lock:      # (two threads building their first engine at once must end up with ONE trio)
                st = cls._aux_streams.get(key)
                if st is None:
                    prio = int(os.environ.get("GAM_AUX_STREAM_PRIORITY", "-1"))     # (0: the A/B switch of profiles/r06_queue_probe.txt)
                    st = cls._aux_streams[key] = tuple(torch.cuda.Stream(device, priority=prio) for _ in range(3))
        return st

    @classmethod
    def _collect_stream(cls, device: torch.device) -> "torch.cuda.Stream":
        return cls.aux_streams(device)[1]

    @staticmethod
    def _flag_of(word: int) -> bool:
        """The handle's flag word: bit 0 = a split-fp16 operand left fp16's range (the caller repeats the batch on the exact path);
        bit 1 = gam_encode_varlen was given host lengths SHORTER than the device's (the batch is incomplete: an error, not a fallback)."""
        if int(word) & 2:
            raise GigaAMHipError("encode(host_lengths=...): a host length is shorter than the device length of the same utterance")
        return bool(int(word) & 1)

    @staticmethod
    def collect(dec, frames: Optional[Tensor] = None, counts: Optional[Tensor] = None):
        """``Decoded`` -> ([(ids, frames)] host lists, range_flag).  One blocking D2H for the counts AND the split-fp16 range
        flag accumulated up to this decode, one for the used part of ids / frames, both on a side stream that waits for the
        decode's own completion event only.  Three bare tensors (ids, frames, counts) are accepted for callers that built them
        some other way: a plain blocking copy on the current stream, flag unknown (False)."""
        whole = None
        if isinstance(dec, Decoded):
            ids, frames, counts, ext, evt = dec[0], dec[1], dec[2], dec.ext, dec.event
            whole = getattr(dec, "whole", None)
        else:
            ids, ext, evt = dec, None, None
        src = ext if ext is not None else counts
        if whole is not None and evt is not None and whole.is_cuda and whole.numel() * 4 <= HipEngine.ONE_COPY_BYTES:
            # one blocking D2H of the whole decode (a second and third round trip cost more than the unused tail of ids / frames)
            arr, = _to_host((whole,), evt)      # (zero-copy numpy; the row conversion's timing: _rows)
            h = Decoded.views(Decoded.layout(*ids.shape), arr)
            n = h["ext"].tolist()
            flag = HipEngine._flag_of(n.pop())
            if n and min(n) < 0:
                raise GigaAMHipError("decode left an utterance undecoded (counts = -1)")
            return _rows(h["ids"], h["frames"], n), flag
        # counts (+ flag word) first, then the used columns of ids and of frames: on the collect stream behind the decode's own event, or ...
        side = HipEngine._collect_stream(ids.device) if evt is not None and ids.is_cuda else None
        if side is None and ids.is_cuda:
            # ... bare tensors carry no completion event: the decode may have run on the engine's side stream, which a .cpu() on the
            # CURRENT stream is not ordered behind -- wait for the whole device rather than read half-written counts
            torch.cuda.synchronize(ids.device)
        with contextlib.nullcontext() if side is None else torch.cuda.stream(side):
            if side is not None:
                side.wait_event(evt)
            n = src.cpu().tolist()
            flag = HipEngine._flag_of(n.pop()) if ext is not None else False
            width = max(n) if n else 0
            ids_h, fr_h = ids[:, :width].cpu(), frames[:, :width].cpu()
        if side is not None:
            for t in (ids, frames, src):
                t.record_stream(side)
        if n and min(n) < 0:   # cannot happen: gam_rnnt_greedy repairs failed clusters itself (gam_api.hip rnnt_single_launch)
            raise GigaAMHipError("RNN-T decode left an utterance undecoded (counts = -1)")
        return _rows(ids_h.numpy(), fr_h.numpy(), n), flag

    def feat_frames(self, n_samples: int) -> int:
        return int(self.lib.gam_feat_frames(self._h, n_samples))

    def enc_frames(self, n_feat: int) -> int:
        return int(self.lib.gam_enc_frames(self._h, n_feat))

    # ------------------------------------------------------------------ operators
    def frontend(self, wav: Tensor, length: Tensor) -> Tuple[Tensor, Tensor]:
        wav = self._dev(wav, torch.float32)
        length = self._dev(length, torch.int64)
        b, l = wav.shape
        t = self.feat_frames(l)
        feat = torch.empty((b, self.cfg.n_mels, t), dtype=torch.float32, device=self.device)
        flen = torch.empty((b,), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_frontend(self._h, _ptr(wav), _ptr(length), b, l, _ptr(feat), _ptr(flen), self._stream())
        self._check(rc, "gam_frontend")
        return feat, flen

    def host_feat_lengths(self, wav_lengths) -> Optional[list]:
        """Feature-frame counts of a batch from its sample counts, ON THE HOST (``FeatureExtractor.out_len``, gam_feat_frames) -- what
        ``encode(host_lengths=...)`` wants for a ragged batch.  None when the lengths live on the GPU (reading them would be a host sync)."""
        if isinstance(wav_lengths, Tensor):
            if wav_lengths.is_cuda:
                return None
            wav_lengths = wav_lengths.tolist()
        return [self.feat_frames(int(n)) for n in wav_lengths]

    def last_encode_rows(self) -> Tuple[int, int]:
        """(token rows the layers of the last ``encode`` ran on, rows of the padded layout): equal unless that call packed its rows."""
        pad = C.c_int(0)
        rows = self.lib.gam_last_encode_rows(self._h, C.byref(pad))
        return int(rows), int(pad.value)

    def encode(self, feat: Tensor, length: Tensor, n_layers_run: int = -1, want_tokens: bool = False, host_lengths=None):
        """``host_lengths``: the same feature lengths as ``length`` as host integers (``host_feat_lengths``).  With them a ragged batch's layers
        run on its valid frames only (gam_encode_varlen: packed rows); without them -- or for an equal-length batch -- on B x T'max rows."""
        if host_lengths is None and isinstance(length, Tensor) and not length.is_cuda:
            host_lengths = length.tolist()        # the caller's lengths are on the host anyway
        feat = self._dev(feat, torch.float32)
        length = self._dev(length, torch.int64)
        b, f, t = feat.shape
        if f != self.cfg.feat_in:
            raise GigaAMHipError(f"expected [B,{self.cfg.feat_in},T] features, got {tuple(feat.shape)}")
        tp = self.enc_frames(t)
        enc = torch.empty((b, self.cfg.d_model, tp), dtype=torch.float32, device=self.device)
        elen = torch.empty((b,), dtype=torch.int32, device=self.device)
        tok = torch.empty((b, tp, self.cfg.d_model), dtype=torch.float32, device=self.device) if want_tokens else None
        with torch.cuda.device(self.device):
            if host_lengths is not None and b > 1:
                if len(host_lengths) != b:
                    raise GigaAMHipError(f"host_lengths has {len(host_lengths)} entries for a batch of {b}")
                hl = (C.c_int64 * b)(*[int(v) for v in host_lengths])
                rc = self.lib.gam_encode_varlen(self._h, _ptr(feat), _ptr(length), hl, b, t, _ptr(enc), _ptr(elen), n_layers_run, _ptr(tok),
                                                self._stream())
            elif n_layers_run < 0 and not want_tokens:
                rc = self.lib.gam_encode(self._h, _ptr(feat), _ptr(length), b, t, _ptr(enc), _ptr(elen), self._stream())
            else:
                rc = self.lib.gam_encode_ex(self._h, _ptr(feat), _ptr(length), b, t, _ptr(enc), _ptr(elen),
                                            n_layers_run, _ptr(tok), self._stream())
        self._check(rc, "gam_encode")
        return (enc, elen, tok) if want_tokens else (enc, elen)

    def ctc_head(self, encoded: Tensor) -> Tensor:
        encoded, _, b, tp = self._in_encoded(encoded, None)
        out = torch.empty((b, tp, self.cfg.num_classes), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_ctc_head(self._h, _ptr(encoded), b, tp, _ptr(out), self._stream())
        self._check(rc, "gam_ctc_head")
        return out

    def emo_probs(self, encoded: Tensor, enc_len: Optional[Tensor] = None) -> Tensor:
        """[B,d_model,T'] -> class probabilities [B,num_classes] (mean over time, Linear, softmax);
        enc_len restricts the mean to each utterance's valid frames (None = all T')."""
        encoded, enc_len, b, tp = self._in_encoded(encoded, enc_len)
        out = torch.empty((b, self.cfg.num_classes), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_emo_probs(self._h, _ptr(encoded), _ptr(enc_len), b, tp, _ptr(out), self._stream())
        self._check(rc, "gam_emo_probs")
        return out

    def ctc_greedy(self, encoded: Tensor, enc_len: Tensor) -> Decoded:
        encoded, enc_len, b, tp = self._in_encoded(encoded, enc_len)
        out = Decoded.packed(self.device, b, tp)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_ctc_greedy(self._h, _ptr(encoded), _ptr(enc_len), b, tp, _ptr(out.ids), _ptr(out.frames),
                                         _ptr(out.counts), self._stream())
            self._check(rc, "gam_ctc_greedy")
            return self._finish(out, True)

    def _pad_targets(self, b: int, targets, target_len) -> Tuple[Tensor, Tensor]:
        """targets: [B, Umax] ints or a list of B int lists; target_len [B] (None: the rows' lengths) -> device i32 [B, Umax], [B]."""
        if isinstance(targets, Tensor):
            tgt = targets.reshape(b, -1)
            tlen = torch.full((b,), tgt.shape[1], dtype=torch.int32) if target_len is None else target_len
        else:
            if len(targets) != b:
                raise GigaAMHipError(f"{len(targets)} targets for a batch of {b}")
            um = max([len(t) for t in targets] + [0])
            tgt = torch.zeros((b, um), dtype=torch.int32)
            for i, t in enumerate(targets):
                if len(t):
                    tgt[i, : len(t)] = torch.as_tensor(list(t), dtype=torch.int32)
            tlen = torch.tensor([len(t) for t in targets], dtype=torch.int32) if target_len is None else target_len
        return self._dev(tgt, torch.int32), self._dev(tlen, torch.int32)

    def _launch_align(self, fn, first, enc_len: Tensor, b: int, tp: int, extra, tgt: Tensor, tlen: Tensor, out: Aligned, what: str) -> None:
        rc = fn(self._h, _ptr(first), _ptr(enc_len), b, tp, *extra, _ptr(tgt), _ptr(tlen), out.umax, _ptr(out.frame_labels),
                _ptr(out.tok_first), _ptr(out.tok_last), _ptr(out.score), _ptr(out.loglik), _ptr(out.status), self._stream())
        self._check(rc, what)

    def ctc_star_row(self, log_probs: Tensor, enc_len: Optional[Tensor] = None, penalty: float = math.log(2)) -> Tensor:
        """gam_op_ctc_star_row: the wildcard's emission row ``max_v log_probs[..., v] - penalty`` (f32 on the device) for ``star=`` of
        ``op_ctc_align`` / ``op_ctc_align_long``.  log_probs [B, T', V] with ``enc_len`` [B] -> [B, T'] (0 on the frames past
        ``enc_len``), or [T, V] (one long utterance, every row valid) -> [T].  ``penalty`` >= 0 and finite; no host sync."""
        log_probs = self._dev(log_probs, torch.float32)
        if log_probs.dim() == 2:
            (tp, v), b, enc_len = log_probs.shape, 1, None
            out = torch.empty((tp,), dtype=torch.float32, device=self.device)
        else:
            b, tp, v = log_probs.shape
            enc_len = None if enc_len is None else self._dev(enc_len, torch.int32)
            out = torch.empty((b, tp), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_op_ctc_star_row(self._h, _ptr(log_probs), _ptr(enc_len), b, tp, v, float(penalty),
                                              _ptr(out), self._stream())
        self._check(rc, "gam_op_ctc_star_row")
        return out

    def ctc_align(self, encoded: Tensor, enc_len: Tensor, targets, target_len: Optional[Tensor] = None,
                  star_penalty: Optional[float] = None) -> Aligned:
        """CTC forced alignment of known targets (gam_ctc_align): the CTC head, its log-softmax and the alignment kernel, no host sync.
        ``targets``: i32 [B, Umax] (entries past ``target_len[b]`` are ignored) or a list of B token-id lists.  The split-fp16 range
        flag is CONSUMED as ``ctc_greedy`` does: it lands in the result's last word (``Aligned.host()['flag']``).
        ``star_penalty`` (a float >= 0): gam_ctc_align_star -- target id V (``num_classes``) is a wildcard whose emission is the
        frame's best log-prob minus the penalty; the result holds V on its frames and its run in ``tok_first`` / ``tok_last``."""
        encoded, enc_len, b, tp = self._in_encoded(encoded, enc_len)
        tgt, tlen = self._pad_targets(b, targets, target_len)
        out = Aligned.empty(self.device, b, tp, tgt.shape[1])
        with torch.cuda.device(self.device):
            if star_penalty is None:
                self._launch_align(self.lib.gam_ctc_align, encoded, enc_len, b, tp, (), tgt, tlen, out, "gam_ctc_align")
            else:
                rc = self.lib.gam_ctc_align_star(self._h, _ptr(encoded), _ptr(enc_len), b, tp, _ptr(tgt), _ptr(tlen), out.umax,
                                                 float(star_penalty), _ptr(out.frame_labels), _ptr(out.tok_first), _ptr(out.tok_last),
                                                 _ptr(out.score), _ptr(out.loglik), _ptr(out.status), self._stream())
                self._check(rc, "gam_ctc_align_star")
            return self._finish(out, True)

    def op_ctc_align(self, log_probs: Tensor, enc_len: Tensor, targets, target_len: Optional[Tensor] = None,
                     star: Optional[Tensor] = None) -> Aligned:
        """gam_op_ctc_align: the alignment kernel alone on caller-supplied log-probs [B, T', V] (used as they are).  The result's flag
        word is 0 (no encoder ran).  ``star`` (f32 [B, T'], used as it is; ``ctc_star_row`` makes one): gam_op_ctc_align_star --
        target id V is a wildcard whose emission at frame t is ``star[b, t]``."""
        log_probs, enc_len, b, tp, v = self._in_log_probs(log_probs, enc_len)
        tgt, tlen = self._pad_targets(b, targets, target_len)
        out = Aligned.empty(self.device, b, tp, tgt.shape[1])
        with torch.cuda.device(self.device):
            if star is None:
                self._launch_align(self.lib.gam_op_ctc_align, log_probs, enc_len, b, tp, (v,), tgt, tlen, out, "gam_op_ctc_align")
            else:
                star = self._dev(star, torch.float32)
                if tuple(star.shape) != (b, tp):
                    raise GigaAMHipError(f"star must be [{b}, {tp}], got {tuple(star.shape)}")
                self._launch_align(self.lib.gam_op_ctc_align_star, log_probs, enc_len, b, tp, (v, _ptr(star)), tgt, tlen, out,
                                   "gam_op_ctc_align_star")
            return self._finish(out, False)

    def op_ctc_align_long(self, log_probs: Tensor, targets, consume_flag: bool = False, star: Optional[Tensor] = None) -> AlignedLong:
        """gam_op_ctc_align_long: CTC forced alignment of ONE long utterance, log-probs f32 [T, V] (used as they are) against ``targets``
        (token ids: a list or an i32 tensor [U]), tiled over the whole GPU (gam_align_long.h); no host sync.  ``consume_flag``: move
        the split-fp16 range flag of the encoder runs that produced the log-probs into the result's flag word (as ``ctc_align`` does);
        otherwise the word is 0.  ``star`` (f32 [T], used as it is): gam_op_ctc_align_long_star -- target id V is a wildcard whose
        emission at frame t is ``star[t]``."""
        log_probs = self._dev(log_probs, torch.float32)
        t, v = log_probs.shape
        tgt = self._dev(targets if isinstance(targets, Tensor) else torch.tensor([int(i) for i in targets], dtype=torch.int32),
                        torch.int32).reshape(-1)
        u = tgt.numel()
        out = AlignedLong.empty(self.device, t, u)
        with torch.cuda.device(self.device):
            if star is None:
                rc = self.lib.gam_op_ctc_align_long(self._h, _ptr(log_probs), t, v, _ptr(tgt), u, _ptr(out.frame_labels), _ptr(out.tok_first),
                                                    _ptr(out.tok_last), _ptr(out.score), _ptr(out.loglik), _ptr(out.status), self._stream())
                self._check(rc, "gam_op_ctc_align_long")
            else:
                star = self._dev(star, torch.float32).reshape(-1)
                if star.numel() != t:
                    raise GigaAMHipError(f"star must be [{t}], got {tuple(star.shape)}")
                rc = self.lib.gam_op_ctc_align_long_star(self._h, _ptr(log_probs), t, v, _ptr(star), _ptr(tgt), u, _ptr(out.frame_labels),
                                                         _ptr(out.tok_first), _ptr(out.tok_last), _ptr(out.score), _ptr(out.loglik),
                                                         _ptr(out.status), self._stream())
                self._check(rc, "gam_op_ctc_align_long_star")
            return self._finish(out, consume_flag)

    def op_ctc_stitch(self, log_probs: Tensor, enc_len: Tensor, lo: Tensor, hi: Tensor, dst: Tensor, out: Tensor) -> Tensor:
        """gam_op_ctc_stitch: rows ``lo[b] <= t < min(hi[b], enc_len[b])`` of every utterance of log_probs f32 [B, T', V] go to
        ``out[dst[b] + t - lo[b]]`` (f32 [T_total, V] on the device, written in place), bit for bit; no host sync.  ``lo`` / ``hi`` i32
        [B], ``dst`` i64 [B].  Returns status i32 [B] on the device: 1 where nothing was clipped and the rows fit ``out``."""
        log_probs, enc_len, b, tp, v = self._in_log_probs(log_probs, enc_len)
        lo, hi, dst = self._dev(lo, torch.int32), self._dev(hi, torch.int32), self._dev(dst, torch.int64)
        if not (lo.numel() == hi.numel() == dst.numel() == enc_len.numel() == b):
            raise GigaAMHipError(f"enc_len / lo / hi / dst must hold {b} entries each")
        if (not out.is_cuda or out.device != self.device or out.dtype != torch.float32 or out.dim() != 2 or out.shape[1] != v
                or not out.is_contiguous()):
            raise GigaAMHipError(f"out must be a contiguous f32 [T_total, {v}] tensor on {self.device}")
        status = torch.empty((b,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_op_ctc_stitch(self._h, _ptr(log_probs), _ptr(enc_len), b, tp, v, _ptr(lo), _ptr(hi), _ptr(dst), _ptr(out),
                                            out.shape[0], _ptr(status), self._stream())
        self._check(rc, "gam_op_ctc_stitch")
        return status

    def op_ctc_greedy_long(self, log_probs: Tensor, consume_flag: bool = False) -> Decoded:
        """gam_op_ctc_greedy_long: the CTC greedy decode of ONE utterance of any length, log-probs f32 [T, V] (used as they are),
        spread over the whole GPU (gam_stitch.h); no host sync.  Returns a ``Decoded`` of one row with room for T tokens:
        ``collect`` reads it like any greedy decode.  ``consume_flag``: as ``op_ctc_align_long``."""
        log_probs = self._dev(log_probs, torch.float32)
        t, v = log_probs.shape
        out = Decoded.packed(self.device, 1, t)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_op_ctc_greedy_long(self._h, _ptr(log_probs), t, v, _ptr(out.ids), _ptr(out.frames), _ptr(out.counts),
                                                 self._stream())
            self._check(rc, "gam_op_ctc_greedy_long")
            return self._finish(out, consume_flag)

    def set_ctc_align_workspace(self, nbytes: int = 0) -> None:
        """Bytes of workspace ``op_ctc_align_long`` may take (gam_set_ctc_align_workspace; 0: the default, 3 GiB).  A call that needs
        more is an error that names the needed and the allowed bytes."""
        self._check(self.lib.gam_set_ctc_align_workspace(self._h, int(nbytes)), "gam_set_ctc_align_workspace")

    def tune_ctc_align_long(self, sb: int = 0, tt: int = 0) -> None:
        """Force the tiling of ``op_ctc_align_long`` (gam_tune_ctc_align_long): ``sb`` states per block (a multiple of 64 in
        [64, 3072]), ``tt`` frames per tile (>= 1); 0 = planned.  Process-wide, like ``gam_tune_sp``."""
        if self.lib.gam_tune_ctc_align_long(int(sb), int(tt)) != 0:
            raise GigaAMHipError(f"gam_tune_ctc_align_long: sb={sb} must be 0 or a multiple of 64 in [64, 3072], tt={tt} must be >= 0")

    def rnnt_align(self, encoded: Tensor, enc_len: Tensor, targets, target_len: Optional[Tensor] = None) -> "RnntAligned":
        """Transducer forced alignment of known targets (gam_rnnt_align): the encoder projection, the teacher-forced predictor, the
        fused joint lattice and its sweep, no host sync.  ``targets``: i32 [B, Umax] (entries past ``target_len[b]`` are ignored) or
        a list of B token-id lists.  ``max_symbols_per_step`` does not bound the lattice; hotwords and the LM are not read.  The
        split-fp16 range flag is CONSUMED as ``rnnt_greedy`` does: it lands in the result's last word."""
        encoded, enc_len, b, tp = self._in_encoded(encoded, enc_len)
        tgt, tlen = self._pad_targets(b, targets, target_len)
        out = RnntAligned.empty(self.device, b, tgt.shape[1])
        with torch.cuda.device(self.device):
            rc = self.lib.gam_rnnt_align(self._h, _ptr(encoded), _ptr(enc_len), b, tp, _ptr(tgt), _ptr(tlen), out.umax, _ptr(out.tok_frame),
                                         _ptr(out.score), _ptr(out.loglik), _ptr(out.status), self._stream())
            self._check(rc, "gam_rnnt_align")
            return self._finish(out, True)

    def op_rnnt_align(self, encp: Tensor, enc_len: Tensor, targets, target_len: Optional[Tensor] = None,
                      want_lattice: bool = False) -> "RnntAligned":
        """gam_op_rnnt_align: the same from a caller-supplied encoder projection encp f32 [B, T', joint_hidden], with this engine's
        predictor and joint weights.  ``want_lattice``: also keep the (log P(blank), log P(next token)) lattice the call swept
        (``RnntAligned.lattice``, f32 [B, T', Umax + 1, 2] on the device).  The flag word is 0."""
        encp, enc_len, b, tp = self._in_encp(encp, enc_len)
        tgt, tlen = self._pad_targets(b, targets, target_len)
        out = RnntAligned.empty(self.device, b, tgt.shape[1])
        with torch.cuda.device(self.device):
            if want_lattice:
                out.lattice = torch.empty((b, tp, out.umax + 1, 2), dtype=torch.float32, device=self.device)
            rc = self.lib.gam_op_rnnt_align(self._h, _ptr(encp), _ptr(enc_len), b, tp, _ptr(tgt), _ptr(tlen), out.umax,
                                            _ptr(out.tok_frame), _ptr(out.score), _ptr(out.loglik), _ptr(out.status),
                                            _ptr(out.lattice), self._stream())
            self._check(rc, "gam_op_rnnt_align")
            return self._finish(out, False)

    def op_rnnt_lattice_align(self, lattice: Tensor, enc_len: Tensor, targets, target_len: Optional[Tensor] = None,
                              num_classes: Optional[int] = None) -> "RnntAligned":
        """gam_op_rnnt_lattice_align: the lattice sweep alone on a caller-supplied lattice f32 [B, T', Umax + 1, 2] of
        (log P(blank), log P(next token)), read as it is.  ``num_classes`` (default: large enough for every id >= 0) only serves
        the id check of the status.  The flag word is 0."""
        lattice = self._dev(lattice, torch.float32)
        enc_len = self._dev(enc_len, torch.int32)
        b, tp, u1, two = lattice.shape
        tgt, tlen = self._pad_targets(b, targets, target_len)
        out = RnntAligned.empty(self.device, b, tgt.shape[1])
        if two != 2 or u1 != out.umax + 1:
            raise GigaAMHipError(f"lattice must be [B, T', Umax + 1 = {out.umax + 1}, 2], got {tuple(lattice.shape)}")
        with torch.cuda.device(self.device):
            rc = self.lib.gam_op_rnnt_lattice_align(self._h, _ptr(lattice), _ptr(enc_len), b, tp, int(num_classes or 1025), _ptr(tgt),
                                                    _ptr(tlen), out.umax, _ptr(out.tok_frame), _ptr(out.score), _ptr(out.loglik),
                                                    _ptr(out.status), self._stream())
            self._check(rc, "gam_op_rnnt_lattice_align")
            return self._finish(out, False)

    def set_rnnt_align_workspace(self, nbytes: int = 0) -> None:
        """Bytes of lattice one slice of ``rnnt_align`` / ``op_rnnt_align`` may take (gam_set_rnnt_align_workspace; 0: the default,
        1 GiB).  A batch above it is processed in slices of utterances; one utterance above it is an error."""
        self._check(self.lib.gam_set_rnnt_align_workspace(self._h, int(nbytes)), "gam_set_rnnt_align_workspace")

    # ---- token confidence of a finished decode (gam_confidence.h)
    MEASURES = {"prob": 0, "entropy": 1}
    AGGREGATIONS = {"mean": 0, "min": 1, "prod": 2}
    MAX_RNNT_CONFIDENCE_TOKENS = 1024     # include/gigaam_hip.h gam_rnnt_confidence

    @classmethod
    def _confidence_codes(cls, measure: str, aggregation: str) -> Tuple[int, int]:
        if measure not in cls.MEASURES:
            raise ValueError(f"unknown confidence measure {measure!r} (one of {', '.join(cls.MEASURES)})")
        if aggregation not in cls.AGGREGATIONS:
            raise ValueError(f"unknown confidence aggregation {aggregation!r} (one of {', '.join(cls.AGGREGATIONS)})")
        return cls.MEASURES[measure], cls.AGGREGATIONS[aggregation]

    def _confidence_tokens(self, b: int, decoded, frames, counts, cap_max: Optional[int] = None):
        """``decoded``: a ``Decoded`` / ``BeamDecoded`` (its ids, frames and counts are used where they are), or ids as an i32
        [B, cap] tensor or B int lists with ``frames`` alike (``counts`` None: the rows' lengths / the full width) -> device i32
        ids, frames [B, cap], counts [B].  ``cap_max``: a wider buffer is narrowed to it (a row that holds more gets status 0)."""
        if isinstance(decoded, Decoded):
            ids, frames, counts = decoded[0], decoded[1], decoded[2]
        elif isinstance(decoded, Tensor):
            if frames is None:
                raise GigaAMHipError("token confidence: ids without frames")
            ids = decoded.reshape(b, -1)
            frames = torch.as_tensor(frames).reshape(b, -1)
            if counts is None:
                counts = torch.full((b,), ids.shape[1], dtype=torch.int32)
        else:
            if frames is None or len(decoded) != b or len(frames) != b or any(len(i) != len(f) for i, f in zip(decoded, frames)):
                raise GigaAMHipError(f"token confidence: ids and frames must hold {b} rows of equal lengths")
            cap = max([len(r) for r in decoded] + [0])
            host = torch.zeros((2, b, cap), dtype=torch.int32)
            for i, (r, f) in enumerate(zip(decoded, frames)):
                if len(r):
                    host[0, i, : len(r)] = torch.as_tensor(list(r), dtype=torch.int32)
                    host[1, i, : len(r)] = torch.as_tensor(list(f), dtype=torch.int32)
            ids, frames = host[0], host[1]
            if counts is None:
                counts = torch.tensor([len(r) for r in decoded], dtype=torch.int32)
        if tuple(ids.shape) != tuple(frames.shape) or ids.shape[0] != b:
            raise GigaAMHipError(f"token confidence: ids {tuple(ids.shape)} and frames {tuple(frames.shape)} must both be [{b}, cap]")
        if cap_max is not None and ids.shape[1] > cap_max:
            ids, frames = ids[:, :cap_max], frames[:, :cap_max]
        return self._dev(ids, torch.int32), self._dev(frames, torch.int32), self._dev(torch.as_tensor(counts), torch.int32)

    def ctc_confidence(self, encoded: Tensor, enc_len: Tensor, decoded, frames=None, counts=None, measure: str = "prob",
                       aggregation: str = "mean") -> "Confidence":
        """Token confidences of a finished CTC decode (gam_ctc_confidence): the CTC head, its log-softmax, one pass over the log-probs
        and the span walk, no host sync.  ``decoded``: what ``ctc_greedy`` / ``ctc_beam`` returned, or ids with ``frames`` (and
        ``counts``) as tensors or lists -- e.g. a transcript's ids at ``ctc_align``'s first frames.  ``measure``: "prob" | "entropy";
        ``aggregation`` over a token's span: "mean" | "min" | "prod".  The split-fp16 range flag is CONSUMED as ``ctc_greedy`` does."""
        m, a = self._confidence_codes(measure, aggregation)
        encoded, enc_len, b, tp = self._in_encoded(encoded, enc_len)
        ids, fr, cnt = self._confidence_tokens(b, decoded, frames, counts)
        out = Confidence.empty(self.device, b, ids.shape[1], True)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_ctc_confidence(self._h, _ptr(encoded), _ptr(enc_len), b, tp, _ptr(ids), _ptr(fr), _ptr(cnt), out.cap, m, a,
                                             _ptr(out.conf), _ptr(out.span), _ptr(out.status), self._stream())
            self._check(rc, "gam_ctc_confidence")
            return self._finish(out, True)

    def op_ctc_confidence(self, log_probs: Tensor, enc_len: Tensor, decoded, frames=None, counts=None, measure: str = "prob",
                          aggregation: str = "mean") -> "Confidence":
        """gam_op_ctc_confidence: the same on caller-supplied log-probs [B, T', V] (used as they are).  The flag word is 0."""
        m, a = self._confidence_codes(measure, aggregation)
        log_probs, enc_len, b, tp, v = self._in_log_probs(log_probs, enc_len)
        ids, fr, cnt = self._confidence_tokens(b, decoded, frames, counts)
        out = Confidence.empty(self.device, b, ids.shape[1], True)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_op_ctc_confidence(self._h, _ptr(log_probs), _ptr(enc_len), b, tp, v, _ptr(ids), _ptr(fr), _ptr(cnt), out.cap,
                                                m, a, _ptr(out.conf), _ptr(out.span), _ptr(out.status), self._stream())
            self._check(rc, "gam_op_ctc_confidence")
            return self._finish(out, False)

    def _confidence_long_tokens(self, decoded, frames, count) -> Tuple[Tensor, Tensor, Tensor]:
        """``decoded``: a ``Decoded`` of one row or a ``BeamStreamDecoded`` (their ids, frames and count are used where they are), or
        ids as an i32 tensor or an int list; ``frames`` (a tensor or a list) replaces the result's own, and is needed beside bare
        ids; ``count`` (a device word, or an int) defaults to the ids' length -> device i32 ids, frames [cap], count [1]."""
        if isinstance(decoded, Decoded):
            if decoded.ids.shape[0] != 1:
                raise GigaAMHipError(f"long token confidence: a decode of one utterance, not of {decoded.ids.shape[0]}")
            ids, own, cnt = decoded.ids.reshape(-1), decoded.frames.reshape(-1), decoded.counts
        elif isinstance(decoded, BeamStreamDecoded):
            ids, own, cnt = decoded.ids, decoded.frames, decoded.count
        else:
            ids = (decoded if isinstance(decoded, Tensor) else torch.tensor([int(i) for i in decoded], dtype=torch.int32)).reshape(-1)
            own, cnt = None, None
        if frames is None:
            frames = own
        if frames is None:
            raise GigaAMHipError("long token confidence: ids without frames")
        frames = (frames if isinstance(frames, Tensor) else torch.tensor([int(f) for f in frames], dtype=torch.int32)).reshape(-1)
        if frames.numel() != ids.numel():
            raise GigaAMHipError(f"long token confidence: {ids.numel()} ids and {frames.numel()} frames")
        if count is None:
            count = cnt if cnt is not None else ids.numel()
        count = count.reshape(-1)[:1] if isinstance(count, Tensor) else torch.tensor([int(count)], dtype=torch.int32)
        return self._dev(ids, torch.int32), self._dev(frames, torch.int32), self._dev(count, torch.int32)

    def op_ctc_confidence_long(self, log_probs: Tensor, decoded=None, frames=None, count=None, measure: str = "prob",
                               aggregation: str = "mean", wildcard: bool = False, consume_flag: bool = False) -> "Confidence":
        """gam_op_ctc_confidence_long: the token confidences of ONE utterance of any length, log-probs f32 [T, V] (used as they are);
        no host sync.  ``decoded``: what ``op_ctc_greedy_long`` or ``BeamStream.finish`` returned (read where it lies on the device:
        no round trip), or ids as a tensor or a list with ``frames`` -- for an aligned text ``AlignedLong.tok_first`` -- and ``count``
        (default: the ids' length).  ``wildcard``: id V is the aligners' wildcard -- it bounds its neighbour's span and is itself not
        scored (conf -1, span 0).  Returns a ``Confidence`` of one row; on at most 8192 frames its conf, span and status are
        bit-identical to ``op_ctc_confidence`` with B = 1.  ``consume_flag``: as ``op_ctc_align_long``."""
        m, a = self._confidence_codes(measure, aggregation)
        log_probs = self._dev(log_probs, torch.float32)
        if log_probs.dim() != 2:
            raise GigaAMHipError(f"long token confidence: log_probs must be [T, V], got {tuple(log_probs.shape)}")
        t, v = log_probs.shape
        ids, fr, cnt = self._confidence_long_tokens(decoded, frames, count)
        out = Confidence.empty(self.device, 1, ids.numel(), True)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_op_ctc_confidence_long(self._h, _ptr(log_probs), t, v, _ptr(ids), _ptr(fr), _ptr(cnt), out.cap, m, a,
                                                     1 if wildcard else 0, _ptr(out.conf), _ptr(out.span), _ptr(out.status), self._stream())
            self._check(rc, "gam_op_ctc_confidence_long")
            return self._finish(out, consume_flag)

    def rnnt_confidence(self, encoded: Tensor, enc_len: Tensor, decoded, frames=None, counts=None, measure: str = "prob") -> "Confidence":
        """Token confidences of a finished RNN-T decode (gam_rnnt_confidence): the encoder projection, the teacher-forced predictor
        over the decoded ids and the joint at the nodes (frames[u], ids[:u]) the tokens were emitted from, no host sync.  ``decoded``:
        what ``rnnt_greedy`` / ``rnnt_beam`` returned, or ids with ``frames`` (and ``counts``) -- e.g. a transcript's ids at
        ``rnnt_align``'s frames.  At most 1024 tokens per utterance: a wider decode buffer is read up to there, and an utterance
        that holds more gets status 0.  The split-fp16 range flag is CONSUMED as ``rnnt_greedy`` does."""
        m, _ = self._confidence_codes(measure, "mean")
        encoded, enc_len, b, tp = self._in_encoded(encoded, enc_len)
        ids, fr, cnt = self._confidence_tokens(b, decoded, frames, counts, self.MAX_RNNT_CONFIDENCE_TOKENS)
        out = Confidence.empty(self.device, b, ids.shape[1], False)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_rnnt_confidence(self._h, _ptr(encoded), _ptr(enc_len), b, tp, _ptr(ids), _ptr(fr), _ptr(cnt), out.cap, m,
                                              _ptr(out.conf), _ptr(out.status), self._stream())
            self._check(rc, "gam_rnnt_confidence")
            return self._finish(out, True)

    def op_rnnt_confidence(self, encp: Tensor, enc_len: Tensor, decoded, frames=None, counts=None, measure: str = "prob") -> "Confidence":
        """gam_op_rnnt_confidence: the same from a caller-supplied encoder projection encp f32 [B, T', joint_hidden], with this engine's
        predictor and joint weights.  The flag word is 0."""
        m, _ = self._confidence_codes(measure, "mean")
        encp, enc_len, b, tp = self._in_encp(encp, enc_len)
        ids, fr, cnt = self._confidence_tokens(b, decoded, frames, counts, self.MAX_RNNT_CONFIDENCE_TOKENS)
        out = Confidence.empty(self.device, b, ids.shape[1], False)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_op_rnnt_confidence(self._h, _ptr(encp), _ptr(enc_len), b, tp, _ptr(ids), _ptr(fr), _ptr(cnt), out.cap, m,
                                                 _ptr(out.conf), _ptr(out.status), self._stream())
            self._check(rc, "gam_op_rnnt_confidence")
            return self._finish(out, False)

    MAX_BEAM = 32     # include/gigaam_hip.h gam_ctc_beam

    MAX_SYMBOLS_BEAM = 16     # include/gigaam_hip.h gam_rnnt_beam

    def _check_beam(self, beam_size: int, max_symbols: Optional[int] = None, n_best: Optional[int] = None) -> None:
        """The beam width, ``n_best`` of an N-best search and ``max_symbols`` of an RNN-T search, each where it is given."""
        if not 1 <= int(beam_size) <= self.MAX_BEAM:
            raise GigaAMHipError(f"beam_size {beam_size} outside [1, {self.MAX_BEAM}]")
        if n_best is not None and not 1 <= int(n_best) <= int(beam_size):
            raise GigaAMHipError(f"n_best {n_best} outside [1, beam_size = {beam_size}]")
        if max_symbols is not None and not 1 <= int(max_symbols) <= self.MAX_SYMBOLS_BEAM:
            raise GigaAMHipError(f"max_symbols {max_symbols} outside [1, {self.MAX_SYMBOLS_BEAM}] for the RNN-T beam search")

    def _beam_out(self, b: int, cap: int, beam_size: int, max_symbols: Optional[int] = None) -> BeamDecoded:
        """Check the width (and the RNN-T search's ``max_symbols``); the result buffers for ``cap`` tokens per utterance."""
        self._check_beam(beam_size, max_symbols)
        return BeamDecoded.empty(self.device, b, cap)

    def _launch_beam(self, fn, first, enc_len: Tensor, b: int, tp: int, extra, beam_size: int, what: str) -> BeamDecoded:
        out = self._beam_out(b, tp, beam_size)
        rc = fn(self._h, _ptr(first), _ptr(enc_len), b, tp, *extra, int(beam_size), _ptr(out.ids), _ptr(out.frames), _ptr(out.counts),
                _ptr(out.score), _ptr(out.logp), self._stream())
        self._check(rc, what)
        return out

    def ctc_beam(self, encoded: Tensor, enc_len: Tensor, beam_size: int) -> BeamDecoded:
        """CTC prefix beam search (gam_ctc_beam): the CTC head, its log-softmax and the beam kernel, no host sync; the hotword set of
        ``set_hotwords`` applies.  The split-fp16 range flag is CONSUMED as ``ctc_greedy`` does: it lands in the flag word."""
        encoded, enc_len, b, tp = self._in_encoded(encoded, enc_len)
        with torch.cuda.device(self.device):
            return self._finish(self._launch_beam(self.lib.gam_ctc_beam, encoded, enc_len, b, tp, (), beam_size, "gam_ctc_beam"), True)

    def op_ctc_beam(self, log_probs: Tensor, enc_len: Tensor, beam_size: int) -> BeamDecoded:
        """gam_op_ctc_beam: the beam kernel alone on caller-supplied log-probs [B, T', V] (used as they are).  The flag word is 0."""
        log_probs, enc_len, b, tp, v = self._in_log_probs(log_probs, enc_len)
        with torch.cuda.device(self.device):
            return self._finish(self._launch_beam(self.lib.gam_op_ctc_beam, log_probs, enc_len, b, tp, (v,), beam_size, "gam_op_ctc_beam"), False)

    def rnnt_beam(self, encoded: Tensor, enc_len: Tensor, beam_size: int, max_symbols: int) -> BeamDecoded:
        """RNN-T beam search (gam_rnnt_beam): the encoder projection GEMM and the beam kernel, no host sync; the hotword set of
        ``set_hotwords`` and the LM of ``set_lm`` apply.  ids / frames are [B, T' * max_symbols].  The split-fp16 range flag is
        CONSUMED as ``rnnt_greedy`` does: it lands in the flag word."""
        encoded, enc_len, b, tp = self._in_encoded(encoded, enc_len)
        with torch.cuda.device(self.device):
            out = self._beam_out(b, tp * int(max_symbols), beam_size, max_symbols)
            rc = self.lib.gam_rnnt_beam(self._h, _ptr(encoded), _ptr(enc_len), b, tp, int(beam_size), int(max_symbols), _ptr(out.ids),
                                        _ptr(out.frames), _ptr(out.counts), _ptr(out.score), _ptr(out.logp), self._stream())
            self._check(rc, "gam_rnnt_beam")
            return self._finish(out, True)

    def op_rnnt_beam(self, encp: Tensor, enc_len: Tensor, beam_size: int, max_symbols: int) -> BeamDecoded:
        """gam_op_rnnt_beam: the beam kernel alone on a caller-supplied encoder projection encp f32 [B, T', joint_hidden], with this
        engine's predictor and joint weights (and the hotwords / LM set on it).  The flag word is 0."""
        encp, enc_len, b, tp = self._in_encp(encp, enc_len)
        with torch.cuda.device(self.device):
            out = self._beam_out(b, tp * int(max_symbols), beam_size, max_symbols)
            rc = self.lib.gam_op_rnnt_beam(self._h, _ptr(encp), _ptr(enc_len), b, tp, int(beam_size), int(max_symbols), _ptr(out.ids),
                                           _ptr(out.frames), _ptr(out.counts), _ptr(out.score), _ptr(out.logp), self._stream())
            self._check(rc, "gam_op_rnnt_beam")
            return self._finish(out, False)

    def _nbest_out(self, b: int, cap: int, beam_size: int, n_best: int, max_symbols: Optional[int] = None) -> NBestDecoded:
        """Check the width, ``n_best`` (and the RNN-T search's ``max_symbols``); the result buffers for ``n_best`` hypotheses of ``cap``
        tokens per utterance."""
        self._check_beam(beam_size, max_symbols, n_best)
        return NBestDecoded.empty(self.device, b, int(n_best), cap)

    def _launch_nbest(self, fn, what: str, first: Tensor, enc_len: Tensor, b: int, tp: int, extra, out: NBestDecoded, op: bool) -> NBestDecoded:
        rc = fn(self._h, _ptr(first), _ptr(enc_len), b, tp, *extra, out.n, _ptr(out.ids), _ptr(out.frames), _ptr(out.counts),
                _ptr(out.score), _ptr(out.logp), _ptr(out.n_hyp), self._stream())
        self._check(rc, what)
        return self._finish(out, not op)

    def ctc_beam_nbest(self, encoded: Tensor, enc_len: Tensor, beam_size: int, n_best: int) -> NBestDecoded:
        """``ctc_beam`` returning the ``n_best`` (<= ``beam_size``) best prefixes of each final beam (gam_ctc_beam_nbest), no host
        sync; hypothesis 0 is ``ctc_beam``'s result bit for bit.  The range flag lands in the flag word, as in ``ctc_beam``."""
        encoded, enc_len, b, tp = self._in_encoded(encoded, enc_len)
        with torch.cuda.device(self.device):
            out = self._nbest_out(b, tp, beam_size, n_best)
            return self._launch_nbest(self.lib.gam_ctc_beam_nbest, "gam_ctc_beam_nbest", encoded, enc_len, b, tp, (int(beam_size),), out, False)

    def op_ctc_beam_nbest(self, log_probs: Tensor, enc_len: Tensor, beam_size: int, n_best: int) -> NBestDecoded:
        """gam_op_ctc_beam_nbest: the N-best beam kernel alone on caller-supplied log-probs [B, T', V].  The flag word is 0."""
        log_probs, enc_len, b, tp, v = self._in_log_probs(log_probs, enc_len)
        with torch.cuda.device(self.device):
            out = self._nbest_out(b, tp, beam_size, n_best)
            return self._launch_nbest(self.lib.gam_op_ctc_beam_nbest, "gam_op_ctc_beam_nbest", log_probs, enc_len, b, tp,
                                      (v, int(beam_size)), out, True)

    def rnnt_beam_nbest(self, encoded: Tensor, enc_len: Tensor, beam_size: int, max_symbols: int, n_best: int) -> NBestDecoded:
        """``rnnt_beam`` returning the ``n_best`` (<= ``beam_size``) best hypotheses of each final beam (gam_rnnt_beam_nbest), no host
        sync; hypothesis 0 is ``rnnt_beam``'s result bit for bit.  ids / frames are [B, n_best, T' * max_symbols]."""
        encoded, enc_len, b, tp = self._in_encoded(encoded, enc_len)
        with torch.cuda.device(self.device):
            out = self._nbest_out(b, tp * int(max_symbols), beam_size, n_best, max_symbols)
            return self._launch_nbest(self.lib.gam_rnnt_beam_nbest, "gam_rnnt_beam_nbest", encoded, enc_len, b, tp,
                                      (int(beam_size), int(max_symbols)), out, False)

    def op_rnnt_beam_nbest(self, encp: Tensor, enc_len: Tensor, beam_size: int, max_symbols: int, n_best: int) -> NBestDecoded:
        """gam_op_rnnt_beam_nbest: the N-best beam kernel alone on a caller-supplied encoder projection encp f32 [B, T', joint_hidden],
        as ``op_rnnt_beam``.  The flag word is 0."""
        encp, enc_len, b, tp = self._in_encp(encp, enc_len)
        with torch.cuda.device(self.device):
            out = self._nbest_out(b, tp * int(max_symbols), beam_size, n_best, max_symbols)
            return self._launch_nbest(self.lib.gam_op_rnnt_beam_nbest, "gam_op_rnnt_beam_nbest", encp, enc_len, b, tp,
                                      (int(beam_size), int(max_symbols)), out, True)

    @staticmethod
    def _flat_phrases(phrases):
        """Token-id lists -> (all tokens end to end, the first token of every phrase + the total) as C i32 arrays."""
        flat = [c for p in phrases for c in p]
        offs = [0]
        for p in phrases:
            offs.append(offs[-1] + len(p))
        return (C.c_int32 * max(len(flat), 1))(*flat), (C.c_int32 * len(offs))(*offs)

    def set_hotwords(self, phrases, boost: float = 2.0) -> None:
        """Hotword phrases (token-id lists) for the beam search, each matched token worth ``boost`` (gam_set_hotwords); an empty
        list clears the set.  Re-uploads only when the set or the boost changed; a setup call that waits for in-flight decodes."""
        key = (tuple(tuple(int(c) for c in p) for p in phrases), float(boost))
        prev = getattr(self, "_hotwords_key", None)
        if key == prev or (not key[0] and (prev is None or not prev[0])):     # (no set and none uploaded: nothing to clear)
            return
        tok, off = self._flat_phrases(key[0])
        self._check(self.lib.gam_set_hotwords(self._h, tok, off, len(key[0]), C.c_float(key[1])), "gam_set_hotwords")
        self._hotwords_key = key

    # ---- keyword search (gam_kws.h)
    MAX_KEYWORD_TOKENS, MAX_KEYWORDS, MAX_KEYWORD_HITS = 64, 4096, 64     # include/gigaam_hip.h gam_set_keywords / gam_ctc_kws

    def set_keywords(self, keywords, min_score) -> None:
        """The keyword set of ``ctc_kws`` / ``op_ctc_kws`` (gam_set_keywords): token-id lists and, per keyword, the lowest score a
        frame may have to count as the end of an occurrence (finite, <= 0; one float for all keywords is accepted).  An empty list
        clears the set.  Re-uploads only when the set or the scores changed; a setup call that waits for in-flight decodes."""
        kws = tuple(tuple(int(c) for c in p) for p in keywords)
        ms = np.broadcast_to(np.asarray(min_score, dtype=np.float32), (len(kws),)) if kws else np.zeros((0,), np.float32)
        key = (kws, ms.tobytes())
        prev = getattr(self, "_keywords_key", None)
        if key == prev or (not kws and (prev is None or not prev[0])):     # (no set and none uploaded: nothing to clear)
            return
        tok, off = self._flat_phrases(kws)
        msc = (C.c_float * max(len(kws), 1))(*ms.tolist())
        self._check(self.lib.gam_set_keywords(self._h, tok, off, len(kws), msc), "gam_set_keywords")
        self._keywords_key = key

    def _kws_out(self, b: int, tp: int, max_hits: int, dense: bool) -> KeywordHits:
        key = getattr(self, "_keywords_key", None)
        k = len(key[0]) if key else 0
        ds = torch.empty((b, k, tp), dtype=torch.float32, device=self.device) if dense else None
        dst = torch.empty((b, k, tp), dtype=torch.int32, device=self.device) if dense else None
        # (no set, or max_hits outside [1, 64]: the library's errors)
        return KeywordHits.empty(self.device, b, k, int(max_hits), dense_score=ds, dense_start=dst)

    def ctc_kws(self, encoded: Tensor, enc_len: Tensor, max_hits: int = 8, dense: bool = False) -> KeywordHits:
        """Keyword search on the encoder output (gam_ctc_kws): the CTC head, its log-softmax and the search kernels, no host sync;
        the set of ``set_keywords`` is searched in every utterance.  ``dense``: also return the per-frame scores and starts.  The
        split-fp16 range flag is CONSUMED as ``ctc_align`` does: it lands in the result's last word (``KeywordHits.host()['flag']``)."""
        encoded, enc_len, b, tp = self._in_encoded(encoded, enc_len)
        out = self._kws_out(b, tp, max_hits, dense)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_ctc_kws(self._h, _ptr(encoded), _ptr(enc_len), b, tp, out.max_hits, _ptr(out.hit_frames), _ptr(out.hit_score),
                                      _ptr(out.n_hits), _ptr(out.dense_score), _ptr(out.dense_start), self._stream())
            self._check(rc, "gam_ctc_kws")
            return self._finish(out, True)

    def op_ctc_kws(self, log_probs: Tensor, enc_len: Tensor, max_hits: int = 8, dense: bool = False) -> KeywordHits:
        """gam_op_ctc_kws: the search kernels alone on caller-supplied log-probs [B, T', V] (used as they are).  The result's flag word
        is 0 (no encoder ran)."""
        log_probs, enc_len, b, tp, v = self._in_log_probs(log_probs, enc_len)
        out = self._kws_out(b, tp, max_hits, dense)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_op_ctc_kws(self._h, _ptr(log_probs), _ptr(enc_len), b, tp, v, out.max_hits, _ptr(out.hit_frames),
                                         _ptr(out.hit_score), _ptr(out.n_hits), _ptr(out.dense_score), _ptr(out.dense_start),
                                         self._stream())
            self._check(rc, "gam_op_ctc_kws")
            return self._finish(out, False)

    MAX_KEYWORD_STREAM_HITS = 4096     # include/gigaam_hip.h gam_op_ctc_kws_stream
    KWS_STATE_WORDS = 272              # gam_kws.h GAM_KWS_ST_WORDS: gam_ctc_kws_state_bytes / (4 K)

    def op_ctc_kws_stream(self, log_probs: Optional[Tensor], v: int, t_base: int, flags: int, state: Tensor, out: KeywordStreamHits,
                          dense: bool = False):
        """gam_op_ctc_kws_stream as it is, on the current stream: rows ``log_probs`` f32 [n, V] (None: n = 0) are stream frames
        ``t_base`` .., ``flags`` of ``KeywordStream.BEGIN`` / ``END``, ``state`` the i32 buffer of gam_ctc_kws_state_bytes, ``out`` the
        stream's hit arrays.  ``dense``: returns (dense_score f32, dense_start i32) [K, n].  ``KeywordStream`` is the caller that
        keeps ``t_base`` and the flags right."""
        n = 0 if log_probs is None else int(log_probs.shape[0])
        # The library launches a wave per keyword of the set AT HAND and cannot see how large the caller's buffers are: buffers made
        # for a set of another size would be read and written out of bounds, so that is refused here, before any launch.  (A set of the
        # same size but other content is the kernel's refusal: status 0.  No set at all is the library's error.)
        key = getattr(self, "_keywords_key", None)
        k_now = len(key[0]) if key else 0
        if k_now and (out.k != k_now or state.numel() != k_now * self.KWS_STATE_WORDS):
            raise GigaAMHipError(f"keyword stream: the state and the hit arrays were made for {out.k} keywords, the set at hand has {k_now} "
                                 "(set_keywords was called with another set since kws_stream(); make a new stream)")
        ds = torch.empty((out.k, n), dtype=torch.float32, device=self.device) if dense else None
        dst = torch.empty((out.k, n), dtype=torch.int32, device=self.device) if dense else None
        rc = self.lib.gam_op_ctc_kws_stream(self._h, _ptr(log_probs if n else None), n, int(v), int(t_base), int(flags), _ptr(state),
                                            out.max_hits, _ptr(out.hit_frames), _ptr(out.hit_score), _ptr(out.n_hits), _ptr(out.status),
                                            _ptr(ds), _ptr(dst), self._stream())
        self._check(rc, "gam_op_ctc_kws_stream")
        return (ds, dst) if dense else None

    def kws_stream(self, max_hits: int = 8) -> KeywordStream:
        """A resumable keyword search over one stream of any length (gam_op_ctc_kws_stream) for the set of ``set_keywords``: feed it
        with ``push``, end it with ``finish``.  Its buffers are sized for the set at hand NOW.  After ``set_keywords`` with a set of another
        size every call of the stream raises ``GigaAMHipError`` before anything is launched; with another set of the same size the kernel
        refuses the calls (status 0, ``host()`` raises)."""
        return KeywordStream(self, max_hits)

    BEAM_STREAM_REBASE = 1024      # gam_beam_stream.h GAM_BEAM_STREAM_REBASE

    def op_ctc_beam_stream(self, log_probs: Optional[Tensor], v: int, t_base: int, flags: int, beam_size: int, state: Tensor,
                           out: BeamStreamDecoded) -> None:
        """gam_op_ctc_beam_stream as it is, on the current stream: rows ``log_probs`` f32 [n, V] (None: n = 0) are stream frames
        ``t_base`` .., ``flags`` of ``BeamStream.BEGIN`` / ``END``, ``state`` the i32 buffer of gam_ctc_beam_stream_bytes, ``out`` the
        stream's result.  ``BeamStream`` is the caller that keeps ``t_base`` and the flags right."""
        n = 0 if log_probs is None else int(log_probs.shape[0])
        # The library sizes the node pool -- and with it how many tokens the END call may write -- from the state's bytes and this W:
        # it is told no more bytes than ``out.max_frames`` frames take, so that ids / frames [max_frames] hold whatever it writes.
        nbytes = state.numel() * 4
        if 1 <= int(beam_size) <= self.MAX_BEAM:
            nbytes = min(nbytes, int(self.lib.gam_ctc_beam_stream_bytes(self._h, int(beam_size), out.max_frames)))
        rc = self.lib.gam_op_ctc_beam_stream(self._h, _ptr(log_probs if n else None), n, int(v), int(t_base), int(flags), int(beam_size),
                                             _ptr(state), nbytes, _ptr(out.ids), _ptr(out.frames), _ptr(out.count), _ptr(out.score),
                                             _ptr(out.logp), _ptr(out.status), self._stream())
        self._check(rc, "gam_op_ctc_beam_stream")

    def beam_stream(self, beam_size: int, max_frames: int) -> BeamStream:
        """A resumable CTC prefix beam search over one stream of at most ``max_frames`` frames (gam_op_ctc_beam_stream), with the
        hotwords of ``set_hotwords`` and the LM of ``set_lm``: feed it with ``push``, end it with ``finish``.  After a later
        ``set_hotwords`` / ``set_lm`` the kernel refuses the stream's calls (status 0, ``host()`` raises)."""
        return BeamStream(self, beam_size, max_frames)

    def _beam_stream_v(self) -> int:
        """The V of a beam stream's END call when no row was pushed: the LM's, else the head's, else any the hotword ids fit."""
        if getattr(self, "_lm_key", None) is not None:
            return self._lm_v
        if int(self.cfg.num_classes) >= 2:
            return int(self.cfg.num_classes)
        key = getattr(self, "_hotwords_key", None)
        return max((max(p) for p in key[0]), default=0) + 2 if key else 2

    def set_lm(self, lm=None, tokenizer=None, weight: float = 0.5, word_bonus: float = 1.0) -> None:
        """An n-gram LM (``lm.NgramLM``) for the beam search, its words spelt by ``tokenizer`` (gam_set_lm); None clears it.
        Re-uploads only when the model, the tokenizer or a parameter changed; a setup call that waits for in-flight decodes."""
        key = None if lm is None else (id(lm), id(tokenizer), float(weight), float(word_bonus), lm.unk_logp)
        prev = getattr(self, "_lm_key", None)
        if key == prev:
            return
        if lm is None:
            rc = self.lib.gam_set_lm(self._h, None, 0, None, 0, 0, None, 0, 0, 0, 0, 0, 0, C.c_float(0), C.c_float(0), C.c_float(0))
        else:
            t = lm.device_tables(tokenizer)
            cls = np.ascontiguousarray(t["classes"], dtype=np.int32)
            self._lm_v = int(cls.shape[0])
            wt, ng = np.ascontiguousarray(t["words"]), np.ascontiguousarray(t["ngrams"])
            rc = self.lib.gam_set_lm(self._h, cls.ctypes.data, int(cls.shape[0]), wt.ctypes.data, int(wt.shape[0]), int(t["word_probe"]),
                                     ng.ctypes.data, int(ng.shape[0]), int(t["ngram_probe"]), int(lm.order), int(lm.bos), int(lm.eos),
                                     int(lm.unk), C.c_float(lm.unk_logp), C.c_float(weight), C.c_float(word_bonus))
        self._check(rc, "gam_set_lm")
        self._lm_key, self._lm_ref = key, (lm, tokenizer)     # (the references keep the ids of the key unique)

    def set_rnnt_cluster(self, n: int) -> None:
        """Workgroups per utterance of the cluster decode kernel (gam_set_rnnt_cluster): -1 auto, 0 one-workgroup kernel, 1..8."""
        self._check(self.lib.gam_set_rnnt_cluster(self._h, int(n)), "gam_set_rnnt_cluster")
        self._rnnt_cluster_user = int(n)

    def rnnt_last_decode(self) -> Tuple[int, int, bool]:
        """What the last ``rnnt_greedy`` launched (gam_rnnt_last_decode): (C used -- 0 = the one-workgroup kernel, index of the
        cluster kernel's instantiation or -1, whether the runtime refused the cluster launch)."""
        out = (C.c_int32 * 3)()
        self._check(self.lib.gam_rnnt_last_decode(self._h, out), "gam_rnnt_last_decode")
        return int(out[0]), int(out[1]), bool(out[2])

    def _decode_side_stream(self) -> "torch.cuda.Stream":
        return self.aux_streams(self.device)[0]      # (shared by the engines of a device: see aux_streams)

    @staticmethod
    def side_cluster(b: int, side_cus: int) -> int:
        """Cluster size of an OVERLAPPED decode: the clusters of ``b`` utterances (8 utterance columns x ceil(b / 8) rows x C
        workgroups, one per CU -- gam_api.hip) together hold at most ``side_cus`` compute units; at least 1."""
        if "GAM_DEBUG_SIDE_CLUSTER" in os.environ:      # debug: force the overlapped decode's cluster size (0 = one-workgroup kernel)
            return int(os.environ["GAM_DEBUG_SIDE_CLUSTER"])
        return max(1, min(8, side_cus // (8 * ((b + 7) // 8))))

    def rnnt_greedy(self, encoded: Tensor, enc_len: Tensor, max_symbols: int, dump_cap: int = 0, overlap: bool = False,
                    side_cus: int = 0) -> Decoded:
        """RNNTGreedyDecoding.decode on the device (gam_rnnt_greedy).  ``overlap``: launch it on this engine's decode SIDE stream
        with small clusters (at most ``side_cus`` CUs held; 0 = by vocabulary: 96 for a char head, 160 where W_out is streamed
        from L2 -- measured on configs 3 / 4, profiles/r05_ab_experiments.txt), ordered behind everything enqueued on the current stream so far, and
        return at once -- the caller's next ``frontend`` / ``encode`` on the current stream then runs BESIDE this decode instead of
        behind it (the greedy loop is latency-bound: with the GPU to itself it keeps ~224 CUs resident and idle).
        The range flag is fetched on the CURRENT stream first, so it covers exactly this batch's frontend + encoder (fetched on
        the side stream it would swallow a flag the next batch's encoder sets meanwhile).  Same kernels; ids are bit-identical to a serial decode
        AT THE SAME CLUSTER SIZE (tests/test_hip_hardening.py).  The cluster size fixes how a member's sums are partitioned, so a decode with
        small clusters may resolve a near-tie (top-1 / top-2 margin below ~1e-5) differently from the full-size clusters' -- inside the 1e-3 logit
        bar, and the reason bench.py and the tests compare overlapped and serial decodes at equal cluster size.  Decode-class calls of one handle
        are ordered by the library whatever streams they run on (gam_api.hip DecodeScope)."""
        encoded, enc_len, b, tp = self._in_encoded(encoded, enc_len)
        cap = tp * max_symbols
        main = torch.cuda.current_stream(self.device)
        side = self._decode_side_stream() if overlap else None
        # ids | frames | counts + flag word as views of ONE buffer (allocated on the launch stream): a small decode reaches the host in one copy
        ids, frames, counts = out = Decoded.packed(self.device, b, cap)
        whole, word = out.whole, out.flag_word()
        if overlap:
            with torch.cuda.device(self.device):
                self._fetch_flag(word)           # on the launch stream: this batch's own flag (its event is not the decode's)
            side.wait_stream(main)
            c_side = self.side_cluster(b, side_cus if side_cus > 0 else (96 if self.cfg.num_classes <= 64 else 160))
            self._check(self.lib.gam_set_rnnt_cluster(self._h, c_side), "gam_set_rnnt_cluster")     # (for this call only: restored below)
        try:
            with torch.cuda.stream(side) if overlap else torch.cuda.device(self.device):
                dump = dcount = None
                if dump_cap > 0:
                    dump = torch.zeros((b, dump_cap, self.cfg.num_classes), dtype=torch.float32, device=self.device)
                    dcount = torch.zeros((b,), dtype=torch.int32, device=self.device)
                rc = self.lib.gam_rnnt_greedy(self._h, _ptr(encoded), _ptr(enc_len), b, tp, max_symbols, _ptr(ids),
                                              _ptr(frames), _ptr(counts), _ptr(dump), _ptr(dcount), dump_cap, self._stream())
                self._check(rc, "gam_rnnt_greedy")
                if overlap:
                    st = torch.cuda.current_stream(self.device)
                    evt = torch.cuda.Event()
                    evt.record(st)
                    for t in (encoded, enc_len, whole):    # allocated on the launch stream, last used on the side stream
                        t.record_stream(st)
                else:
                    evt, st = self._fetch_flag(word)
        finally:
            if overlap:
                self._check(self.lib.gam_set_rnnt_cluster(self._h, self._rnnt_cluster_user), "gam_set_rnnt_cluster")
        return Decoded(ids, frames, counts, out.ext, evt, st, dump, dcount, whole=whole)

    def rnnt_encp(self, encoded: Tensor) -> Tensor:
        """[B, d_model, T'] -> the encoder half of the joint, encp f32 [B, T', joint_hidden] = W_enc f + b_enc (gam_rnnt_encp: the
        projection GEMM ``rnnt_greedy`` runs): what the ``op_rnnt_*`` calls and ``RnntGreedyStream.push`` take.  The RNN-T twin of
        ``ctc_head``; no host sync."""
        encoded, _, b, tp = self._in_encoded(encoded, None)
        out = torch.empty((b, tp, int(self.cfg.joint_hidden)), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_rnnt_encp(self._h, _ptr(encoded), b, tp, _ptr(out), self._stream())
        self._check(rc, "gam_rnnt_encp")
        return out

    def op_rnnt_greedy(self, encp: Tensor, enc_len: Tensor, max_symbols: int) -> Decoded:
        """gam_op_rnnt_greedy: ``rnnt_greedy`` from a caller-supplied encoder projection encp f32 [B, T', joint_hidden], on the current
        stream: the same plan (the cluster setting is honoured, the repair pass runs), no logits dump.  The flag word is 0."""
        encp, enc_len, b, tp = self._in_encp(encp, enc_len)
        out = Decoded.packed(self.device, b, tp * int(max_symbols))
        with torch.cuda.device(self.device):
            rc = self.lib.gam_op_rnnt_greedy(self._h, _ptr(encp), _ptr(enc_len), b, tp, int(max_symbols), _ptr(out.ids), _ptr(out.frames),
                                             _ptr(out.counts), self._stream())
            self._check(rc, "gam_op_rnnt_greedy")
            return self._finish(out, False)

    def op_rnnt_greedy_stream(self, encp_rows: Optional[Tensor], t_base: int, flags: int, max_symbols: int, state: Tensor,
                              state_bytes: int, out: Decoded, status: Tensor, cap: Optional[int] = None) -> None:
        """gam_op_rnnt_greedy_stream as it is, on the current stream: rows ``encp_rows`` f32 [n, joint_hidden] (None: n = 0) are stream
        frames ``t_base`` .., ``flags`` of ``RnntGreedyStream.BEGIN`` / ``END``, ``state`` the buffer of gam_rnnt_greedy_stream_bytes
        (``state_bytes`` of it are the record), ``out`` a one-row ``Decoded`` (``cap``: how many of its columns the library may
        use, default all), ``status`` i32 [1].  ``RnntGreedyStream`` is the caller that keeps ``t_base`` and the flags right."""
        n = 0 if encp_rows is None else int(encp_rows.shape[0])
        cap = int(out.ids.shape[1]) if cap is None else min(int(cap), int(out.ids.shape[1]))
        rc = self.lib.gam_op_rnnt_greedy_stream(self._h, _ptr(encp_rows if n else None), n, int(t_base), int(flags), int(max_symbols),
                                                _ptr(state), int(state_bytes), _ptr(out.ids), _ptr(out.frames), cap, _ptr(out.counts),
                                                _ptr(status), self._stream())
        self._check(rc, "gam_op_rnnt_greedy_stream")

    def rnnt_greedy_stream(self, max_frames: int, max_symbols: int) -> RnntGreedyStream:
        """A resumable RNN-T greedy decode over one stream of at most ``max_frames`` frames (gam_op_rnnt_greedy_stream): feed it rows
        of ``rnnt_encp`` with ``push``, end it with ``finish``.  One workgroup, the one-workgroup kernel's arithmetic (cluster size 0);
        the predictor's state is carried from call to call, so the stream is decoded as ONE utterance wherever it is cut."""
        return RnntGreedyStream(self, max_frames, max_symbols)

    RNNT_BEAM_STREAM_REBASE = 256      # gam_rnnt_beam.h GAM_RB_STREAM_REBASE

    def op_rnnt_beam_stream(self, encp_rows: Optional[Tensor], t_base: int, flags: int, beam_size: int, max_symbols: int, state: Tensor,
                            state_bytes: int, out: BeamStreamDecoded, cap: Optional[int] = None) -> None:
        """gam_op_rnnt_beam_stream as it is, on the current stream: rows ``encp_rows`` f32 [n, joint_hidden] (None: n = 0) are stream
        frames ``t_base`` .., ``flags`` of ``RnntBeamStream.BEGIN`` / ``END``, ``state`` the i32 buffer of gam_rnnt_beam_stream_bytes
        (``state_bytes`` of it are the record), ``out`` the stream's result (``cap``: how many of its token columns the library may
        use, default all).  ``RnntBeamStream`` is the caller that keeps ``t_base`` and the flags right."""
        n = 0 if encp_rows is None else int(encp_rows.shape[0])
        cap = int(out.max_frames) if cap is None else min(int(cap), int(out.max_frames))
        rc = self.lib.gam_op_rnnt_beam_stream(self._h, _ptr(encp_rows if n else None), n, int(t_base), int(flags), int(beam_size),
                                              int(max_symbols), _ptr(state), min(int(state_bytes), state.numel() * 4), _ptr(out.ids),
                                              _ptr(out.frames), cap, _ptr(out.count), _ptr(out.score), _ptr(out.logp), _ptr(out.status),
                                              self._stream())
        self._check(rc, "gam_op_rnnt_beam_stream")

    def rnnt_beam_stream(self, beam_size: int, max_frames: int, max_symbols: int) -> RnntBeamStream:
        """A resumable RNN-T beam search over one stream of at most ``max_frames`` frames (gam_op_rnnt_beam_stream), with the hotwords
        of ``set_hotwords`` and the LM of ``set_lm``: feed it rows of ``rnnt_encp`` with ``push``, end it with ``finish``.  One
        workgroup; the beam with every hypothesis's predictor, hotword and LM state is carried from call to call, so the stream is
        searched as ONE utterance wherever it is cut.  After a later ``set_hotwords`` / ``set_lm`` the kernel refuses the stream's
        calls (status 0, ``host()`` raises)."""
        return RnntBeamStream(self, beam_size, max_frames, max_symbols)

    def rnnt_predict(self, labels: Optional[Tensor], state: Optional[Tuple[Tensor, Tensor]], batch_size: int = 1):
        """One predictor step (reference RNNTDecoder.predict, gigaam/decoder.py:85-102): labels i [B] or None (zero input),
        state (h, c) f32 [L,B,pred_hidden] or None -> (g f32 [B,pred_hidden], (h', c'))."""
        ph, nl = self.cfg.pred_hidden, self.cfg.pred_rnn_layers
        if labels is not None:
            labels = self._dev(labels.reshape(-1), torch.int32)
            b = labels.shape[0]
        else:
            b = batch_size if state is None else state[0].shape[1]
        h_in = c_in = None
        if state is not None:
            h_in, c_in = self._dev(state[0], torch.float32), self._dev(state[1], torch.float32)
            if tuple(h_in.shape) != (nl, b, ph) or tuple(c_in.shape) != (nl, b, ph):
                raise GigaAMHipError(f"predictor state must be two [{nl},{b},{ph}] tensors, got {tuple(h_in.shape)} / {tuple(c_in.shape)}")
        g = torch.empty((b, ph), dtype=torch.float32, device=self.device)
        h_out = torch.empty((nl, b, ph), dtype=torch.float32, device=self.device)
        c_out = torch.empty_like(h_out)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_rnnt_predict(self._h, _ptr(labels), _ptr(h_in), _ptr(c_in), b, _ptr(g), _ptr(h_out), _ptr(c_out), self._stream())
        self._check(rc, "gam_rnnt_predict")
        return g, (h_out, c_out)

    def rnnt_joint(self, enc: Tensor, dec: Tensor) -> Tensor:
        """Reference RNNTJoint.joint (gigaam/decoder.py:41-47): enc f32 [B,T,d_model], dec f32 [B,U,pred_hidden] ->
        log-probs f32 [B,T,U,num_classes]."""
        enc, dec = self._dev(enc, torch.float32), self._dev(dec, torch.float32)
        b, t, d = enc.shape
        b2, u, ph = dec.shape
        if b != b2 or d != self.cfg.d_model or ph != self.cfg.pred_hidden:
            raise GigaAMHipError(f"joint expects [B,T,{self.cfg.d_model}] and [B,U,{self.cfg.pred_hidden}], got {tuple(enc.shape)} / {tuple(dec.shape)}")
        out = torch.empty((b, t, u, self.cfg.num_classes), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_rnnt_joint(self._h, _ptr(enc), _ptr(dec), b, t, u, _ptr(out), self._stream())
        self._check(rc, "gam_rnnt_joint")
        return out

    def op_gemm(self, a: Tensor, w: Tensor, bias: Optional[Tensor] = None, act: int = 0, resid: Optional[Tensor] = None,
                alpha: float = 1.0) -> Tensor:
        """alpha * act(a @ w.T + bias) + resid (the encoder's residual epilogue when ``resid`` is given)."""
        a = self._dev(a, torch.float32)
        w = self._dev(w, torch.float32)
        bias = None if bias is None else self._dev(bias, torch.float32)
        resid = None if resid is None else self._dev(resid, torch.float32)
        m, k = a.shape
        n = w.shape[0]
        out = torch.empty((m, n), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_op_gemm_ex(self._h, _ptr(a), _ptr(w), _ptr(bias), _ptr(resid), alpha, _ptr(out), m, n, k, act,
                                         self._stream())
        self._check(rc, "gam_op_gemm_ex")
        return out

    def op_gemm_fmt(self, a: Tensor, w: Tensor, out: Tensor, bias: Optional[Tensor] = None, act: int = 0, resid: Optional[Tensor] = None,
                    alpha: float = 1.0, c_split: int = 0, c_guard: bool = False) -> Tensor:
        """gam_op_gemm_fmt: op_gemm into the caller's ``out`` (f32 [M, ldc], ldc >= N; ``resid`` has the same pitch and may BE ``out``) in
        the encoder's output formats -- c_split 0 fp32, 1 sp32 (hi / lo fp16 planes per 32 columns), 2 plain fp16 rows -- with the range
        guard on the stored values (``range_flag`` reads it).  Split-fp16 modes only."""
        a = self._dev(a, torch.float32)
        w = self._dev(w, torch.float32)
        bias = None if bias is None else self._dev(bias, torch.float32)
        m, k = a.shape
        n = w.shape[0]
        with torch.cuda.device(self.device):
            rc = self.lib.gam_op_gemm_fmt(self._h, _ptr(a), _ptr(w), _ptr(bias), _ptr(resid), alpha, _ptr(out), out.stride(0), m, n, k, act,
                                          int(c_split), int(bool(c_guard)), self._stream())
        self._check(rc, "gam_op_gemm_fmt")
        return out

    def op_attention(self, q: Tensor, k: Tensor, v: Tensor, lens: Optional[Tensor] = None) -> Tensor:
        """q, k, v [B,T,H*48] -> ctx [B,T,H*48]; keys >= lens[b] are masked."""
        q, k, v = (self._dev(t, torch.float32) for t in (q, k, v))
        b, t, d = q.shape
        lens_d = None if lens is None else self._dev(lens, torch.int32)
        out = torch.empty_like(q)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_op_attention(self._h, _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lens_d), b, t, d // 48, self._stream())
        self._check(rc, "gam_op_attention")
        return out

    def op_attention_ex(self, q: Tensor, k: Tensor, v: Tensor, B: int, Ta: int, Tv: int, H: int, lens: Optional[Tensor] = None,
                        cu: Optional[Tensor] = None, pbuf: Optional[Tensor] = None, pos_u: Optional[Tensor] = None,
                        pos_v: Optional[Tensor] = None) -> Tensor:
        """gam_op_attention_ex: q, k, v [rows, ldq] views sharing one row stride (columns of one [rows, 3*H*48] buffer allowed)
        -> ctx [rows, H*48]; cu = first packed row of every utterance, pbuf / pos_u / pos_v select relative-position attention."""
        ldq = q.stride(0)
        if not (q.is_cuda and k.is_cuda and v.is_cuda) or k.stride(0) != ldq or v.stride(0) != ldq or any(t.stride(1) != 1 for t in (q, k, v)):
            raise GigaAMHipError("op_attention_ex: q, k, v must be CUDA row views with one row stride")
        lens_d, cu_d = (None if t is None else self._dev(t, torch.int32) for t in (lens, cu))
        pbuf, pos_u, pos_v = (None if t is None else self._dev(t, torch.float32) for t in (pbuf, pos_u, pos_v))
        out = torch.full((q.shape[0], H * 48), float("nan"), dtype=torch.float32, device=self.device)   # (rows no utterance owns stay NaN)
        with torch.cuda.device(self.device):
            rc = self.lib.gam_op_attention_ex(self._h, _ptr(q), _ptr(k), _ptr(v), ldq, _ptr(out), _ptr(lens_d), _ptr(cu_d), B, Ta, Tv, H,
                                              _ptr(pbuf), _ptr(pos_u), _ptr(pos_v), self._stream())
        self._check(rc, "gam_op_attention_ex")
        return out

    def _op_ptr(self, what: str, name: str, t: Optional[Tensor], dtype: torch.dtype = torch.float32) -> Optional[int]:
        """Device address of a caller-owned operand of a raw op (written or read in place: no copy may be made), None = NULL."""
        if t is None:
            return None
        if not (t.is_cuda and t.device == self.device and t.dtype == dtype and t.is_contiguous()):
            raise GigaAMHipError(f"{what}: {name} must be a contiguous {dtype} tensor on {self.device}")
        return t.data_ptr()

    def op_layernorm(self, mode: int, rows: int, d: int, x: Optional[Tensor], out1: Tensor, w1: Tensor, b1: Tensor, *,
                     out2: Optional[Tensor] = None, w2: Optional[Tensor] = None, b2: Optional[Tensor] = None, split1: int = 0,
                     split2: int = 0, rs: Optional[Tensor] = None, rcos: Optional[Tensor] = None, rsin: Optional[Tensor] = None,
                     dk: int = 0, ta: int = 0, rope_rows: Optional[int] = None, row_t: Optional[Tensor] = None,
                     part: Optional[Tensor] = None, nsplit: int = 0, pbias: Optional[Tensor] = None, presid: Optional[Tensor] = None,
                     palpha: float = 1.0, xstore: Optional[Tensor] = None, eps: float = 1e-5) -> None:
        """gam_op_layernorm (include/gigaam_hip.h): one launch of the LayerNorm family on the caller's device tensors, which are
        written in place (out1 may be x; buffers may be longer than ``rows`` rows).  ``rope_rows`` defaults to the rows of rcos."""
        what = "op_layernorm"
        op = _lib.GamLnOp()
        for name, t in (("x", x), ("out1", out1), ("out2", out2), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2), ("rcos", rcos),
                        ("rsin", rsin), ("rs", rs), ("part", part), ("pbias", pbias), ("presid", presid), ("xstore", xstore)):
            setattr(op, name, self._op_ptr(what, name, t))
        op.row_t = self._op_ptr(what, "row_t", row_t, torch.int32)
        op.mode, op.rows, op.d, op.split1, op.split2, op.dk, op.ta, op.nsplit = mode, rows, d, split1, split2, dk, ta, nsplit
        op.rope_rows = (0 if rcos is None else rcos.shape[0]) if rope_rows is None else rope_rows
        op.eps, op.palpha = eps, palpha
        with torch.cuda.device(self.device):
            rc = self.lib.gam_op_layernorm(self._h, C.byref(op), self._stream())
        self._check(rc, "gam_op_layernorm")

    def op_convmod(self, u: Tensor, z: Tensor, dw_w: Tensor, dw_b: Tensor, n_scale: Tensor, n_shift: Tensor, lens: Tensor, B: int,
                   Ta: int, Tv: int, d: int, ks: int, layer_norm: bool, z_split: int = 0, cu: Optional[Tensor] = None) -> None:
        """gam_op_convmod (include/gigaam_hip.h): the fused conv-module middle on the caller's device tensors; z is written in place
        (it may be longer than the rows the launch owns).  A value beyond fp16's safe range raises the handle's range flag."""
        what = "op_convmod"
        ptrs = [self._op_ptr(what, n, t) for n, t in (("u", u), ("z", z), ("dw_w", dw_w), ("dw_b", dw_b), ("n_scale", n_scale),
                                                      ("n_shift", n_shift))]
        ptrs += [self._op_ptr(what, "lens", lens, torch.int32), self._op_ptr(what, "cu", cu, torch.int32)]
        with torch.cuda.device(self.device):
            rc = self.lib.gam_op_convmod(self._h, *ptrs, B, Ta, Tv, d, ks, int(bool(layer_norm)), z_split, self._stream())
        self._check(rc, "gam_op_convmod")

    # ------------------------------------------------------------------ profiling
    def profile_enable(self, on=True) -> None:
        """True/1: time every launch; 2: GEMM family only; False/0: off."""
        self._check(self.lib.gam_profile_enable(self._h, int(on)), "gam_profile_enable")

    def profile_level(self, on) -> None:
        """Change the collection level without resetting (sampled profiling: gam_profile_pause)."""
        self._check(self.lib.gam_profile_pause(self._h, int(on)), "gam_profile_pause")

    def profile_read(self) -> Dict[str, Dict[str, float]]:
        out = {}
        for i, name in enumerate(_lib.PF_CLASSES):
            ms, n, work = C.c_double(), C.c_int64(), C.c_double()
            self._check(self.lib.gam_profile_read(self._h, i, C.byref(ms), C.byref(n), C.byref(work)), "gam_profile_read")
            nbytes = C.c_double()
            self._check(self.lib.gam_profile_read_bytes(self._h, i, C.byref(nbytes)), "gam_profile_read_bytes")
            out[name] = {"ms": ms.value, "launches": int(n.value), "work": work.value, "bytes": nbytes.value}
        return out
