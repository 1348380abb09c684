"""``cfg.decoding`` slot: greedy decoders (reference gigaam/decoding.py:10-207).

``decode(head, encoded [B,D,T'], lengths [B]) -> [(text, ids, frames)]``.  The
token work (argmax/collapse, the RNN-T predictor/joint loop) runs in one HIP
launch per batch; only the final ragged ids/frames cross PCIe, once.
"""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from .decoder import CTCHead, RNNTHead


class Tokenizer:
    """Char-wise vocabulary or a SentencePiece model (reference decoding.py:10-44)."""

    def __init__(self, vocab: List[str], model_path: Optional[str] = None):
        self.charwise = model_path is None
        if self.charwise:
            self.vocab = vocab
        else:
            from sentencepiece import SentencePieceProcessor

            self.model = SentencePieceProcessor()
            self.model.load(model_path)

    def encode(self, text: str) -> List[int]:
        """Text -> token ids (the inverse of ``decode``): one id per character of a char-wise vocabulary -- a ``ValueError`` names
        every character it does not hold, nothing is normalised -- or the SentencePiece model's ``EncodeAsIds``."""
        if not self.charwise:
            return list(self.model.EncodeAsIds(text))
        index = getattr(self, "_index", None)
        if index is None:
            index = self._index = {}
            for i, c in enumerate(self.vocab):
                index.setdefault(c, i)
        unknown = sorted({c for c in text if c not in index})
        if unknown:
            raise ValueError(f"characters not in the vocabulary: {', '.join(repr(c) for c in unknown)}")
        return [index[c] for c in text]

    def decode(self, tokens: List[int]) -> str:
        if self.charwise:
            return "".join(self.vocab[t] for t in tokens)
        return self.model.decode(tokens)

    def __len__(self) -> int:
        return len(self.vocab) if self.charwise else len(self.model)

    def id_to_str(self, token_id: int) -> str:
        return self.vocab[token_id] if self.charwise else self.model.IdToPiece(token_id)


class RangeOverflow(RuntimeError):
    """Raised by ``finish`` when the batch it collects set the split-fp16 range flag (include/gigaam_hip.h,
    gam_range_flag): an activation left fp16's range somewhere before this decode, so its ids are not to be trusted.
    The model shim catches it and repeats the work under GAM_GEMM_F32 (model.py); a caller that drives the decoders
    directly sees it as an error, never as silently wrong ids."""


def check_range(flag) -> None:
    """Raise ``RangeOverflow`` if ``flag`` -- the range flag a collected result carries -- is set."""
    if flag:
        raise RangeOverflow("activation beyond the split-fp16 GEMM range (repeat under GAM_GEMM_F32)")


def _ragged(dec, *rest) -> List[Tuple[List[int], List[int]]]:
    """What decode_device returned (an ``engine.Decoded``; three bare tensors are accepted) -> host lists (one D2H for
    counts + range flag, one for ids / frames)."""
    from .engine import HipEngine
    rows, flag = HipEngine.collect(dec, *rest[:2])
    check_range(flag)
    return rows


def keyword_min_scores(token_counts, threshold) -> "np.ndarray":
    """Per keyword the lowest score that still counts: ``U_k * ln(threshold_k)`` in float32 -- ``threshold`` (one value, or one per
    keyword) is the geometric-mean likelihood ratio per token a hit must reach, in (0, 1]."""
    import numpy as np
    n = len(token_counts)
    thr = np.asarray(threshold, dtype=np.float64)
    if thr.ndim > 1 or (thr.ndim == 1 and thr.shape[0] != n):
        raise ValueError(f"threshold: one value or one per keyword ({n}) expected, got shape {thr.shape}")
    thr = np.broadcast_to(thr, (n,))
    if not np.all(np.isfinite(thr) & (thr > 0.0) & (thr <= 1.0)):
        raise ValueError(f"threshold must lie in (0, 1], got {threshold!r}")
    return (np.asarray(token_counts, dtype=np.float64) * np.log(thr)).astype(np.float32)


def keyword_hits(h, b: int, keywords, texts, frame_shift: float, offset: float = 0.0, segment=None):
    """Row ``b`` of a ``KeywordHits.host()`` dict -> (``KeywordHit`` list in keyword order, indices of the truncated keywords):
    ``start`` = start_frame x frame_shift, ``end`` = (end_frame + 1) x frame_shift (frames_to_words' convention); with ``segment``
    (a longform speech region) both are shifted by ``offset``, the region's start in the file."""
    import math
    from .types import KeywordHit
    hits, truncated = [], []
    mh = h["hit_frames"].shape[2]
    for k, ids in enumerate(keywords):
        n = int(h["n_hits"][b, k])
        if n > mh:
            truncated.append(k)
        for r in range(min(n, mh)):
            s, e = int(h["hit_frames"][b, k, r, 0]), int(h["hit_frames"][b, k, r, 1])
            sc = float(h["hit_score"][b, k, r])
            t0, t1 = s * frame_shift, (e + 1) * frame_shift
            if segment is not None:     # file times, rounded as transcribe_longform rounds its shifted word times
                t0, t1 = round(t0 + offset, 3), round(t1 + offset, 3)
            hits.append(KeywordHit(keyword=texts[k], keyword_index=k, start=t0, end=t1, score=sc, confidence=math.exp(sc / len(ids)),
                                   start_frame=s, end_frame=e, segment=segment))
    return hits, truncated


def keyword_stream_hits(h, keywords, texts, plan):
    """A ``KeywordStreamHits.host()`` dict of a search over the stitched stream of ``plan`` (windows.WindowPlan) -> (``KeywordHit`` list
    in keyword order, indices of the truncated keywords).  A hit's ``segment`` / ``end_segment`` are the windows its start and end
    frames were kept from, ``start_frame`` / ``end_frame`` the local frames inside those windows (the dropped ones counted, as
    ``plan.locate`` reports them); ``start`` = the start window's start + start_frame x its frame shift, ``end`` = the end window's
    start + (end_frame + 1) x its frame shift."""
    import math
    from .types import KeywordHit
    hits, truncated = [], []
    mh = h["hit_frames"].shape[1]
    for k, ids in enumerate(keywords):
        n = int(h["n_hits"][k])
        if n > mh:
            truncated.append(k)
        n = min(n, mh)
        fr = h["hit_frames"][k, :n]
        w0, j0, _ = plan.locate(fr[:, 0].tolist())
        w1, j1, _ = plan.locate(fr[:, 1].tolist())
        for r in range(n):
            sc = float(h["hit_score"][k, r])
            a, b = plan.windows[w0[r]], plan.windows[w1[r]]
            hits.append(KeywordHit(keyword=texts[k], keyword_index=k, start=a.start_s + j0[r] * a.shift,
                                   end=b.start_s + (j1[r] + 1) * b.shift, score=sc, confidence=math.exp(sc / len(ids)),
                                   start_frame=j0[r], end_frame=j1[r], segment=w0[r], end_segment=w1[r]))
    return hits, truncated


def sort_keyword_hits(hits):
    """By start time, then keyword index (then end time)."""
    return sorted(hits, key=lambda x: (x.start, x.keyword_index, x.end))


class _BeamInputs:
    """Hotwords and the LM as the beam searches take them (per-object caches); mixed into the decoding classes that search by beam."""

    def finish_nbest(self, dec) -> List[List[Tuple[str, List[int], List[int], float, float]]]:
        """An ``engine.NBestDecoded`` -> per utterance its hypotheses ``(text, ids, frames, score, logp)``, best first (at most two
        D2H copies: ``NBestDecoded.host``); raises ``RangeOverflow`` like ``finish``."""
        h = dec.host()
        check_range(h["flag"])
        return [[(self.tokenizer.decode(i), i, f, float(h["score"][b][r]), float(h["logp"][b][r])) for r, (i, f) in enumerate(rows)]
                for b, rows in enumerate(h["rows"])]

    def hotword_ids(self, hotwords) -> List[List[int]]:
        """Hotwords (each a string in the vocabulary -- ``Tokenizer.encode`` -- or token ids) -> token-id lists, the strings'
        encodings cached."""
        cache = self.__dict__.setdefault("_hotword_cache", {})
        out = []
        for w in hotwords or ():
            if isinstance(w, str):
                if w not in cache:
                    cache[w] = self.tokenizer.encode(w)
                out.append(cache[w])
            else:
                out.append([int(i) for i in w])
        return out

    def language_model(self, lm):
        """``lm`` (an ``lm.NgramLM``, a path to an ARPA or ``.npz`` file, or None) -> an ``NgramLM`` or None; a path is read once."""
        if lm is None:
            return None
        from .lm import NgramLM
        if isinstance(lm, NgramLM):
            return lm
        cache = self.__dict__.setdefault("_lm_cache", {})
        key = os.fspath(lm)
        if key not in cache:
            cache[key] = NgramLM.open(key)
        return cache[key]


class CTCGreedyDecoding(_BeamInputs):
    def __init__(self, vocabulary: List[str], model_path: Optional[str] = None):
        self.tokenizer = Tokenizer(vocabulary, model_path)
        self.blank_id = len(self.tokenizer)

    @torch.inference_mode()
    def decode_device(self, head: CTCHead, encoded: Tensor, lengths: Tensor, overlap: bool = False):
        """The device half of ``decode``: (ids, frames, counts) i32 tensors on the GPU, no host sync -- a driver
        can launch the next batch before it looks at this one (``finish``).  ``overlap`` is accepted for signature symmetry
        with the RNN-T decoder and ignored: the CTC decode is one 8 us kernel."""
        c = head.num_classes
        assert c == len(self.tokenizer) + 1, f"Num classes {c} != len(vocab)+1 {len(self.tokenizer)+1}"
        return head.engine.ctc_greedy(encoded, lengths)

    def finish(self, dec, *rest) -> List[Tuple[str, List[int], List[int]]]:
        """``dec``: the object ``decode_device`` returned (pass it whole: it carries the range flag word and the decode's
        completion event as explicit fields)."""
        return [(self.tokenizer.decode(i), i, f) for i, f in _ragged(dec, *rest)]

    @torch.inference_mode()
    def decode(self, head: CTCHead, encoded: Tensor, lengths: Tensor) -> List[Tuple[str, List[int], List[int]]]:
        return self.finish(self.decode_device(head, encoded, lengths))

    @torch.inference_mode()
    def decode_beam_device(self, head: CTCHead, encoded: Tensor, lengths: Tensor, beam_size: int = 8, hotwords=None,
                           hotword_boost: float = 2.0, lm=None, lm_weight: float = 0.5, word_bonus: float = 1.0):
        """The device half of ``decode_beam``: CTC prefix beam search (gam_ctc_beam), no host sync.  Returns an
        ``engine.BeamDecoded``: ``finish`` takes it as it takes a greedy decode; its ``host()`` also brings the scores.  The
        hotword set and the LM are uploaded only when they differ from the ones the engine holds."""
        c = head.num_classes
        assert c == len(self.tokenizer) + 1, f"Num classes {c} != len(vocab)+1 {len(self.tokenizer)+1}"
        head.engine.set_hotwords(self.hotword_ids(hotwords), hotword_boost)
        head.engine.set_lm(self.language_model(lm), self.tokenizer, lm_weight, word_bonus)
        return head.engine.ctc_beam(encoded, lengths, beam_size)

    @torch.inference_mode()
    def decode_beam(self, head: CTCHead, encoded: Tensor, lengths: Tensor, beam_size: int = 8, hotwords=None,
                    hotword_boost: float = 2.0, lm=None, lm_weight: float = 0.5,
                    word_bonus: float = 1.0) -> List[Tuple[str, List[int], List[int], float, float]]:
        """Beam search decode -> per utterance ``(text, ids, frames, score, logp)``: ``frames`` the frame at which each token entered
        the beam, ``score`` log p + committed hotword bonus + LM term, ``logp`` log p over the paths the beam kept.  ``lm`` (an
        ``NgramLM`` or a path) fuses a word n-gram LM: ``lm_weight`` * ln P(word | history) + ``word_bonus`` per word (gam_set_lm).
        ONE D2H copy; raises ``RangeOverflow`` like ``finish``."""
        h = self.decode_beam_device(head, encoded, lengths, beam_size, hotwords, hotword_boost, lm, lm_weight, word_bonus).host()
        check_range(h["flag"])
        return [(self.tokenizer.decode(i), i, f, float(h["score"][k]), float(h["logp"][k])) for k, (i, f) in enumerate(h["rows"])]

    @torch.inference_mode()
    def decode_nbest_device(self, head: CTCHead, encoded: Tensor, lengths: Tensor, n_best: int, beam_size: int = 8, hotwords=None,
                            hotword_boost: float = 2.0, lm=None, lm_weight: float = 0.5, word_bonus: float = 1.0):
        """The device half of ``decode_nbest`` (gam_ctc_beam_nbest), no host sync: an ``engine.NBestDecoded``."""
        c = head.num_classes
        assert c == len(self.tokenizer) + 1, f"Num classes {c} != len(vocab)+1 {len(self.tokenizer)+1}"
        head.engine.set_hotwords(self.hotword_ids(hotwords), hotword_boost)
        head.engine.set_lm(self.language_model(lm), self.tokenizer, lm_weight, word_bonus)
        return head.engine.ctc_beam_nbest(encoded, lengths, beam_size, n_best)

    @torch.inference_mode()
    def decode_nbest(self, head: CTCHead, encoded: Tensor, lengths: Tensor, n_best: int, beam_size: int = 8, hotwords=None,
                     hotword_boost: float = 2.0, lm=None, lm_weight: float = 0.5,
                     word_bonus: float = 1.0) -> List[List[Tuple[str, List[int], List[int], float, float]]]:
        """``decode_beam`` returning the ``n_best`` (<= ``beam_size``) best prefixes of the final beam: per utterance a list of
        ``(text, ids, frames, score, logp)``, best first by ``score`` (ties: the beam's order); entry 0 is ``decode_beam``'s result
        bit for bit.  A short utterance can have fewer than ``n_best``.  Raises ``RangeOverflow`` like ``finish``."""
        return self.finish_nbest(self.decode_nbest_device(head, encoded, lengths, n_best, beam_size, hotwords, hotword_boost, lm,
                                                          lm_weight, word_bonus))

    MAX_KEYWORD_TOKENS, MAX_KEYWORDS = 64, 4096     # include/gigaam_hip.h gam_set_keywords

    def keyword_ids(self, keywords) -> List[List[int]]:
        """Keywords (each a string in the vocabulary -- ``Tokenizer.encode``, nothing is normalised -- or token ids) -> token-id
        lists.  ``ValueError`` for characters outside the vocabulary, an empty keyword or list, more than 64 tokens in a keyword,
        more than 4096 keywords, an id outside the vocabulary."""
        if isinstance(keywords, str):
            raise ValueError("keywords: a list of keywords is expected, not one string")
        out = []
        for w in keywords:
            ids = self.tokenizer.encode(w) if isinstance(w, str) else [int(i) for i in w]
            if not ids:
                raise ValueError(f"keyword {len(out)} is empty")
            if len(ids) > self.MAX_KEYWORD_TOKENS:
                raise ValueError(f"keyword {len(out)} has {len(ids)} tokens, at most {self.MAX_KEYWORD_TOKENS} are searched")
            bad = [i for i in ids if not 0 <= i < self.blank_id]
            if bad:
                raise ValueError(f"keyword {len(out)}: token id {bad[0]} outside [0, {self.blank_id - 1}]")
            out.append(ids)
        if not out:
            raise ValueError("keywords: the list is empty")
        if len(out) > self.MAX_KEYWORDS:
            raise ValueError(f"{len(out)} keywords, at most {self.MAX_KEYWORDS} are searched at once")
        return out

    @torch.inference_mode()
    def find_keywords_device(self, head: CTCHead, encoded: Tensor, lengths: Tensor, keywords: List[List[int]], min_score,
                             max_hits: int = 8):
        """The device half of ``find_keywords`` (gam_ctc_kws), no host sync: an ``engine.KeywordHits``.  The keyword set is uploaded
        only when it differs from the one the engine holds."""
        c = head.num_classes
        assert c == len(self.tokenizer) + 1, f"Num classes {c} != len(vocab)+1 {len(self.tokenizer)+1}"
        if not 1 <= int(max_hits) <= 64:
            raise ValueError(f"max_hits={max_hits} outside [1, 64]")
        head.engine.set_keywords(keywords, min_score)
        return head.engine.ctc_kws(encoded, lengths, max_hits)

    def finish_keywords(self, dec) -> dict:
        """An ``engine.KeywordHits`` -> its host arrays (ONE D2H copy); raises ``RangeOverflow`` like ``finish``."""
        h = dec.host()
        check_range(h["flag"])
        return h

    MAX_ALIGN_TOKENS = 1024     # include/gigaam_hip.h gam_ctc_align

    @torch.inference_mode()
    def align(self, head: CTCHead, encoded: Tensor, lengths: Tensor, targets: List[List[int]], star_penalty: Optional[float] = None):
        """CTC forced alignment of known token ids (one list per utterance) on the device (gam_ctc_align), ONE D2H for the
        result.  Returns per utterance ``(ids, first_frames, last_frames, score, loglik, feasible)``: the first / last encoder frame
        of each token's run on the best path, that path's log-prob, log p(ids | audio) (= -ctc_loss) and whether any path exists
        (if not: empty frame lists, -inf scores).  Raises ``RangeOverflow`` like ``finish``.
        ``star_penalty`` (>= 0): gam_ctc_align_star -- id ``num_classes`` in a target is a wildcard (gigaam_amd/wildcard.py)."""
        c = head.num_classes
        assert c == len(self.tokenizer) + 1, f"Num classes {c} != len(vocab)+1 {len(self.tokenizer)+1}"
        targets = [[int(t) for t in ids] for ids in targets]
        too_long = [len(t) for t in targets if len(t) > self.MAX_ALIGN_TOKENS]
        if too_long:
            raise ValueError(f"forced alignment takes at most {self.MAX_ALIGN_TOKENS} tokens per utterance (got {max(too_long)})")
        if star_penalty is None:
            h = head.engine.ctc_align(encoded, lengths, targets).host()
        else:
            h = head.engine.ctc_align(encoded, lengths, targets, star_penalty=star_penalty).host()
        check_range(h["flag"])
        out = []
        for i, ids in enumerate(targets):
            ok = bool(h["status"][i])
            n = len(ids)
            first = h["tok_first"][i, :n].tolist() if ok else []
            last = h["tok_last"][i, :n].tolist() if ok else []
            out.append((ids, first, last, float(h["score"][i]), float(h["loglik"][i]), ok))
        return out


class RNNTGreedyDecoding:
    def __init__(self, vocabulary: List[str], model_path: Optional[str] = None, max_symbols_per_step: int = 10):
        self.tokenizer = Tokenizer(vocabulary, model_path)
        self.blank_id = len(self.tokenizer)
        self.max_symbols = max_symbols_per_step

    @torch.inference_mode()
    def decode_device(self, head: RNNTHead, encoded: Tensor, enc_len: Tensor, overlap: bool = False):
        """``overlap``: the caller is about to launch ANOTHER batch's frontend + encoder on the current stream -- run this
        latency-bound greedy loop beside it (decode side stream, small clusters: engine.HipEngine.rnnt_greedy) instead of in
        front of it.  Leave it False for a batch whose result is collected next (full-size clusters are faster alone)."""
        return head.engine.rnnt_greedy(encoded, enc_len, self.max_symbols, overlap=overlap)

    def finish(self, dec, *rest) -> List[Tuple[str, List[int], List[int]]]:
        """``dec``: the object ``decode_device`` returned (pass it whole: it carries the range flag word and the decode's
        completion event as explicit fields)."""
        return [(self.tokenizer.decode(i), i, f) for i, f in _ragged(dec, *rest)]

    @torch.inference_mode()
    def decode(self, head: RNNTHead, encoded: Tensor, enc_len: Tensor) -> List[Tuple[str, List[int], List[int]]]:
        return self.finish(self.decode_device(head, encoded, enc_len))

    MAX_ALIGN_TOKENS = 1024     # include/gigaam_hip.h gam_rnnt_align

    @torch.inference_mode()
    def align(self, head: RNNTHead, encoded: Tensor, enc_len: Tensor, targets: List[List[int]]):
        """Transducer forced alignment of known token ids (one list per utterance) on the device (gam_rnnt_align), ONE D2H for the
        result.  Returns per utterance ``(ids, frames, score, loglik, feasible)``: the frame at which each token is emitted on the
        best path (the meaning ``decode``'s frames have), that path's log-prob, log p(ids | audio) over all alignments (=
        -rnnt_loss) and whether any path exists (if not: an empty frame list, -inf scores).  The lattice is the loss's:
        ``max_symbols_per_step`` does not bound it, and neither hotwords nor the LM are read.  Raises ``RangeOverflow`` like
        ``finish``."""
        targets = [[int(t) for t in ids] for ids in targets]
        too_long = [len(t) for t in targets if len(t) > self.MAX_ALIGN_TOKENS]
        if too_long:
            raise ValueError(f"forced alignment takes at most {self.MAX_ALIGN_TOKENS} tokens per utterance (got {max(too_long)})")
        h = head.engine.rnnt_align(encoded, enc_len, targets).host()
        check_range(h["flag"])
        out = []
        for i, ids in enumerate(targets):
            ok = bool(h["status"][i])
            out.append((ids, h["tok_frame"][i, :len(ids)].tolist() if ok else [], float(h["score"][i]), float(h["loglik"][i]), ok))
        return out


class RNNTBeamDecoding(RNNTGreedyDecoding, _BeamInputs):
    """RNN-T beam search with hotword boosting and word n-gram LM fusion (gam_rnnt_beam; the contract is in
    gigaam_amd/csrc/gam_rnnt_beam.h).  A ``cfg.decoding`` target like the greedy one, so a config naming
    ``gigaam.decoding.RNNTBeamDecoding`` loads a model that decodes by beam, and ``GigaAMASR.set_decoding`` switches to it.
    ``beam_size`` 1..32; ``hotwords`` (strings in the vocabulary -- ``Tokenizer.encode`` -- or token ids) bias the search toward those
    phrases, ``hotword_boost`` per matched token.  ``lm`` (an ``lm.NgramLM`` or a path to an ARPA / ``.arpa.gz`` / ``.npz`` file)
    adds ``lm_weight`` * ln P(word | history) + ``word_bonus`` per completed word, and ln P(</s> | history) at the end.
    ``max_symbols_per_step`` 1..16."""

    def __init__(self, vocabulary: List[str], model_path: Optional[str] = None, max_symbols_per_step: int = 10, beam_size: int = 4,
                 hotwords=None, hotword_boost: float = 2.0, lm=None, lm_weight: float = 0.5, word_bonus: float = 1.0):
        super().__init__(vocabulary, model_path, max_symbols_per_step)
        if not 1 <= int(beam_size) <= 32:
            raise ValueError(f"beam_size {beam_size} outside [1, 32]")
        if not 1 <= int(max_symbols_per_step) <= 16:
            raise ValueError(f"max_symbols_per_step {max_symbols_per_step} outside [1, 16] for the RNN-T beam search")
        self.beam_size = int(beam_size)
        self.hotwords = list(hotwords) if hotwords else []
        self.hotword_boost = float(hotword_boost)
        self.set_lm(lm, lm_weight, word_bonus)

    def set_lm(self, lm=None, lm_weight: float = 0.5, word_bonus: float = 1.0) -> None:
        """The LM of every later search (None: none); a path is read here, once."""
        self.lm = self.language_model(lm)
        self.lm_weight, self.word_bonus = float(lm_weight), float(word_bonus)

    @torch.inference_mode()
    def decode_device(self, head: RNNTHead, encoded: Tensor, enc_len: Tensor, overlap: bool = False, beam_size: Optional[int] = None,
                      hotwords=None, hotword_boost: Optional[float] = None):
        """The device half of ``decode``: an ``engine.BeamDecoded``, no host sync; ``finish`` takes it as it takes a greedy decode.
        ``overlap`` is accepted for signature symmetry and ignored: the search runs on the current stream (the side-stream overlap of
        the greedy decode relies on its small clusters).  ``beam_size`` / ``hotwords`` / ``hotword_boost`` override this object's
        settings for one call; the hotword set and the LM (this object's, or none) are uploaded only when they differ from the ones
        the engine holds."""
        hw = self.hotwords if hotwords is None else hotwords
        boost = self.hotword_boost if hotword_boost is None else hotword_boost
        head.engine.set_hotwords(self.hotword_ids(hw), boost)
        head.engine.set_lm(self.lm, self.tokenizer, self.lm_weight, self.word_bonus)
        return head.engine.rnnt_beam(encoded, enc_len, self.beam_size if beam_size is None else beam_size, self.max_symbols)

    @torch.inference_mode()
    def decode_beam(self, head: RNNTHead, encoded: Tensor, enc_len: Tensor, beam_size: Optional[int] = None, hotwords=None,
                    hotword_boost: Optional[float] = None) -> List[Tuple[str, List[int], List[int], float, float]]:
        """Beam search decode -> per utterance ``(text, ids, frames, score, logp)``: ``frames`` the frame at which each token was
        emitted, ``score`` log p + committed hotword bonus + LM term (every word and </s>), ``logp`` log p summed over the
        alignments the beam merged.  Per-call
        ``beam_size`` / ``hotwords`` / ``hotword_boost`` default to this object's.  ONE D2H copy; raises ``RangeOverflow`` like
        ``finish``."""
        h = self.decode_device(head, encoded, enc_len, beam_size=beam_size, hotwords=hotwords, hotword_boost=hotword_boost).host()
        check_range(h["flag"])
        return [(self.tokenizer.decode(i), i, f, float(h["score"][k]), float(h["logp"][k])) for k, (i, f) in enumerate(h["rows"])]

    @torch.inference_mode()
    def decode_nbest_device(self, head: RNNTHead, encoded: Tensor, enc_len: Tensor, n_best: int, beam_size: Optional[int] = None,
                            hotwords=None, hotword_boost: Optional[float] = None):
        """The device half of ``decode_nbest`` (gam_rnnt_beam_nbest), no host sync: an ``engine.NBestDecoded``.  The per-call
        overrides are ``decode_device``'s."""
        hw = self.hotwords if hotwords is None else hotwords
        boost = self.hotword_boost if hotword_boost is None else hotword_boost
        head.engine.set_hotwords(self.hotword_ids(hw), boost)
        head.engine.set_lm(self.lm, self.tokenizer, self.lm_weight, self.word_bonus)
        return head.engine.rnnt_beam_nbest(encoded, enc_len, self.beam_size if beam_size is None else beam_size, self.max_symbols, n_best)

    @torch.inference_mode()
    def decode_nbest(self, head: RNNTHead, encoded: Tensor, enc_len: Tensor, n_best: int, beam_size: Optional[int] = None,
                     hotwords=None, hotword_boost: Optional[float] = None) -> List[List[Tuple[str, List[int], List[int], float, float]]]:
        """``decode_beam`` returning the ``n_best`` (<= the beam width) best hypotheses of the final beam: per utterance a list of
        ``(text, ids, frames, score, logp)``, best first by ``score`` (ties: the beam's order); entry 0 is ``decode_beam``'s result
        bit for bit.  Raises ``RangeOverflow`` like ``finish``."""
        return self.finish_nbest(self.decode_nbest_device(head, encoded, enc_len, n_best, beam_size, hotwords, hotword_boost))
