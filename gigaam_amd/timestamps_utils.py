"""Encoder frames -> word timestamps (reference gigaam/timestamps_utils.py:8-53).
Pure host-side string work over the exact ``frames`` the HIP decoders emit."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

from .decoding import Tokenizer
from .preprocess import SAMPLE_RATE
from .types import ScoredSegment, ScoredWord, Segment, Word


def compute_frame_shift(audio_length_samples: int, seq_len: int) -> float:
    return audio_length_samples / SAMPLE_RATE / seq_len


def frames_to_words(tokenizer: Tokenizer, token_ids: List[int], token_frames: List[int], frame_shift: float) -> List[Word]:
    """A word ends at a space token (char vocab) or right before a piece that
    starts with the SentencePiece marker; start = first frame, end = last frame + 1."""
    words: List[Word] = []
    pieces: List[str] = []
    frames: List[int] = []

    def flush() -> None:
        text = "".join(pieces).strip()
        if text:
            words.append(Word(text=text, start=frames[0] * frame_shift, end=(frames[-1] + 1) * frame_shift))
        pieces.clear()
        frames.clear()

    for tok, frame in zip(token_ids, token_frames):
        piece = tokenizer.id_to_str(tok)
        if piece.startswith("▁"):
            flush()
            piece = piece[1:]
        elif piece == " ":
            flush()
            continue
        pieces.append(piece)
        frames.append(frame)
    flush()
    return words


def word_token_groups(tokenizer: Tokenizer, token_ids: List[int]) -> List[List[int]]:
    """The positions in ``token_ids`` of the tokens of every word ``frames_to_words`` returns, word by word: a piece that starts with
    the SentencePiece marker belongs to the word it starts, the space token of a char-wise vocabulary to none (the token classes of
    lm.py), and a group whose text is empty is no word."""
    groups: List[List[int]] = []
    pieces: List[str] = []
    members: List[int] = []

    def flush() -> None:
        if "".join(pieces).strip():
            groups.append(list(members))
        pieces.clear()
        members.clear()

    for i, tok in enumerate(token_ids):
        piece = tokenizer.id_to_str(tok)
        if piece.startswith("▁"):
            flush()
            piece = piece[1:]
        elif piece == " ":
            flush()
            continue
        pieces.append(piece)
        members.append(i)
    flush()
    return groups


def aggregate_confidence(values: List[float], aggregation: str):
    """"mean" | "min" | "prod" of token confidences; None for no tokens."""
    if aggregation not in ("mean", "min", "prod"):
        raise ValueError(f"unknown confidence aggregation {aggregation!r} (one of mean, min, prod)")
    if not values:
        return None
    if aggregation == "mean":
        return float(sum(values) / len(values))
    if aggregation == "min":
        return float(min(values))
    out = 1.0
    for v in values:
        out *= float(v)
    return out


def score_longform(tokenizer: Tokenizer, token_ids: Sequence[int], conf: Sequence[float], words: Sequence[Word],
                   segments: Sequence[Segment], aggregation: str, wildcard_id: Optional[int] = None):
    """Confidences added to a finished longform result.  ``words`` are the words a longform route built from ``token_ids`` (in order:
    ``frames_to_words`` / ``longform_words`` on each wildcard-free run), ``segments`` hold those same ``Word`` objects, ``conf`` one
    value per token (what stands at a wildcard is not read).  Returns (token confidences with None at the wildcards, ``ScoredWord``
    per word, ``ScoredSegment`` per segment, the file's confidence): a word aggregates its tokens (``word_token_groups``), a segment
    the tokens of its words, the file every token that is no wildcard; None where there is no token."""
    ids = [int(i) for i in token_ids]
    token_conf = [None if i == wildcard_id else float(c) for i, c in zip(ids, conf)]
    groups: List[List[int]] = []
    a = 0
    for b in [k for k, i in enumerate(ids) if i == wildcard_id] + [len(ids)]:      # word groups run by run: no word spans a wildcard
        groups += [[a + k for k in g] for g in word_token_groups(tokenizer, ids[a:b])]
        a = b + 1
    if len(groups) != len(words):
        raise ValueError(f"{len(words)} words for {len(groups)} word groups of the token list")
    scored = [ScoredWord(text=w.text, start=w.start, end=w.end, confidence=aggregate_confidence([token_conf[k] for k in g], aggregation))
              for w, g in zip(words, groups)]
    index = {id(w): k for k, w in enumerate(words)}
    out_segments = []
    for sg in segments:
        ks = [index[id(w)] for w in sg.words or []]
        out_segments.append(ScoredSegment(text=sg.text, start=sg.start, end=sg.end, words=[scored[k] for k in ks],
                                          confidence=aggregate_confidence([token_conf[t] for k in ks for t in groups[k]], aggregation)))
    return token_conf, scored, out_segments, aggregate_confidence([c for c in token_conf if c is not None], aggregation)


def concat_frames_to_segments(frames: Sequence[int], seg_frames: Sequence[int], seg_starts: Sequence[float],
                              seg_shifts: Sequence[float]) -> Tuple[List[int], List[int], List[float]]:
    """Frames of the concatenation of several segments' encoder frames (segment i contributes ``seg_frames[i]`` of them, starts at
    ``seg_starts[i]`` seconds in the file and has a frame shift of ``seg_shifts[i]`` seconds) -> per frame (segment, frame inside the
    segment, time in the file = start + local frame x shift).  Segments without frames are skipped over."""
    bounds, total = [], 0
    for n in seg_frames:
        total += int(n)
        bounds.append(total)
    segs, local, times = [], [], []
    from bisect import bisect_right
    for f in frames:
        f = int(f)
        if f < 0 or f >= total:
            raise ValueError(f"frame {f} outside the {total} concatenated frames")
        i = bisect_right(bounds, f)
        loc = f - (bounds[i - 1] if i else 0)
        segs.append(i)
        local.append(loc)
        times.append(seg_starts[i] + loc * seg_shifts[i])
    return segs, local, times


def longform_words(tokenizer: Tokenizer, token_ids: Sequence[int], token_segments: Sequence[int], token_frames: Sequence[int],
                   boundaries: Sequence[Tuple[float, float]], seg_shifts: Sequence[float]) -> Tuple[List[Word], List[Segment]]:
    """Words of a transcript aligned to concatenated segments, by the rule of ``frames_to_words`` applied to file times: a word
    starts at its first token's first frame and ends one frame after its last token's first frame, each taken in the segment the
    token fell in (so a word whose tokens straddle two regions starts in the first and ends in the second).  Returns the words and
    one ``Segment(text, start, end, words)`` per entry of ``boundaries`` holding the words whose first token fell in it."""
    words: List[Word] = []
    per_seg: List[List[Word]] = [[] for _ in boundaries]
    for group in word_token_groups(tokenizer, list(token_ids)):
        a, b = group[0], group[-1]
        sa, sb = token_segments[a], token_segments[b]
        text = "".join(tokenizer.id_to_str(token_ids[i]) for i in group).replace("▁", "").strip()
        w = Word(text=text, start=round(boundaries[sa][0] + token_frames[a] * seg_shifts[sa], 3),
                 end=round(boundaries[sb][0] + (token_frames[b] + 1) * seg_shifts[sb], 3))
        words.append(w)
        per_seg[sa].append(w)
    segments = [Segment(text=" ".join(w.text for w in ws), start=s, end=e, words=ws) for (s, e), ws in zip(boundaries, per_seg)]
    return words, segments
