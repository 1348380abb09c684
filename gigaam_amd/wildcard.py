"""Wildcards in forced alignment: the host side of ``align(..., wildcard=)`` (the kernels' side is csrc/gam_trellis.h).

A wildcard is target id ``V = len(tokenizer) + 1``, one past blank: an ordinary CTC token -- at least one frame, blanks may flank
it -- whose emission is the frame's best log-prob minus a penalty.  Here: a text is cut at the wildcard string into pieces, the
pieces are tokenised and joined by id ``V``; a finished alignment is cut back at the wildcards into runs of ordinary tokens (whose
words are built run by run, so no word spans a gap) and the ``Gap`` each wildcard took.  Pure string / list work, no device.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple, Union

from .decoding import Tokenizer
from .types import Gap, Segment, Word

DEFAULT_PENALTY = math.log(2)     # (its identity tells a penalty that was passed from the default: GigaAMASR.align)


def spellable(tokenizer: Tokenizer, text: str) -> bool:
    """Whether the tokenizer turns ``text`` into ordinary tokens (then it cannot serve as the wildcard string)."""
    try:
        ids = tokenizer.encode(text)
    except ValueError:
        return False
    if tokenizer.charwise:
        return True
    unk = tokenizer.model.unk_id()
    return unk not in ids


def check(tokenizer: Tokenizer, wildcard: Optional[str], penalty: float) -> float:
    """Every error of the two keywords that needs no audio; returns the penalty as a float."""
    try:
        p = float(penalty)
    except (TypeError, ValueError):
        raise ValueError(f"wildcard_penalty must be a number, got {penalty!r}") from None
    if not math.isfinite(p) or p < 0:
        raise ValueError(f"wildcard_penalty must be finite and >= 0, got {penalty!r}")
    if wildcard is not None:
        if not isinstance(wildcard, str) or wildcard == "":
            raise ValueError("the wildcard string must be a non-empty str")
        if spellable(tokenizer, wildcard):
            raise ValueError(f"the wildcard string {wildcard!r} is text the tokenizer can spell: choose one outside the vocabulary")
    return p


def merge(ids: Sequence[int], wildcard_id: int) -> List[int]:
    """Adjacent wildcards merge into one."""
    out: List[int] = []
    for i in ids:
        if i == wildcard_id and out and out[-1] == wildcard_id:
            continue
        out.append(int(i))
    return out


def encode(tokenizer: Tokenizer, text: Union[str, Sequence[int]], wildcard: Optional[str], wildcard_id: int, enabled: bool) -> List[int]:
    """Token ids of one target.  A ``str`` is split at ``wildcard`` (when given), each piece tokenised as it is -- nothing normalised,
    spaces stay where they are -- and id ``wildcard_id`` put between the pieces; wildcards that touch, or that only empty pieces
    separate, merge into one.  A list of ids may hold ``wildcard_id`` when ``enabled`` (``ValueError`` otherwise: out of vocabulary)."""
    if isinstance(text, str):
        if wildcard is None:
            return tokenizer.encode(text)
        ids: List[int] = []
        for k, piece in enumerate(text.split(wildcard)):
            if k:
                ids.append(wildcard_id)
            ids.extend(tokenizer.encode(piece))
        return merge(ids, wildcard_id)
    ids = [int(i) for i in text]
    if wildcard_id in ids:
        if not enabled:
            raise ValueError(f"token id {wildcard_id} is outside the vocabulary (it is the wildcard id: pass wildcard= or wildcard_penalty=)")
        ids = merge(ids, wildcard_id)
    return ids


def runs(ids: Sequence[int], wildcard_id: int) -> Tuple[List[Tuple[int, int]], List[int]]:
    """(the [a, b) position ranges of the wildcard-free runs of ``ids``, empty ones left out; the positions of the wildcards)"""
    spans: List[Tuple[int, int]] = []
    stars: List[int] = []
    a = 0
    for i, t in enumerate(ids):
        if t == wildcard_id:
            if i > a:
                spans.append((a, i))
            stars.append(i)
            a = i + 1
    if len(ids) > a:
        spans.append((a, len(ids)))
    return spans, stars


def text_of(tokenizer: Tokenizer, ids: Sequence[int], wildcard_id: int, wildcard: Optional[str]) -> str:
    """The pieces' text joined by the wildcard string (``""`` when none was given)."""
    out, piece = [], []
    for t in ids:
        if t == wildcard_id:
            out.append(tokenizer.decode(piece))
            piece = []
        else:
            piece.append(t)
    out.append(tokenizer.decode(piece))
    return (wildcard or "").join(out)


def short_result(tokenizer: Tokenizer, ids: Sequence[int], first: Sequence[int], last: Sequence[int], frame_shift: float,
                 wildcard_id: int) -> Tuple[List[Word], List[Gap]]:
    """Words and gaps of one aligned utterance: ``frames_to_words`` per wildcard-free run, a ``Gap`` per wildcard from its run
    ``first[u] .. last[u]`` by the timing rule of words."""
    from .timestamps_utils import frames_to_words

    spans, stars = runs(ids, wildcard_id)
    words: List[Word] = []
    for a, b in spans:
        words.extend(frames_to_words(tokenizer, list(ids[a:b]), list(first[a:b]), frame_shift))
    gaps = [Gap(start=first[u] * frame_shift, end=(last[u] + 1) * frame_shift, start_frame=int(first[u]), end_frame=int(last[u]))
            for u in stars]
    return words, gaps


def longform_result(tokenizer: Tokenizer, ids: Sequence[int], token_segments: Sequence[int], token_frames: Sequence[int],
                    last_segments: Sequence[int], last_frames: Sequence[int], boundaries: Sequence[Tuple[float, float]],
                    seg_shifts: Sequence[float], wildcard_id: int) -> Tuple[List[Word], List[Segment], List[Gap]]:
    """The same over concatenated speech regions: ``longform_words`` per wildcard-free run (their per-region segments merged), a
    ``Gap`` per wildcard in file times -- it starts in region ``segment`` and ends in ``end_segment``."""
    from .timestamps_utils import longform_words

    spans, stars = runs(ids, wildcard_id)
    words: List[Word] = []
    per_seg: List[List[Word]] = [[] for _ in boundaries]
    for a, b in spans:
        ws, segs = longform_words(tokenizer, list(ids[a:b]), list(token_segments[a:b]), list(token_frames[a:b]), boundaries, seg_shifts)
        words.extend(ws)
        for k, sg in enumerate(segs):
            per_seg[k].extend(sg.words or [])
    segments = [Segment(text=" ".join(w.text for w in ws), start=s, end=e, words=ws) for (s, e), ws in zip(boundaries, per_seg)]
    gaps = []
    for u in stars:
        sa, sb = token_segments[u], last_segments[u]
        gaps.append(Gap(start=round(boundaries[sa][0] + token_frames[u] * seg_shifts[sa], 3),
                        end=round(boundaries[sb][0] + (last_frames[u] + 1) * seg_shifts[sb], 3),
                        start_frame=int(token_frames[u]), end_frame=int(last_frames[u]), segment=int(sa), end_segment=int(sb)))
    return words, segments, gaps
