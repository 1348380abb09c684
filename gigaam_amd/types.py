"""Result containers returned by ``transcribe*`` -- same fields and ``str()``
behaviour as the reference's gigaam/types.py:18-68 (boundary types)."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Iterator, List, Optional, Sequence


@dataclass
class Word:
    text: str
    start: float
    end: float


@dataclass
class TranscriptionResult:
    text: str
    words: Optional[List[Word]] = None

    def __str__(self) -> str:
        return self.text


@dataclass
class Gap:
    """The stretch of audio a wildcard of a partial transcript took (``align(..., wildcard="*")``): ``start_frame`` / ``end_frame`` are
    the first and the last encoder frame of the wildcard's run on the best path, ``start`` / ``end`` their times by the rule of
    words (``start_frame`` x frame shift, (``end_frame`` + 1) x frame shift).  In a longform result the times are file times, the
    frames count inside speech regions ``segment`` (where the gap starts) and ``end_segment`` (where it ends: a gap may run across
    regions)."""
    start: float
    end: float
    start_frame: int
    end_frame: int
    segment: Optional[int] = None
    end_segment: Optional[int] = None


@dataclass
class AlignmentResult:
    """``GigaAMASR.align``: a known transcript placed on the audio by CTC forced alignment.  ``token_frames``: the first encoder
    frame of each token on the best path; ``score``: that path's log-prob; ``log_likelihood``: log p(text | audio) over all paths
    (= -CTC loss); ``feasible``: False when no path exists (the text is too long for the audio) -- then ``words`` and
    ``token_frames`` are empty and both scores are -inf.
    ``GigaAMASR.rnnt_align`` returns the same for RNN-T heads (transducer forced alignment): ``token_frames`` are then the frames at
    which the tokens are emitted on the best path, ``log_likelihood`` is -RNN-T loss, and every clip with a frame is feasible.
    With wildcards (``align(..., wildcard=)``): ``token_ids`` holds ``model.wildcard_id`` at a wildcard and ``token_frames`` its first
    frame, ``gaps`` one ``Gap`` per wildcard in order, ``text`` the pieces joined by the wildcard string; no word spans a gap; ``score``
    and ``log_likelihood`` are those of the lattice with the wildcards in it -- no longer the log-probability of a text."""
    text: str
    words: List[Word]
    token_ids: List[int]
    token_frames: List[int]
    score: float
    log_likelihood: float
    feasible: bool
    gaps: List[Gap] = field(default_factory=list)

    def __str__(self) -> str:
        return self.text


@dataclass
class ScoredWord:
    """A ``Word`` with its confidence: the aggregation of its tokens' confidences."""
    text: str
    start: float
    end: float
    confidence: float


@dataclass
class ConfidenceResult:
    """``GigaAMASR.confidence``: a transcript -- the model's own decode, or a known text placed by forced alignment -- with a
    confidence in [0, 1] per token, per word and for the utterance.  ``token_confidence``: the measure ("prob": p(token) under the
    distribution it was emitted from; "entropy": 1 - H / ln V) per token, for CTC heads aggregated over the frames of the token's
    run; ``words``: the words of ``transcribe(word_timestamps=True)``, each with the aggregation ("mean" / "min" / "prod") of its
    tokens; ``confidence``: the same aggregation over all tokens, None for an empty transcript.  ``feasible``: False when a given
    text cannot be aligned to the audio -- then ``words``, ``token_frames`` and ``token_confidence`` are empty."""
    text: str
    words: List[ScoredWord]
    token_ids: List[int]
    token_frames: List[int]
    token_confidence: List[float]
    confidence: Optional[float]
    feasible: bool

    def __str__(self) -> str:
        return self.text


@dataclass
class Hypothesis:
    """One entry of an ``NBestResult``.  ``token_frames``: the frames the search's ``frames`` are; ``score``: log p + committed hotword
    bonus + LM term, the value the list is ordered by; ``logp``: that log p alone (over the paths / alignments the beam kept);
    ``posterior``: the softmax of ``score`` over the hypotheses RETURNED -- the usual N-best posterior: it sums to 1 over the list
    whatever its length and is not a calibrated probability; ``words``: with ``word_timestamps=True``."""
    text: str
    token_ids: List[int]
    token_frames: List[int]
    score: float
    logp: float
    posterior: float
    words: Optional[List[Word]] = None

    def __str__(self) -> str:
        return self.text


def nbest_posteriors(scores: Sequence[float]) -> List[float]:
    """Softmax of the scores in float64 (empty -> empty)."""
    if not scores:
        return []
    m = max(scores)
    if m == -math.inf:
        return [1.0 / len(scores)] * len(scores)
    e = [math.exp(float(s) - m) for s in scores]
    z = math.fsum(e)
    return [x / z for x in e]


@dataclass
class NBestResult:
    """``GigaAMASR.transcribe_nbest``: the hypotheses of the final beam, best first (score descending).  ``best`` is what ``transcribe``
    returns under the same options."""
    hypotheses: List[Hypothesis]

    @property
    def best(self) -> Hypothesis:
        return self.hypotheses[0]

    @property
    def text(self) -> str:
        return self.hypotheses[0].text if self.hypotheses else ""

    def __str__(self) -> str:
        return self.text

    def __iter__(self) -> Iterator[Hypothesis]:
        return iter(self.hypotheses)

    def __len__(self) -> int:
        return len(self.hypotheses)


@dataclass
class Segment:
    text: str
    start: float
    end: float
    words: Optional[List[Word]] = None


@dataclass
class LongformTranscriptionResult:
    segments: List[Segment]

    @property
    def words(self) -> List[Word]:
        return [w for seg in self.segments if seg.words for w in seg.words]

    @property
    def has_word_timestamps(self) -> bool:
        return len(self.segments) > 0 and self.segments[0].words is not None

    @property
    def text(self) -> str:
        return " ".join(seg.text for seg in self.segments)

    def __str__(self) -> str:
        return self.text

    def __iter__(self) -> Iterator[Segment]:
        return iter(self.segments)

    def __len__(self) -> int:
        return len(self.segments)


@dataclass
class LongformAlignmentResult:
    """``GigaAMASR.align_longform``: a known transcript placed on a long recording by CTC forced alignment of the whole text against
    the concatenated speech regions.  ``words``: file times; ``token_segments`` / ``token_frames`` / ``token_times``: per token the
    speech region its first frame fell in, that frame counted inside the region, and its time in the file; ``score`` /
    ``log_likelihood``: the best path's log-prob and log p(text | audio) = -CTC loss over the concatenated frames; ``segments``: one
    ``Segment(text, start, end, words)`` per speech region, holding the words whose first token fell in it; ``feasible``: always
    True on a returned result (an infeasible text is a ``ValueError``)."""
    text: str
    words: List[Word]
    token_ids: List[int]
    token_segments: List[int]
    token_frames: List[int]
    token_times: List[float]
    score: float
    log_likelihood: float
    segments: List[Segment]
    feasible: bool
    gaps: List[Gap] = field(default_factory=list)     # one per wildcard (``align_longform(..., wildcard=)``), as ``AlignmentResult.gaps``

    def __str__(self) -> str:
        return self.text

    def __iter__(self) -> Iterator[Segment]:
        return iter(self.segments)

    def __len__(self) -> int:
        return len(self.segments)


@dataclass
class ScoredSegment:
    """A ``Segment`` whose words carry confidences; ``confidence``: the aggregation over the tokens of its words, None without any."""
    text: str
    start: float
    end: float
    words: List[ScoredWord]
    confidence: Optional[float]


@dataclass
class LongformConfidenceResult:
    """``GigaAMASR.confidence_longform``: the transcript of a recording of any length -- the model's own decode, or a known (partial)
    text placed by forced alignment -- with a confidence in [0, 1] per token, per word, per segment and for the file.  Words
    (text, start, end), segments, ``token_ids`` and ``gaps`` are those of ``transcribe_longform(word_timestamps=True)`` (without text)
    or ``align_longform`` (with text) under the same arguments; ``token_segments`` / ``token_frames`` / ``token_times`` as in
    ``LongformAlignmentResult``.  ``token_confidence``: per token as ``ConfidenceResult.token_confidence``, None at a wildcard, which
    belongs to no word and is left out of every aggregate; ``confidence``: the aggregation over all scored tokens, None without any.
    ``score`` / ``log_likelihood``: the alignment's, None without text."""
    text: str
    segments: List[ScoredSegment]
    words: List[ScoredWord]
    token_ids: List[int]
    token_segments: List[int]
    token_frames: List[int]
    token_times: List[float]
    token_confidence: List[Optional[float]]
    confidence: Optional[float]
    gaps: List[Gap] = field(default_factory=list)
    score: Optional[float] = None
    log_likelihood: Optional[float] = None

    def __str__(self) -> str:
        return self.text

    def __iter__(self) -> Iterator[ScoredSegment]:
        return iter(self.segments)

    def __len__(self) -> int:
        return len(self.segments)


@dataclass
class KeywordHit:
    """One occurrence of a keyword (``GigaAMASR.find_keywords``).  ``start`` / ``end``: seconds, ``start_frame`` x frame shift and
    (``end_frame`` + 1) x frame shift -- the convention of ``transcribe(word_timestamps=True)``; in a longform result they are file
    times and the frames count inside speech region ``segment``.  ``score``: the occurrence's log-likelihood ratio against the
    greedy path (<= 0; 0 where the greedy path spells the keyword); ``confidence`` = exp(score / tokens), the geometric mean of
    that ratio per token, in (0, 1] -- UNCALIBRATED: a ranking value, not a probability of being right.  On the windowed longform route
    (``find_keywords_longform(vad="windows")``) ``segment`` / ``end_segment`` are the windows the start and the end frame were kept
    from and ``start_frame`` / ``end_frame`` count inside those windows; elsewhere ``end_segment`` is None."""
    keyword: str
    keyword_index: int
    start: float
    end: float
    score: float
    confidence: float
    start_frame: int
    end_frame: int
    segment: Optional[int] = None
    end_segment: Optional[int] = None


@dataclass
class KeywordSearchResult:
    """``GigaAMASR.find_keywords``: ``hits`` sorted by start time, then keyword index; ``truncated``: the indices of the keywords that
    had more than ``max_hits`` occurrences (in one utterance / speech region) -- only the first ``max_hits`` of those are listed;
    ``keywords``: the keywords as text."""
    hits: List[KeywordHit]
    truncated: List[int]
    keywords: List[str]

    def __iter__(self) -> Iterator[KeywordHit]:
        return iter(self.hits)

    def __len__(self) -> int:
        return len(self.hits)
