"""The word n-gram LM of the float64 beam search references (the word rules of gigaam_amd/csrc/gam_search.h): ``LMSpec`` is what
``ctc_beam_ref.beam_search`` and ``rnnt_beam_ref.beam_search`` take as ``lm``.  numpy only; used by the CPU and the GPU tests.
Partial words are real tuples here, the ARPA model a dict of word tuples; the kernels identify them by 64-bit hashes (gigaam_amd/lm.py).

The searches are unchanged by it (same candidates, merges, ties and frame rule) but for one more per-prefix term:
  Words.  Every token has a class: 0 continues the current word, 1 starts a new word (the token belongs to it), 2 separates words
  (belongs to none).  A prefix's partial word is its tokens since the last class-1/2 token; its LM state the last order - 1
  completed words, ("<s>",) at the start.  Extending y by a class-1/2 token completes y's partial word w when it is non-empty:
  lm += alpha * ln P(w | state) + beta, and w enters the state.  w is the word the spelling table maps the partial word to, else
  "<unk>".  ln P is ARPA back-off in natural log: the longest context c with (c, w) listed gives ln p(c, w) plus the back-off
  weights of the longer contexts; a word with no unigram (only "<unk>" of a model without one) scores unk_logp.
  rank = (p_b (+) p_nb) + hotword bonus + lm.
  Final pick: the last non-empty partial word is completed, then alpha * ln P("</s>" | state) is added; best (p_b (+) p_nb) +
  committed hotword bonus + lm, ties to the lower beam position.  score = logp + committed + lm; an empty utterance (T = 0) scores
  0, as without the LM."""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

HASH_P = 0x100000001B3
MASK64 = (1 << 64) - 1


def spelling_hash(ids: Sequence[int]) -> int:
    """h = 0, then h = h * P + (id + 1) mod 2^64 per token: the kernel's partial-word identity."""
    h = 0
    for c in ids:
        h = (h * HASH_P + int(c) + 1) & MASK64
    return h


class ArpaLM:
    """A dict-based ARPA back-off model: ``ngrams[(w1, .., wn)] = (ln p, ln back-off)`` (words as strings)."""

    def __init__(self, text: str, unk_logp: float = -10.0):
        self.ngrams: Dict[Tuple[str, ...], Tuple[float, float]] = {}
        self.unk_logp = unk_logp
        section = 0
        ln10 = np.log(10.0)
        for line in text.splitlines():
            s = line.strip()
            if not s or s.startswith("ngram ") or s in ("\\data\\", "\\end\\"):
                continue
            if s.startswith("\\") and s.endswith("-grams:"):
                section = int(s[1:s.index("-")])
                continue
            p = s.split()
            words = tuple(p[1:section + 1])
            bo = float(p[section + 1]) if len(p) == section + 2 else 0.0
            self.ngrams.setdefault(words, (float(p[0]) * ln10, bo * ln10))
        self.order = max(len(k) for k in self.ngrams)
        self.words = {k[0] for k in self.ngrams if len(k) == 1}

    def lnprob(self, w: str, ctx: Sequence[str]) -> float:
        ctx = tuple(ctx)[-(self.order - 1):] if self.order > 1 else ()
        bo = 0.0
        for k in range(len(ctx), -1, -1):
            c = ctx[len(ctx) - k:]
            e = self.ngrams.get(c + (w,))
            if e is not None:
                return e[0] + bo
            if k == 0:
                return self.unk_logp
            b = self.ngrams.get(c)
            bo += b[1] if b is not None else 0.0
        return self.unk_logp

    def sentence(self, words: Sequence[str]) -> float:
        """ln P(<s> words </s>), out-of-vocabulary words as <unk>."""
        ctx, total = ["<s>"], 0.0
        for w in list(words) + ["</s>"]:
            w = w if w in self.words or w == "</s>" else "<unk>"
            total += self.lnprob(w, ctx)
            ctx.append(w)
        return total


class LMSpec:
    """What the search needs: the model, the token classes [V] (blank included), the spelling table (token-id tuple -> word), alpha
    and beta."""

    def __init__(self, lm: ArpaLM, classes: Sequence[int], spell: Dict[tuple, str], alpha: float, beta: float):
        self.lm, self.classes, self.spell, self.alpha, self.beta = lm, [int(c) for c in classes], dict(spell), float(alpha), float(beta)
        self.m = lm.order - 1

    def start(self) -> Tuple[tuple, tuple, float]:
        return (), (("<s>",) if self.m > 0 else ()), 0.0

    def complete(self, st):
        """(partial, ctx, lm) with the partial word completed (if non-empty)."""
        partial, ctx, acc = st
        if not partial:
            return st
        w = self.spell.get(partial, "<unk>")
        acc += self.alpha * self.lm.lnprob(w, ctx) + self.beta
        ctx = (ctx + (w,))[-self.m:] if self.m > 0 else ()
        return (), ctx, acc

    def step(self, st, c: int):
        cls = self.classes[c]
        if cls == 0:
            return st[0] + (c,), st[1], st[2]
        _, ctx, acc = self.complete(st)
        return ((c,) if cls == 1 else ()), ctx, acc

    def final(self, st) -> float:
        _, ctx, acc = self.complete(st)
        return acc + self.alpha * self.lm.lnprob("</s>", ctx)


def words_of(ids: Sequence[int], classes: Sequence[int]) -> List[tuple]:
    """The words (token-id tuples) of a label sequence under the class rule."""
    out, cur = [], ()
    for c in ids:
        k = classes[c]
        if k == 0:
            cur = cur + (c,)
            continue
        if cur:
            out.append(cur)
        cur = (c,) if k == 1 else ()
    if cur:
        out.append(cur)
    return out


def lm_term(ids: Sequence[int], spec: LMSpec) -> float:
    """The LM term of a complete label sequence: every word, then </s> (what the final pick adds up)."""
    st = spec.start()
    for c in ids:
        st = spec.step(st, int(c))
    return spec.final(st)
