"""Word-level n-gram language model for CTC beam search (gam_set_lm, gigaam_amd/csrc/gam_search.h).

``NgramLM.from_arpa`` reads a plain or gzipped ARPA file with no external dependency; ``save`` / ``load`` keep the parsed model in a
``.npz`` (parsing a large ARPA in Python is slow).  ``score_words`` is the float64 sentence score the beam kernel's LM term follows.
``device_tables`` builds what the kernel reads: the token classes of a tokenizer, a word table (spelling hash -> LM word id) and an
n-gram table (key of a word-id tuple -> ln p, ln backoff), both open addressing with linear probing at load <= 0.5.

Hashes (shared with gam_search.h and tests/ctc_lm_ref.py; all arithmetic mod 2^64, P = 0x100000001b3):
  spelling   h = 0, then h = h * P + (token + 1) per token of the word
  n-gram     h = n, then h = h * P + (word id + 1) per word, oldest first
  table key  mix64(h) (the splitmix64 finaliser), 1 where that is 0; slot i of a probe: (key + i) & (slots - 1); key 0 marks a free
             slot.  Full keys are stored and compared: a collision of two 64-bit keys is accepted (2^-64 per compare)."""
from __future__ import annotations

import gzip
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

HASH_P = 0x100000001B3
MASK64 = (1 << 64) - 1
LN10 = math.log(10.0)
MAX_ORDER = 5                  # include/gigaam_hip.h gam_set_lm
MAX_SLOTS = 1 << 30            # slots per table: an int32 slot count
WORD_START = "▁"          # SentencePiece's word-start mark


def mix64(x: np.ndarray) -> np.ndarray:
    """splitmix64 finaliser of uint64 values, 0 mapped to 1 (0 marks a free slot)."""
    x = np.asarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    x[x == 0] = 1
    return x


def spelling_hash(ids: Sequence[int]) -> int:
    """The spelling hash of a word's token ids (the kernel keeps it incrementally per beam entry)."""
    h = 0
    for c in ids:
        h = (h * HASH_P + int(c) + 1) & MASK64
    return h


def ngram_hashes(ids: np.ndarray) -> np.ndarray:
    """The n-gram hashes of word-id tuples [N, n] (oldest word first), uint64 [N]."""
    ids = np.asarray(ids, dtype=np.int64)
    h = np.full(ids.shape[0], ids.shape[1], dtype=np.uint64)
    with np.errstate(over="ignore"):
        for k in range(ids.shape[1]):
            h = h * np.uint64(HASH_P) + (ids[:, k] + 1).astype(np.uint64)
    return h


def _open_table(keys: np.ndarray) -> Tuple[np.ndarray, np.ndarray, int]:
    """Linear-probing placement of unique non-zero uint64 keys at load <= 0.5 -> (slot keys [S], slot of each key [N], longest probe
    chain).  S is a power of two >= 16."""
    n = int(keys.shape[0])
    slots = 16
    while slots < 2 * n:
        slots *= 2
    if slots > MAX_SLOTS:
        raise ValueError(f"{n} table entries need {slots} slots, beyond the limit of {MAX_SLOTS}")
    mask = np.uint64(slots - 1)
    table = np.zeros(slots, dtype=np.uint64)
    slot_of = np.empty(n, dtype=np.int64)
    pend = np.arange(n, dtype=np.int64)
    probe = 0
    longest = 1 if n else 0
    with np.errstate(over="ignore"):
        while pend.size:
            s = ((keys[pend] + np.uint64(probe)) & mask).astype(np.int64)
            free = table[s] == 0
            cand, cs = pend[free], s[free]
            uniq, first = np.unique(cs, return_index=True)
            win = cand[first]
            table[uniq] = keys[win]
            slot_of[win] = uniq
            placed = np.zeros(pend.size, dtype=bool)
            placed[np.flatnonzero(free)[first]] = True
            if win.size:
                longest = max(longest, probe + 1)
            pend = pend[~placed]
            probe += 1
    return table, slot_of, longest


def _slot_words(keys: np.ndarray, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """16-byte slots {u64 key, 32-bit a, 32-bit b} as uint32 [S, 4]."""
    out = np.zeros((keys.shape[0], 4), dtype=np.uint32)
    out[:, 0] = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    out[:, 1] = (keys >> np.uint64(32)).astype(np.uint32)
    out[:, 2] = a.view(np.uint32)
    out[:, 3] = b.view(np.uint32)
    return out


def token_classes(tokenizer) -> np.ndarray:
    """Word class per token id of a tokenizer (``decoding.Tokenizer``), int32 [len + 1] (the blank last, class 0): 2 for the " "
    separator of a char-wise vocabulary, 1 for a piece that starts a word (begins with U+2581), 0 for one that continues it."""
    n = len(tokenizer)
    out = np.zeros(n + 1, dtype=np.int32)
    for i in range(n):
        s = tokenizer.id_to_str(i)
        out[i] = 2 if s == " " else (1 if s.startswith(WORD_START) else 0)
    return out


def word_spelling(tokenizer, word: str, classes: Optional[np.ndarray] = None) -> Optional[List[int]]:
    """The token ids a tokenizer spells a word with, or None when it cannot (out of vocabulary).  SentencePiece: ``encode``.  A
    char-wise vocabulary: one id per character.  A list vocabulary of pieces: the greedy longest match of U+2581 + word.  A spelling
    whose first token is a separator or whose later tokens start a word is rejected too (the beam could never hold it as one word)."""
    if not word:
        return None
    if not tokenizer.charwise:
        ids = list(tokenizer.encode(word))
        if not ids or tokenizer.model.unk_id() in ids:
            return None
    else:
        index = getattr(tokenizer, "_piece_index", None)
        if index is None:
            index = tokenizer._piece_index = {}
            for i, s in enumerate(tokenizer.vocab):
                index.setdefault(s, i)
            tokenizer._piece_max = max((len(s) for s in tokenizer.vocab), default=1)
        if tokenizer._piece_max <= 1:
            ids = [index.get(ch, -1) for ch in word]
        else:
            text, ids, i = WORD_START + word, [], 0
            while i < len(text):
                for L in range(min(tokenizer._piece_max, len(text) - i), 0, -1):
                    k = index.get(text[i:i + L])
                    if k is not None:
                        ids.append(k)
                        i += L
                        break
                else:
                    return None
        if not ids or min(ids) < 0:
            return None
    if classes is not None and (classes[ids[0]] == 2 or any(classes[c] != 0 for c in ids[1:])):
        return None
    return ids


class NgramLM:
    """An ARPA back-off n-gram model: ``vocab`` (word id -> word; ids in unigram order), ``order``, and per order k the n-grams as
    word-id tuples [n_k, k] (oldest first) with their natural-log probability and back-off weight.  ``unk`` is the id of "<unk>",
    one past the vocabulary when the ARPA has none (it then belongs to no n-gram and an out-of-vocabulary word scores
    ``unk_logp``)."""

    def __init__(self, vocab: Sequence[str], ngrams: Sequence[Tuple[np.ndarray, np.ndarray, np.ndarray]], unk_logp: float = -10.0):
        self.vocab = list(vocab)
        self.order = len(ngrams)
        if not 1 <= self.order <= MAX_ORDER:
            raise ValueError(f"n-gram order {self.order} outside [1, {MAX_ORDER}]")
        self.ngrams = []
        for k, (ids, lnp, lnbo) in enumerate(ngrams, start=1):
            ids = np.asarray(ids, dtype=np.int32).reshape(-1, k)
            self.ngrams.append((ids, np.asarray(lnp, dtype=np.float64), np.asarray(lnbo, dtype=np.float64)))
        self.unk_logp = float(unk_logp)
        self.index = {w: i for i, w in enumerate(self.vocab)}
        for w in ("<s>", "</s>"):
            if w not in self.index:
                raise ValueError(f"the n-gram model has no {w}")
        self.bos, self.eos = self.index["<s>"], self.index["</s>"]
        self.has_unk = "<unk>" in self.index
        self.unk = self.index["<unk>"] if self.has_unk else len(self.vocab)
        self._dict: Optional[Dict[tuple, Tuple[float, float]]] = None
        self._tables: Dict[tuple, Dict[str, object]] = {}

    @property
    def counts(self) -> List[int]:
        return [int(ids.shape[0]) for ids, _, _ in self.ngrams]

    # ---- reading and writing
    @classmethod
    def from_arpa(cls, path: str, unk_logp: float = -10.0) -> "NgramLM":
        """Parse an ARPA file (plain, or gzip when the name ends in .gz)."""
        opener = gzip.open if str(path).endswith(".gz") else open
        with opener(path, "rt", encoding="utf-8") as f:
            lines = f.read().splitlines()
        i, counts = 0, {}
        while i < len(lines) and lines[i].strip() != "\\data\\":
            i += 1
        if i == len(lines):
            raise ValueError(f"{path}: no \\data\\ section")
        i += 1
        while i < len(lines) and lines[i].strip().startswith("ngram "):
            n, c = lines[i].strip()[6:].split("=")
            counts[int(n)] = int(c)
            i += 1
        if not counts:
            raise ValueError(f"{path}: no n-gram counts")
        order = max(counts)
        if sorted(counts) != list(range(1, order + 1)):
            raise ValueError(f"{path}: n-gram orders {sorted(counts)} are not 1..{order}")
        if order > MAX_ORDER:
            raise ValueError(f"n-gram order {order} outside [1, {MAX_ORDER}]")
        index: Dict[str, int] = {}
        vocab: List[str] = []
        ngrams = []
        for n in range(1, order + 1):
            while i < len(lines) and lines[i].strip() != f"\\{n}-grams:":
                i += 1
            if i == len(lines):
                raise ValueError(f"{path}: no \\{n}-grams: section")
            i += 1
            ids, lp, bo = [], [], []
            while i < len(lines):
                s = lines[i].strip()
                if not s:
                    i += 1
                    continue
                if s.startswith("\\"):
                    break
                p = s.split()
                if len(p) not in (n + 1, n + 2):
                    raise ValueError(f"{path}:{i + 1}: expected {n} words and 1-2 values")
                words = p[1:n + 1]
                if n == 1:
                    if words[0] in index:
                        raise ValueError(f"{path}:{i + 1}: unigram {words[0]!r} listed twice")
                    index[words[0]] = len(vocab)
                    vocab.append(words[0])
                try:
                    ids.append([index[w] for w in words])
                except KeyError as e:
                    raise ValueError(f"{path}:{i + 1}: word {e.args[0]!r} is not a unigram") from None
                lp.append(float(p[0]))
                bo.append(float(p[n + 1]) if len(p) == n + 2 else 0.0)
                i += 1
            if len(ids) != counts[n]:
                raise ValueError(f"{path}: {len(ids)} {n}-grams, the header says {counts[n]}")
            ngrams.append((np.asarray(ids, dtype=np.int32).reshape(-1, n), np.asarray(lp) * LN10, np.asarray(bo) * LN10))
        return cls(vocab, ngrams, unk_logp)

    def save(self, path: str) -> None:
        arrays = {"vocab": np.asarray(self.vocab, dtype=object).astype(str), "unk_logp": np.float64(self.unk_logp)}
        for k, (ids, lnp, lnbo) in enumerate(self.ngrams, start=1):
            arrays[f"ids{k}"], arrays[f"lnp{k}"], arrays[f"lnbo{k}"] = ids, lnp, lnbo
        np.savez(path, **arrays)

    @classmethod
    def load(cls, path: str) -> "NgramLM":
        with np.load(path, allow_pickle=False) as z:
            order = sum(1 for k in z.files if k.startswith("ids"))
            return cls([str(w) for w in z["vocab"]], [(z[f"ids{k}"], z[f"lnp{k}"], z[f"lnbo{k}"]) for k in range(1, order + 1)],
                       float(z["unk_logp"]))

    @classmethod
    def open(cls, lm) -> "NgramLM":
        """An ``NgramLM``, or a path: ``.npz`` (``save``) or ARPA."""
        if isinstance(lm, NgramLM):
            return lm
        path = os.fspath(lm)
        return cls.load(path) if path.endswith(".npz") else cls.from_arpa(path)

    # ---- scoring (float64, natural log)
    def _table(self) -> Dict[tuple, Tuple[float, float]]:
        if self._dict is None:
            d = {}
            for ids, lnp, lnbo in self.ngrams:
                for t, p, b in zip(map(tuple, ids.tolist()), lnp.tolist(), lnbo.tolist()):
                    d.setdefault(t, (p, b))
            self._dict = d
        return self._dict

    def word_id(self, word: str) -> int:
        return self.index.get(word, self.unk)

    def lnprob(self, w: int, context: Sequence[int]) -> float:
        """ln P(w | context) by ARPA back-off (context: word ids, oldest first, the last order - 1 of them used).  A word with no
        unigram (only "<unk>" of a model without one) scores ``unk_logp``."""
        d = self._table()
        ctx = tuple(context)[-(self.order - 1):] if self.order > 1 else ()
        bo = 0.0
        for k in range(len(ctx), -1, -1):
            c = ctx[len(ctx) - k:]
            e = d.get(c + (w,))
            if e is not None:
                return e[0] + bo
            if k == 0:
                return self.unk_logp
            b = d.get(c)
            bo += b[1] if b is not None else 0.0
        return self.unk_logp

    def score_words(self, words: Sequence[str], bos: bool = True, eos: bool = True) -> float:
        """ln P of a word sequence: sum of ln P(w | the preceding order - 1 words), from "<s>" when ``bos``, with "</s>" at the end
        when ``eos``.  Words outside the vocabulary are "<unk>"."""
        ctx: List[int] = [self.bos] if bos else []
        total = 0.0
        ids = [self.word_id(w) for w in words] + ([self.eos] if eos else [])
        for w in ids:
            total += self.lnprob(w, ctx)
            ctx.append(w)
        return total

    # ---- device tables
    def device_tables(self, tokenizer) -> Dict[str, object]:
        """What gam_set_lm takes for this tokenizer, cached per vocabulary: ``classes`` int32 [V] (with the blank), ``words``
        uint32 [S_w, 4] and ``ngrams`` uint32 [S_n, 4] slot arrays, their longest probe chains ``word_probe`` / ``ngram_probe``,
        and ``oov``: how many LM words the tokenizer cannot spell (dropped from the word table)."""
        vkey = (tokenizer.charwise, tuple(tokenizer.vocab) if tokenizer.charwise else id(tokenizer.model))
        got = self._tables.get(vkey)
        if got is not None:
            return got
        classes = token_classes(tokenizer)
        keys, wids, oov = [], [], 0
        for i, w in enumerate(self.vocab):
            if w in ("<s>", "</s>", "<unk>"):
                continue
            sp = word_spelling(tokenizer, w, classes)
            if sp is None:
                oov += 1
                continue
            keys.append(spelling_hash(sp))
            wids.append(i)
        wk, first = np.unique(mix64(np.asarray(keys, dtype=np.uint64)), return_index=True)   # (two words spelt alike: the first)
        wid = np.asarray(wids, dtype=np.int32)[first]
        wt, wslot, wprobe = _open_table(wk)
        wa = np.zeros(wt.shape[0], dtype=np.int32)
        wa[wslot] = wid
        nkeys = np.concatenate([mix64(ngram_hashes(ids)) for ids, _, _ in self.ngrams])
        lnp = np.concatenate([p for _, p, _ in self.ngrams]).astype(np.float32)
        lnbo = np.concatenate([b for _, _, b in self.ngrams]).astype(np.float32)
        nkeys, first = np.unique(nkeys, return_index=True)   # (an n-gram listed twice: the first keeps it)
        nt, nslot, nprobe = _open_table(nkeys)
        na = np.zeros(nt.shape[0], dtype=np.float32)
        nb = np.zeros(nt.shape[0], dtype=np.float32)
        na[nslot], nb[nslot] = lnp[first], lnbo[first]
        got = {"classes": classes, "words": _slot_words(wt, wa, np.zeros_like(wa)), "word_probe": wprobe,
               "ngrams": _slot_words(nt, na, nb), "ngram_probe": nprobe, "oov": oov}
        self._tables[vkey] = got
        return got


def probe(table: np.ndarray, key: int, max_probe: int) -> Optional[np.ndarray]:
    """Host emulation of the kernel's probe: the slot [4] holding ``key`` (a table key, already mixed), or None."""
    mask = table.shape[0] - 1
    for i in range(max_probe):
        e = table[(key + i) & mask]
        k = int(e[0]) | (int(e[1]) << 32)
        if k == key:
            return e
        if k == 0:
            return None
    return None
