"""Seeded inputs of the keyword-search tests (CPU and GPU): log-probs of the three kinds test_hip_ctc_align uses, keywords, and
utterances with keywords PLANTED on the greedy path."""
import numpy as np
import torch


def log_probs(rng, B, T, V, kind, top=None):
    """Seeded log-probs [B, T, V] (float32): "peaked" (one dominant class per frame -- ``top`` [B, T] when given), "flat" (small
    logits: many near-equal paths) or "dyadic" (unnormalised values in {0, -0.5, -1, -2}: exact ties in fp32 and fp64 alike)."""
    if kind == "dyadic":
        return rng.choice(np.array([0.0, -0.5, -1.0, -2.0], dtype=np.float32), size=(B, T, V))
    x = rng.standard_normal((B, T, V)).astype(np.float32) * (0.3 if kind == "flat" else 1.0)
    if kind == "peaked":
        if top is None:
            top = rng.integers(0, V, (B, T))
        np.put_along_axis(x, np.asarray(top)[..., None], 9.0, axis=2)
    return torch.log_softmax(torch.from_numpy(x), dim=-1).numpy()


def keyword(rng, U, V, repeats=0):
    """U ids in [0, V - 2], ``repeats`` of them equal to their left neighbour."""
    y = rng.integers(0, V - 1, U)
    for i in (rng.choice(np.arange(1, U), size=min(repeats, U - 1), replace=False) if U > 1 else []):
        y[i] = y[i - 1]
    return [int(v) for v in y]


def background(rng, T, V):
    """A greedy path of T frames: blank on about 60 % of them, a random class elsewhere."""
    return np.where(rng.random(T) < 0.6, V - 1, rng.integers(0, V, T))


def plant(rng, top, V, y, pos, T):
    """Write one occurrence of y into the greedy path ``top`` from frame ``pos`` on: runs of 1-2 frames per token, a blank between
    two tokens when they are equal (needed) or at random, a blank before and behind.  Returns (start, end, next free frame), or
    None when it does not fit below T."""
    if pos < 1 or pos + 2 * len(y) + 1 >= T:
        return None
    s = pos
    top[s - 1] = V - 1
    for i, v in enumerate(y):
        top[pos] = v
        pos += 1
        if rng.random() < 0.5:
            top[pos] = v
            pos += 1
        if i + 1 < len(y) and (y[i + 1] == v or rng.random() < 0.5):
            top[pos] = V - 1
            pos += 1
    top[pos] = V - 1
    return s, pos - 1, pos + 2
