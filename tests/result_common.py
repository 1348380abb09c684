"""Shared by tests/test_result_layouts_host.py (CPU) and tests/test_hip_result_collect.py (GPU): what ``host()`` of a packed decode
result of gigaam_amd/engine.py must return, told from the object's own device views.  Only constructors, attributes, ``host()`` and
``collect`` are used, so the checks hold an engine.py of any age to the same behaviour."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_result_layouts as M  # noqa: E402

# host() keys that are arrays (or, for AlignedLong, scalars) named like the attribute they come from
ARRAY_KEYS = {
    "Aligned": ("frame_labels", "tok_first", "tok_last", "status", "score", "loglik"),
    "RnntAligned": ("tok_frame", "status", "score", "loglik"),
    "AlignedLong": ("frame_labels", "tok_first", "tok_last"),
    "Confidence": ("conf", "span", "status"),
    "KeywordHits": ("n_hits", "hit_frames", "hit_score"),
    "BeamDecoded": ("score", "logp"),
    "NBestDecoded": ("score", "logp", "n_hyp"),
}
OTHER_KEYS = {"AlignedLong": ("score", "loglik", "status"), "BeamDecoded": ("rows",), "NBestDecoded": ("rows",)}
COPIES = ("BeamDecoded", "NBestDecoded")      # their arrays are copies; the other classes return views of the one host array
BEAM_COUNTS = [2, 0, 5]
NBEST_N_HYP, NBEST_COUNTS = [2, 1, 0], [[3, 5], [1, 0], [0, 0]]


def build(cls: str, d: dict, device="cpu"):
    """The result object on ``arange`` buffers, with plausible counts where ``host()`` reads them to cut rows."""
    bufs = M.buffers(cls, d, device)
    obj = M.construct(cls, d, bufs)
    if cls in ("BeamDecoded", "Decoded"):
        obj.counts.copy_(torch.tensor(BEAM_COUNTS[: d["b"]], dtype=torch.int32))
    if cls == "NBestDecoded":
        obj.n_hyp.copy_(torch.tensor(NBEST_N_HYP[: d["b"]], dtype=torch.int32))
        obj.counts.copy_(torch.tensor(NBEST_COUNTS[: d["b"]], dtype=torch.int32))
    return obj, bufs


def set_flag(obj, word: int) -> None:
    obj.ext[-1:].fill_(word)
    if obj.ext.is_cuda:       # host() / collect copy on the collect stream, which is ordered behind the result's EVENT only
        torch.cuda.synchronize()


def bits(a: np.ndarray) -> np.ndarray:
    return a.view(np.int32) if a.dtype == np.float32 else a


def rows_of(ids, frames, counts):
    ids, frames = ids.cpu().tolist(), frames.cpu().tolist()
    return [(ids[i][:c], frames[i][:c]) for i, c in enumerate(counts)]


def check_host(cls: str, obj, h: dict, flag: bool) -> None:
    """``h`` = ``obj.host()``: keys, dtypes, shapes, Python types and every value, against the object's own views."""
    assert set(h) == set(ARRAY_KEYS[cls]) | set(OTHER_KEYS.get(cls, ())) | {"flag"}, sorted(h)
    assert h["flag"] is flag
    for key in ARRAY_KEYS[cls]:
        view = getattr(obj, key)
        if view is None:
            assert h[key] is None
            continue
        want = view.cpu().numpy()
        assert isinstance(h[key], np.ndarray) and h[key].dtype == want.dtype and h[key].shape == want.shape, (key, h[key])
        assert np.array_equal(bits(h[key]), bits(want)), key
        assert h[key].flags.owndata == (cls in COPIES), key
    if cls == "AlignedLong":
        assert type(h["score"]) is float and type(h["loglik"]) is float and type(h["status"]) is int
        assert h["score"] == float(obj.score.cpu()[0]) and h["loglik"] == float(obj.loglik.cpu()[0])
        assert h["score"] != h["loglik"] and h["status"] == int(obj.status.cpu()[0])
    if cls == "BeamDecoded":
        assert h["rows"] == rows_of(obj.ids, obj.frames, obj.counts.cpu().tolist())
    if cls == "NBestDecoded":
        n_hyp, counts = obj.n_hyp.cpu().tolist(), obj.counts.cpu().tolist()
        assert h["rows"] == [rows_of(obj.ids[i], obj.frames[i], counts[i])[: n_hyp[i]] for i in range(obj.b)]
        m = max([c for r in counts for c in r] + [0])
        assert obj.copied_bytes == 4 * obj.small.numel() + (4 * 2 * obj.b * obj.n * min(m, obj.cap) if m > 0 else 0)


def check_flags(cls: str, obj) -> None:
    """Flag word 0 / 1 -> False / True; bit 1 raises (``HipEngine._flag_of``)."""
    from gigaam_amd.engine import GigaAMHipError
    for word, flag in ((0, False), (1, True)):
        set_flag(obj, word)
        check_host(cls, obj, obj.host(), flag)
    for word in (2, 3):
        set_flag(obj, word)
        with pytest.raises(GigaAMHipError, match="host length is shorter"):
            obj.host()
