"""Fixture for the packed decode results of gigaam_amd/engine.py: where every tensor attribute of a result object lies in its buffer.

For every case of ``CASES`` the result object is built through its public constructor on ``torch.arange`` i32 CPU buffers, and every
tensor attribute is recorded as (buffer it is a view of, byte offset in it, shape, dtype), next to the buffers' word counts as the
allocation expressions of the engine's methods give them (``parent_words``: copied from the commit this fixture was written on, where
every layout was still spelled by hand; tests/test_result_layouts_host.py holds the engine to them).  No GPU, no library.

    python tests/golden/make_result_layouts.py      ->  tests/golden/result_layouts.json

tests/test_result_layouts_host.py and tests/test_hip_result_collect.py import ``CASES`` / ``construct`` / ``attr_map`` from here.
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (class, constructor dimensions).  First the smallest dimensions that tell every field apart, then the degenerate ones.
CASES = [
    ("Aligned", dict(b=3, tp=5, umax=4)), ("Aligned", dict(b=1, tp=5, umax=4)), ("Aligned", dict(b=3, tp=5, umax=0)),
    ("RnntAligned", dict(b=3, umax=4)), ("RnntAligned", dict(b=1, umax=4)), ("RnntAligned", dict(b=3, umax=0)),
    ("AlignedLong", dict(t=7, u=3)), ("AlignedLong", dict(t=7, u=0)),
    ("Confidence", dict(b=3, cap=5, has_span=True)), ("Confidence", dict(b=3, cap=5, has_span=False)),
    ("Confidence", dict(b=1, cap=5, has_span=True)), ("Confidence", dict(b=1, cap=5, has_span=False)),
    ("KeywordHits", dict(b=3, k=2, max_hits=4)), ("KeywordHits", dict(b=1, k=2, max_hits=4)), ("KeywordHits", dict(b=3, k=0, max_hits=4)),
    ("KeywordHits", dict(b=3, k=2, max_hits=-1)),        # (the library rejects it; the buffers are those of max_hits = 0)
    ("BeamDecoded", dict(b=3, cap=5)), ("BeamDecoded", dict(b=1, cap=5)),
    ("NBestDecoded", dict(b=3, n=2, cap=5)), ("NBestDecoded", dict(b=1, n=2, cap=5)),
    ("Decoded", dict(b=3, cap=5)), ("Decoded", dict(b=1, cap=5)),
]


def case_id(case) -> str:
    return case[0] + "-" + "-".join(f"{k}{int(v)}" for k, v in case[1].items())


def parent_words(cls: str, d: dict) -> dict:
    """Words of every buffer of a result, as the engine's methods allocated them when each wrote its own expression."""
    if cls == "Aligned":            # _align_buffers
        return {"whole": d["b"] * d["tp"] + 2 * d["b"] * d["umax"] + 3 * d["b"] + 1}
    if cls == "RnntAligned":        # _rnnt_align_buffers
        return {"whole": d["b"] * d["umax"] + 3 * d["b"] + 1}
    if cls == "AlignedLong":        # op_ctc_align_long
        return {"whole": 6 + d["t"] + 2 * d["u"]}
    if cls == "Confidence":         # _confidence_out
        return {"whole": (2 if d["has_span"] else 1) * d["b"] * d["cap"] + d["b"] + 1}
    if cls == "KeywordHits":        # _kws_out
        return {"whole": d["b"] * d["k"] * (1 + 3 * max(d["max_hits"], 0)) + 1}
    if cls == "BeamDecoded":        # _beam_out
        return {"buf": 2 * d["b"] * d["cap"] + 3 * d["b"] + 1}
    if cls == "NBestDecoded":       # _nbest_out
        return {"tok": 2 * d["b"] * d["n"] * d["cap"], "small": d["b"] + 3 * d["b"] * d["n"] + 1}
    if cls == "Decoded":            # ctc_greedy, rnnt_greedy
        return {"whole": 2 * d["b"] * d["cap"] + d["b"] + 1}
    raise KeyError(cls)


def buffers(cls: str, d: dict, device="cpu") -> dict:
    """``arange`` i32 buffers of ``parent_words``' sizes (every word differs from its neighbours: a shifted view shows)."""
    out = {k: torch.arange(n, dtype=torch.int32, device=device) for k, n in parent_words(cls, d).items()}
    if cls == "NBestDecoded":
        out["tok"] = out["tok"].view(2, d["b"], d["n"], d["cap"])
    return out


def construct(cls: str, d: dict, bufs: dict):
    """The result object over ``bufs``, through its public constructor."""
    from gigaam_amd import engine as E
    if cls == "Aligned":
        return E.Aligned(bufs["whole"], d["b"], d["tp"], d["umax"])
    if cls == "RnntAligned":
        return E.RnntAligned(bufs["whole"], d["b"], d["umax"])
    if cls == "AlignedLong":
        return E.AlignedLong(bufs["whole"], d["t"], d["u"])
    if cls == "Confidence":
        return E.Confidence(bufs["whole"], d["b"], d["cap"], d["has_span"])
    if cls == "KeywordHits":
        return E.KeywordHits(bufs["whole"], d["b"], d["k"], d["max_hits"])
    if cls == "BeamDecoded":
        return E.BeamDecoded(bufs["buf"], d["b"], d["cap"])
    if cls == "NBestDecoded":
        return E.NBestDecoded(bufs["tok"], bufs["small"])
    if cls == "Decoded":            # the views ctc_greedy / rnnt_greedy take of their one buffer
        w, b, cap = bufs["whole"], d["b"], d["cap"]
        ids, frames, ext = w[: b * cap].view(b, cap), w[b * cap: 2 * b * cap].view(b, cap), w[2 * b * cap:]
        return E.Decoded(ids, frames, ext[:b], ext, whole=w)
    raise KeyError(cls)


def attr_map(obj, bufs: dict) -> dict:
    """{attribute: {buffer, byte offset, shape, dtype} | None} of every public tensor-or-None attribute (and of the tuple's members
    ids / frames / counts for a ``Decoded``)."""
    named = {k: v for k, v in vars(obj).items() if not k.startswith("_") and (v is None or isinstance(v, torch.Tensor))}
    if isinstance(obj, tuple):
        named.update(ids=obj[0], frames=obj[1], counts=obj[2])
    out = {}
    for name, t in sorted(named.items()):
        if t is None:
            out[name] = None
            continue
        home = [k for k, buf in bufs.items() if buf.untyped_storage().data_ptr() == t.untyped_storage().data_ptr()]
        assert len(home) == 1, (name, home)
        buf = bufs[home[0]]        # (storage offsets: an empty view has no data_ptr() to subtract)
        out[name] = {"buffer": home[0], "offset": t.storage_offset() * t.element_size() - buf.storage_offset() * buf.element_size(), "shape": list(t.shape),
                     "dtype": str(t.dtype).replace("torch.", "")}
    return out


def main():
    fx = []
    for cls, d in CASES:
        bufs = buffers(cls, d)
        fx.append({"cls": cls, "dims": d, "words": parent_words(cls, d), "attrs": attr_map(construct(cls, d, bufs), bufs)})
    with open(os.path.join(HERE, "result_layouts.json"), "w", encoding="utf-8") as f:
        json.dump(fx, f, indent=0)
    print(len(fx), "cases")


if __name__ == "__main__":
    main()
