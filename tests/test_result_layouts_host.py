"""The packed decode results of gigaam_amd/engine.py, without a GPU: every class's one layout statement gives the views, the
word count and the host arrays that tests/golden/result_layouts.json recorded before the layouts were stated once (three
hand-written copies each: allocation, constructor, ``host()``).  Fixture: tests/golden/make_result_layouts.py."""
import json
import os

import numpy as np
import pytest
import torch

import result_common as R
from result_common import M

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "result_layouts.json"), encoding="utf-8") as _f:
    FIXTURE = json.load(_f)


def test_fixture_covers_the_cases():
    assert [(fx["cls"], fx["dims"]) for fx in FIXTURE] == [(cls, d) for cls, d in M.CASES]


@pytest.mark.parametrize("fx", FIXTURE, ids=lambda fx: M.case_id((fx["cls"], fx["dims"])))
def test_views_and_words_are_the_recorded_ones(fx):
    from gigaam_amd import engine as E
    cls, d = fx["cls"], fx["dims"]
    bufs = M.buffers(cls, d)
    assert {k: v.numel() for k, v in bufs.items()} == fx["words"]
    assert M.attr_map(M.construct(cls, d, bufs), bufs) == fx["attrs"]
    # the allocator: the same words, and the same views of them
    klass, cpu = getattr(E, cls), torch.device("cpu")
    obj = klass.packed(cpu, d["b"], d["cap"]) if cls == "Decoded" else klass.empty(cpu, *d.values())
    own = {k: getattr(obj, k) for k in fx["words"]}
    assert {k: v.numel() for k, v in own.items()} == fx["words"] and all(v.dtype == torch.int32 for v in own.values())
    assert M.attr_map(obj, own) == fx["attrs"]
    for k, v in d.items():
        if cls not in ("Decoded", "BeamDecoded"):
            assert getattr(obj, k) == v       # (max_hits: the caller's value, not the clamped one)


@pytest.mark.parametrize("case", [c for c in M.CASES if c[0] != "Decoded"], ids=M.case_id)
def test_host_returns_the_views(case):
    cls, d = case
    obj, _ = R.build(cls, d)
    R.check_flags(cls, obj)


def test_an_f64_field_must_start_on_an_even_word():
    from gigaam_amd.engine import AlignedLong, GigaAMHipError

    class Odd(AlignedLong):
        FIELDS = (("status", (1,), torch.int32),) + AlignedLong.FIELDS

    with pytest.raises(GigaAMHipError, match="even word"):
        Odd.words(7, 3)


def test_decoded_has_the_layout_but_not_the_packed_allocator():
    from gigaam_amd.engine import BeamDecoded, Decoded
    assert not hasattr(Decoded, "empty") and hasattr(BeamDecoded, "empty")      # (Decoded's constructor takes views, not a buffer: ``packed``)
    assert Decoded.words(3, 5) == 2 * 3 * 5 + 3 + 1 and BeamDecoded.words(3, 5) == Decoded.words(3, 5) + 2 * 3


def test_confidence_without_span():
    from gigaam_amd.engine import Confidence
    obj, _ = R.build("Confidence", dict(b=3, cap=5, has_span=False))
    R.set_flag(obj, 0)
    assert obj.span is None and obj.host()["span"] is None and obj.status.data_ptr() - obj.whole.data_ptr() == 4 * 15
    assert Confidence.words(3, 5, True) - Confidence.words(3, 5, False) == 15


def test_nbest_with_no_tokens_copies_the_small_block_only():
    obj, _ = R.build("NBestDecoded", dict(b=3, n=2, cap=5))
    obj.counts.zero_()
    R.set_flag(obj, 0)
    h = obj.host()
    assert h["rows"] == [[([], []), ([], [])], [([], [])], []] and obj.copied_bytes == 4 * obj.small.numel()
    R.check_host("NBestDecoded", obj, h, False)


def test_nbest_rows_stop_at_n_hyp():
    obj, _ = R.build("NBestDecoded", dict(b=3, n=2, cap=5))
    R.set_flag(obj, 1)
    h = obj.host()
    assert R.NBEST_N_HYP == [2, 1, 0] and [len(r) for r in h["rows"]] == [2, 1, 0]
    assert h["rows"][0][1] == (obj.ids[0, 1].tolist(), obj.frames[0, 1].tolist()) and h["rows"][1][0] == ([obj.ids[1, 0, 0].item()], [obj.frames[1, 0, 0].item()])
    assert obj.copied_bytes == 4 * obj.small.numel() + 4 * obj.tok.numel()


def test_keyword_hits_dense_outputs_on_the_host():
    from gigaam_amd.engine import KeywordHits
    d = dict(b=3, k=2, max_hits=4)
    ds = torch.arange(42, dtype=torch.float32).view(3, 2, 7)
    obj = KeywordHits(M.buffers("KeywordHits", d)["whole"], 3, 2, 4, ds, ds.to(torch.int32))
    R.set_flag(obj, 0)
    h = obj.host()
    assert np.array_equal(h.pop("dense_score"), ds.numpy()) and h.pop("dense_start").dtype == np.int32
    R.check_host("KeywordHits", obj, h, False)


@pytest.mark.parametrize("b", [3, 1])
def test_collect_of_cpu_tensors(b):
    from gigaam_amd.engine import GigaAMHipError, HipEngine
    dec, _ = R.build("Decoded", dict(b=b, cap=5))
    want = R.rows_of(dec.ids, dec.frames, R.BEAM_COUNTS[:b])
    for word, flag in ((0, False), (1, True)):
        R.set_flag(dec, word)
        assert HipEngine.collect(dec) == (want, flag) and HipEngine.collect(*dec) == (want, False)
    R.set_flag(dec, 2)
    with pytest.raises(GigaAMHipError, match="host length is shorter"):
        HipEngine.collect(dec)
    R.set_flag(dec, 0)
    dec.counts[0] = -1
    with pytest.raises(GigaAMHipError, match="undecoded"):
        HipEngine.collect(dec)
