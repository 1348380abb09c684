"""The device-to-host side of every packed decode result (gigaam_amd/engine.py): ``host()`` of each result class and the three
regimes of ``HipEngine.collect``, on the GPU, against the objects' own device views.  No model weights, no library call: the
buffers are filled with ``arange``, so a field read from the wrong words shows as wrong numbers."""
import pytest
import torch

import result_common as R
from result_common import M

# (max_hits < 0 never reaches a result object: the library rejects it.  tests/test_result_layouts_host.py holds its layout.)
CASES = [c for c in M.CASES if c[0] != "Decoded" and not (c[0] == "KeywordHits" and c[1]["max_hits"] < 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=M.case_id)
def test_host_returns_the_device_views(case):
    cls, d = case
    obj, _ = R.build(cls, d, "cuda:0")
    for with_event in (True, False):
        if with_event:
            obj.event, obj.stream = torch.cuda.Event(), torch.cuda.current_stream()
            obj.event.record(obj.stream)
        else:
            obj.event = None
        R.check_flags(cls, obj)


@pytest.mark.gpu
def test_keyword_hits_host_brings_the_dense_outputs():
    d = dict(b=3, k=2, max_hits=4)
    from gigaam_amd.engine import KeywordHits
    whole = M.buffers("KeywordHits", d, "cuda:0")["whole"]
    ds = torch.arange(3 * 2 * 7, dtype=torch.float32, device="cuda:0").view(3, 2, 7)
    obj = KeywordHits(whole, d["b"], d["k"], d["max_hits"], ds, (ds * 2).to(torch.int32))
    R.set_flag(obj, 0)
    h = obj.host()
    assert torch.equal(torch.from_numpy(h.pop("dense_score")), ds.cpu()) and torch.equal(torch.from_numpy(h.pop("dense_start")), obj.dense_start.cpu())
    R.check_host("KeywordHits", obj, h, False)


@pytest.mark.gpu
@pytest.mark.parametrize("b", [3, 1])
def test_collect_regimes_agree(b):
    """One copy of the whole buffer, the event path (counts first, then the used columns) and three bare tensors: same rows;
    the first two also the flag, and each its own error for an undecoded utterance."""
    from gigaam_amd.engine import GigaAMHipError, HipEngine
    dec, _ = R.build("Decoded", dict(b=b, cap=5), "cuda:0")
    dec.event, dec.stream = torch.cuda.Event(), torch.cuda.current_stream()
    dec.event.record(dec.stream)
    want = R.rows_of(dec.ids, dec.frames, R.BEAM_COUNTS[:b])
    assert dec.whole.numel() * 4 <= HipEngine.ONE_COPY_BYTES
    keep = HipEngine.ONE_COPY_BYTES
    try:
        for one_copy_bytes in (keep, 0):
            HipEngine.ONE_COPY_BYTES = one_copy_bytes
            for word, flag in ((0, False), (1, True)):
                R.set_flag(dec, word)
                assert HipEngine.collect(dec) == (want, flag)
            R.set_flag(dec, 2)
            with pytest.raises(GigaAMHipError, match="host length is shorter"):
                HipEngine.collect(dec)
        R.set_flag(dec, 1)
        assert HipEngine.collect(dec.ids, dec.frames, dec.counts) == (want, False)      # bare tensors: flag unknown
        assert HipEngine.collect(*dec) == (want, False)
        dec.counts[0] = -1
        torch.cuda.synchronize()        # (as in set_flag: the copies are not ordered behind this write)
        HipEngine.ONE_COPY_BYTES = keep
        with pytest.raises(GigaAMHipError, match=r"^decode left an utterance undecoded \(counts = -1\)"):
            HipEngine.collect(dec)
        HipEngine.ONE_COPY_BYTES = 0
        with pytest.raises(GigaAMHipError, match=r"^RNN-T decode left an utterance undecoded \(counts = -1\)"):
            HipEngine.collect(dec)
    finally:
        HipEngine.ONE_COPY_BYTES = keep
