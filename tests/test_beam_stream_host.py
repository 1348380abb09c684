"""CPU: the host side of the resumable CTC beam search (gam_op_ctc_beam_stream): the packed result's layout and its host views, the
ctypes declarations against the header, the constants the header and the kernel share, and the keyword errors of
``transcribe_longform(stream_search=True)`` that need no GPU."""
import ctypes as C
import os
import re

import pytest
import torch

from common import ROOT

from gigaam_amd import _lib

_CTYPES = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}


def test_packed_result_layout_has_f64_on_even_words_and_the_flag_word_last():
    from gigaam_amd.engine import BeamStreamDecoded, _Packed
    assert issubclass(BeamStreamDecoded, _Packed)
    for mf in (0, 1, 7, 90000):
        fields, sizes, words = BeamStreamDecoded.layout(mf)
        by = {name: (o, n, dtype) for name, o, n, _, dtype in fields}
        assert set(by) == {"ids", "frames", "count", "score", "logp", "status", "ext"}
        for name in ("score", "logp"):
            o, n, dtype = by[name]
            assert dtype is torch.float64 and n == 2 and o % 2 == 0, (name, o)
        assert by["ids"][1] == by["frames"][1] == max(mf, 1) and by["count"][1] == by["status"][1] == 1
        assert by["ext"][0] == words - 1 and by["ext"][1] == 1                     # the flag word is the last word
        assert sum(sizes) == words == 2 * max(mf, 1) + 7      # (an empty stream keeps one word each: the library takes no NULL buffer)
        # the small block ``host`` copies first holds score, logp, count and status and nothing else
        head = sorted(o for name, (o, n, _) in by.items() if name in ("score", "logp", "count", "status") for o in range(o, o + n))
        assert head == list(range(BeamStreamDecoded.HEAD_WORDS))


def test_packed_result_host_returns_the_views():
    from gigaam_amd._lib import GigaAMHipError
    from gigaam_amd.engine import BeamStreamDecoded
    mf = 9
    out = BeamStreamDecoded.empty(torch.device("cpu"), mf)
    out.whole.fill_(-7)
    out.score[0], out.logp[0] = -12.5, -13.25
    out.count[0], out.status[0] = 3, 1
    out.ids[:4] = torch.tensor([5, 6, 7, 99], dtype=torch.int32)
    out.frames[:4] = torch.tensor([0, 4, 2_000_000_000, 99], dtype=torch.int32)
    out.ext[0] = 1
    h = out.host()
    assert h["ids"].tolist() == [5, 6, 7] and h["frames"].tolist() == [0, 4, 2_000_000_000]
    assert (h["count"], h["status"], h["score"], h["logp"], h["flag"]) == (3, 1, -12.5, -13.25, True)
    assert out.flag_word().data_ptr() == out.whole[-1:].data_ptr()
    # a refused stream raises; unchecked it gives no tokens, whatever ``count`` holds
    out.status[0] = 0
    out.ext[0] = 0
    with pytest.raises(GigaAMHipError, match="refused"):
        out.host()
    h = out.host(check=False)
    assert h["status"] == 0 and h["count"] == 0 and h["ids"].shape == (0,) and h["flag"] is False


@pytest.mark.parametrize("name,ret", [("gam_op_ctc_beam_stream", "int"), ("gam_ctc_beam_stream_bytes", "int64_t")])
def test_lib_declares_the_stream_symbols_with_the_headers_signature(name, ret):
    header = open(os.path.join(ROOT, "include", "gigaam_hip.h")).read()
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in the header"
    want = [C.c_void_p if "*" in a else _CTYPES[a.strip().replace("const ", "").split()[0]] for a in m.group(1).split(",")]
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is _CTYPES[ret] and argtypes == want
    from gigaam_amd.engine import BeamStream
    assert (BeamStream.BEGIN, BeamStream.END) == tuple(int(re.search(r"#define GAM_BEAM_STREAM_" + f + r"\s+(\d+)", header).group(1))
                                                       for f in ("BEGIN", "END"))


def test_the_kernel_header_agrees_with_the_public_header():
    src = open(os.path.join(ROOT, "gigaam_amd", "csrc", "gam_beam_stream.h")).read()
    header = open(os.path.join(ROOT, "include", "gigaam_hip.h")).read()
    for f, v in (("BEGIN", 1), ("END", 2)):
        assert int(re.search(r"#define GAM_BEAM_F_" + f + r"\s+(\d+)", src).group(1)) == v
    r = int(re.search(r"#define GAM_BEAM_STREAM_REBASE\s+(\d+)", src).group(1))
    assert r & (r - 1) == 0 and 1 <= r <= 8192
    from gigaam_amd.engine import HipEngine
    assert HipEngine.BEAM_STREAM_REBASE == r
    assert f"T <= {r} frames" in header and f"every {r} stream frames" in header


def test_stream_search_keyword_errors_need_no_gpu():
    import gigaam_amd
    from gigaam_amd import synth
    ctc = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=1, n_layers=1), "cpu")
    rnnt = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_rnnt", seed=1, n_layers=1), "cpu")
    path = "no-such-file.wav"       # (every error below is raised before the file is opened)
    for kw in (dict(beam_size=4), dict(hotwords=["да"]), dict(lm="missing.arpa")):
        with pytest.raises(ValueError, match="8192.*stream_search"):
            ctc.transcribe_longform(path, vad="windows", **kw)
        with pytest.raises(ValueError, match='stream_search=True searches the stitched stream of vad="windows"'):
            ctc.transcribe_longform(path, stream_search=True, speech_regions=[(0.0, 1.0)], **kw)
    with pytest.raises(ValueError, match="stream_search=True needs beam_size, hotwords or lm"):
        ctc.transcribe_longform(path, vad="windows", stream_search=True)
    with pytest.raises(ValueError, match="speech_regions"):
        ctc.transcribe_longform(path, vad="windows", stream_search=True, beam_size=4, speech_regions=[(0.0, 1.0)])
    with pytest.raises(TypeError, match="windowed longform needs a CTC head"):
        rnnt.transcribe_longform(path, vad="windows", stream_search=True, beam_size=4)
