"""CPU: the host side of GigaAMASR.align_longform -- the frame -> (region, local frame, time) mapping, the word / segment assignment,
the result type, and the ctypes declarations of the three new entry points against the header."""
import ctypes as C
import os
import re

import pytest

from common import ROOT

from gigaam_amd import _lib, synth
from gigaam_amd.decoding import Tokenizer
from gigaam_amd.timestamps_utils import concat_frames_to_segments, frames_to_words, longform_words
from gigaam_amd.types import LongformAlignmentResult, Segment, Word


def test_concatenated_frames_map_back_to_region_local_frame_and_time():
    seg_frames, starts, shifts = [5, 0, 3, 4], [1.0, 7.0, 10.0, 20.0], [0.04, 0.0, 0.05, 0.1]
    frames = [0, 4, 5, 7, 8, 11]
    segs, local, times = concat_frames_to_segments(frames, seg_frames, starts, shifts)
    assert segs == [0, 0, 2, 2, 3, 3]                      # the region without frames is skipped over
    assert local == [0, 4, 0, 2, 0, 3]
    assert times == pytest.approx([1.0, 1.16, 10.0, 10.1, 20.0, 20.3])
    assert concat_frames_to_segments([], seg_frames, starts, shifts) == ([], [], [])
    for bad in (12, -1):
        with pytest.raises(ValueError):
            concat_frames_to_segments([bad], seg_frames, starts, shifts)


def test_words_take_file_times_and_go_to_the_region_of_their_first_token():
    tok = Tokenizer(synth.CHAR_VOCAB)
    text = "да нет ой"
    ids = tok.encode(text)
    bounds = [(1.0, 2.0), (5.0, 6.0), (9.0, 9.5)]
    shifts = [0.1, 0.2, 0.05]
    #        д  а  ' ' н  е | т  ' ' о  й      ("нет" starts in region 0 and ends in region 1; region 2 gets nothing)
    segs = [0, 0, 0, 0, 0, 1, 1, 1, 1]
    local = [1, 3, 4, 6, 9, 0, 2, 3, 4]
    words, segments = longform_words(tok, ids, segs, local, bounds, shifts)
    assert [w.text for w in words] == ["да", "нет", "ой"]
    assert words[0] == Word("да", 1.1, 1.4)                # first token's frame .. one past the last token's frame, as frames_to_words
    assert words[1] == Word("нет", 1.6, 5.2)               # starts in region 0, ends in region 1
    assert words[2] == Word("ой", 5.6, 6.0)
    assert [s.text for s in segments] == ["да нет", "ой", ""]
    assert [(s.start, s.end) for s in segments] == bounds
    assert segments[0].words == words[:2] and segments[1].words == words[2:] and segments[2].words == []
    # one region: the rule is frames_to_words' own
    one = frames_to_words(tok, ids, list(range(0, 18, 2)), 0.04)
    got, _ = longform_words(tok, ids, [0] * 9, list(range(0, 18, 2)), [(0.0, 1.0)], [0.04])
    assert [(w.text, round(w.start, 3), round(w.end, 3)) for w in one] == [(w.text, w.start, w.end) for w in got]


def test_longform_alignment_result_prints_its_text():
    seg = Segment(text="да", start=0.0, end=1.0, words=[Word("да", 0.1, 0.3)])
    res = LongformAlignmentResult(text="да", words=seg.words, token_ids=[4, 0], token_segments=[0, 0], token_frames=[2, 6],
                                  token_times=[0.08, 0.24], score=-1.5, log_likelihood=-1.25, segments=[seg], feasible=True)
    assert str(res) == "да" and len(res) == 1 and list(res) == [seg]
    import gigaam_amd
    assert gigaam_amd.LongformAlignmentResult is LongformAlignmentResult


_CTYPES = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}


def _header_signature(name):
    header = open(os.path.join(ROOT, "include", "gigaam_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in the header"
    out = []
    for arg in m.group(1).split(","):
        arg = arg.strip()
        if "*" in arg:
            out.append(C.c_void_p)
        else:
            out.append(_CTYPES[arg.replace("const ", "").split()[0]])
    return out


@pytest.mark.parametrize("name", ["gam_op_ctc_align_long", "gam_set_ctc_align_workspace", "gam_tune_ctc_align_long"])
def test_lib_declares_the_new_symbols_with_the_headers_signature(name):
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int
    assert argtypes == _header_signature(name)
    if name == "gam_op_ctc_align_long":
        assert argtypes[2] is C.c_int64 and len(argtypes) == 13      # T is 64-bit; score / loglik are pointers (to double)
