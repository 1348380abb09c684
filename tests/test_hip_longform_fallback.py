"""GPU: the fp32 rerun of every file-level longform route.  A 2-layer CTC model whose FFN hidden leaves fp16's range (the construction
of test_hip_range.test_range_flag_and_fp32_fallback) raises the split-fp16 range flag on every encoder batch; each route must then
warn once, redo the whole file under GAM_GEMM_F32 -- a stream route on a NEW stream -- and restore the arithmetic.  The expectation
is the same call on a model of the same weights that runs in f32 throughout: the rerun IS that computation, so every comparison is
exact.  The file is cut into two windows: one feeder batch at ``fr_batch_size=2``, and two -- a second push into a stream that a first
batch began -- at ``fr_batch_size=1``; both are run.  The packer joins the two speech regions into one chunk: the region routes run one
batch."""
import warnings

import pytest

from test_hip_ctc_align import _wav_file

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EXPONENT = 16      # the FFN hidden times 2^16 (as test_range_flag_and_fp32_fallback): every route's first pass raises the flag
WINDOWS = dict(vad="windows", chunk_length_s=6.0, stride_length_s=1.0, fr_batch_size=2)
WINDOWS_TWO_BATCHES = dict(WINDOWS, fr_batch_size=1)
REGIONS = dict(speech_regions=[(0.0, 4.0), (4.5, 9.0)])


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """(the model whose split-fp16 run overflows, the same weights in f32, the file, keywords and a text from the f32 greedy decode)"""
    import gigaam_amd
    from gigaam_amd import synth
    ck = synth.make_checkpoint("v2_ctc", seed=1, n_layers=2)
    sd = {k: v.clone() for k, v in ck["state_dict"].items()}
    for i in range(ck["cfg"]["encoder"]["n_layers"]):     # hidden * 2^EXPONENT, undone by linear2: the same function
        p = f"encoder.layers.{i}.feed_forward1."
        sd[p + "linear1.weight"] *= 2.0 ** EXPONENT
        sd[p + "linear1.bias"] *= 2.0 ** EXPONENT
        sd[p + "linear2.weight"] *= 2.0 ** -EXPONENT
    model = gigaam_amd.model_from_checkpoint({"cfg": ck["cfg"], "state_dict": sd}, DEV)
    model32 = gigaam_amd.model_from_checkpoint({"cfg": ck["cfg"], "state_dict": sd}, DEV)
    model32.set_arithmetic("f32")
    path = _wav_file(tmp_path_factory.mktemp("fallback"), 9.0, 17)
    text = " ".join(s.text for s in model32.transcribe_longform(path, **WINDOWS).segments)
    assert len(model32.decoding.tokenizer.encode(text)) > 8, text
    # (the synthetic model's "words" run long: a keyword is the first six characters of one)
    keywords = [w[:6] for w in text.split() if len(w) >= 2][:3] + [text[:3]]
    return model, model32, path, keywords, text


ROUTES = {
    "transcribe_regions": lambda m, path, kws, text: m.transcribe_longform(path, word_timestamps=True, **REGIONS),
    "transcribe_windows": lambda m, path, kws, text: m.transcribe_longform(path, word_timestamps=True, **WINDOWS),
    "transcribe_windows_beam": lambda m, path, kws, text: m.transcribe_longform(path, word_timestamps=True, stream_search=True, beam_size=4,
                                                                               **WINDOWS),
    "keywords_regions": lambda m, path, kws, text: m.find_keywords_longform(path, kws, threshold=0.3, **REGIONS),
    "keywords_windows": lambda m, path, kws, text: m.find_keywords_longform(path, kws, threshold=0.3, **WINDOWS),
    "align_regions": lambda m, path, kws, text: m.align_longform(path, text, **REGIONS),
    "align_windows": lambda m, path, kws, text: m.align_longform(path, text, **WINDOWS),
    # the windowed routes again, one window per feeder batch
    "transcribe_windows_two_batches": lambda m, path, kws, text: m.transcribe_longform(path, word_timestamps=True, **WINDOWS_TWO_BATCHES),
    "transcribe_windows_beam_two_batches": lambda m, path, kws, text: m.transcribe_longform(path, word_timestamps=True, stream_search=True,
                                                                                           beam_size=4, **WINDOWS_TWO_BATCHES),
    "keywords_windows_two_batches": lambda m, path, kws, text: m.find_keywords_longform(path, kws, threshold=0.3, **WINDOWS_TWO_BATCHES),
    "align_windows_two_batches": lambda m, path, kws, text: m.align_longform(path, text, **WINDOWS_TWO_BATCHES),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_file_is_recomputed_in_fp32(case, route):
    model, model32, path, keywords, text = case
    call = ROUTES[route]
    eng = model.encoder.engine
    with warnings.catch_warnings(record=True) as w32:
        warnings.simplefilter("always")
        want = call(model32, path, keywords, text)
    assert not [x for x in w32 if "recomputed" in str(x.message)]
    before = eng.gemm_mode
    assert before != "f32"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = call(model, path, keywords, text)
    said = [str(x.message) for x in w if "the file was recomputed" in str(x.message)]
    print(route, "warnings:", len(said), "mode:", before, "->", eng.gemm_mode, "equal:", got == want)
    assert len(said) == 1, [str(x.message) for x in w]
    assert eng.gemm_mode == before
    assert type(got) is type(want) and got == want
    # nothing is compared on an empty result
    if route.startswith("transcribe"):
        assert len(got.segments) >= 1 and all(s.text and s.words for s in got.segments)
    elif route.startswith("keywords"):
        assert len(got.hits) >= 2
    else:
        assert got.feasible and len(got.token_ids) > 8 and len(got.token_frames) == len(got.token_ids)
