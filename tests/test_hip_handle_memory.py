"""GPU: the handle owns its device memory (gigaam_amd/csrc/gam_api.hip, DESIGN.md "Handle memory").  Destroying a handle gives back
every buffer it grew lazily -- the alignment workspaces and the keyword / hotword / LM tables among them --, and a workspace that was
regrown serves the shapes before and after the growth like a fresh one."""
import numpy as np
import pytest
import torch

from test_hip_ctc_align import _log_probs, _run_op, _target

pytestmark = pytest.mark.gpu

V = 34
LONG_T, LONG_U = 32768, 4096
# the long aligner's backpointer block alone: T * ceil((2U + 1) / 64) * 16 bytes (gam_align_long.h)
W_BYTES = LONG_T * ((2 * LONG_U + 1 + 63) // 64) * 16


def _engine():
    """A fresh op-only engine (no weights), as tests/beam_common.ctc_op_engine builds its cached one."""
    from gigaam_amd import synth
    from gigaam_amd.engine import HipEngine, build_config
    cfg = synth.model_cfg("v2_ctc")
    eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], None), {}, torch.device("cuda:0"))
    eng.set_gemm_mode("f16x3")
    return eng


def _unigram_lm(n_words):
    """A unigram LM over n_words three-letter words of the character vocabulary: small tables, or larger ones."""
    from gigaam_amd import synth
    from gigaam_amd.lm import NgramLM
    letters = synth.CHAR_VOCAB[1:]
    words = [letters[i % 32] + letters[(i // 32) % 32] + letters[(i * 7 + 3) % 32] for i in range(n_words)]
    vocab = ["<s>", "</s>", "<unk>"] + words
    n = len(vocab)
    return NgramLM(vocab, [(np.arange(n, dtype=np.int32).reshape(n, 1), np.full(n, -np.log(n)), np.zeros(n))])


def _phrases(rng, n, length):
    return [[int(c) for c in rng.integers(0, V - 1, length)] for _ in range(n)]


def _exercise(eng, case):
    """Everything that grows a buffer lazily: both CTC aligners' global workspaces and the three tables (set, grown, one cleared)."""
    from beam_common import tokenizer
    out = eng.op_ctc_align_long(case["long_lp"], case["long_y"]).host()
    assert out["status"] == 1
    # S = 2 * 600 + 1 states at T' = 625: the backpointers (190 KB) do not fit the workgroup's LDS -> the global scratch (align_bp)
    h = _run_op(eng, case["bp_lp"], [625, 625], case["bp_y"])
    assert h["status"].shape == (2,)
    tok = tokenizer(V)
    for n in (4, 300):                                  # the second set of each is larger: the grow path
        eng.set_keywords(_phrases(case["rng"], n, 5), -1.0)
        eng.set_hotwords(_phrases(case["rng"], n, 4), 1.5)
        eng.set_lm(case["lm"][n], tok, 0.5, 1.0)
    eng.set_hotwords([])                                # one of them cleared before the handle goes


def test_destroying_a_handle_returns_its_lazily_grown_buffers():
    rng = np.random.default_rng(3)
    case = {"rng": rng,
            "long_lp": torch.from_numpy(_log_probs(rng, 1, LONG_T, V, "flat")[0]).to("cuda:0"), "long_y": _target(rng, LONG_U, V),
            "bp_lp": _log_probs(rng, 2, 625, V, "flat"), "bp_y": [_target(rng, 600, V), _target(rng, 300, V)],
            "lm": {4: _unigram_lm(6), 300: _unigram_lm(900)}}
    free = []
    for _ in range(4):
        eng = _engine()
        _exercise(eng, case)
        eng.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    print("free bytes after each create / exercise / close cycle:", free, "W =", W_BYTES)
    # cycle 1 absorbs what torch's allocator caches; a handle that forgets the long aligner's workspace loses >= 3 W by cycle 4
    assert free[0] - free[3] <= W_BYTES // 2, (free, W_BYTES)


_SHAPES = {"small": (300, 40, 21), "large": (3000, 1400, 22)}      # (T, U, seed); large: three state blocks of 1024, twelve time tiles
_FRESH = {}


def _long_case(name):
    """Inputs of a shape and a FRESH engine's result on them, computed once and shared (read-only)."""
    if name not in _FRESH:
        T, U, seed = _SHAPES[name]
        rng = np.random.default_rng(seed)
        lp, y = torch.from_numpy(_log_probs(rng, 1, T, V, "flat")[0]), _target(rng, U, V)
        eng = _engine()
        ref = eng.op_ctc_align_long(lp, y).host()
        eng.close()
        assert ref["status"] == 1
        _FRESH[name] = (lp, y, ref)
    return _FRESH[name]


@pytest.mark.parametrize("order", [("small", "large", "small"), ("large", "small", "large")])
def test_a_regrown_workspace_serves_every_shape_like_a_fresh_one(order):
    for name in order:
        _long_case(name)
    eng = _engine()
    for name in order:
        lp, y, ref = _long_case(name)
        got = eng.op_ctc_align_long(lp, y).host()
        assert got["status"] == ref["status"] and got["score"] == ref["score"] and got["loglik"] == ref["loglik"], (name, got, ref)
        for k in ("frame_labels", "tok_first", "tok_last"):
            assert np.array_equal(got[k], ref[k]), (name, k)
    eng.close()
    assert not eng._h
