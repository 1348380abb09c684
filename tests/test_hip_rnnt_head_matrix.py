"""GPU: RNN-T beam search (gam_rnnt_beam.h) on heads other than pred_hidden = joint_hidden = 320, against the float64 references of
tests/rnnt_beam_ref.py and tests/nbest_ref.py -- the four instantiations of gam_rnnt_beam_kernel (plain, LM, N-best, LM + N-best) on
the heads of tests/rnnt_cluster_cases.py, with the inputs of tests/rnnt_head_cases.py.  Between them the heads and widths make every
member of the kernel's union region the largest once (the LM state and the hotword trie lie behind it), run the wave-tile loops with
1, 3, 21 and 31 tiles and H != JH, both row-tile counts (W <= 16, W > 16) next to their switch (W = 16, 17), and the LDS limit
(H = JH = 512, L = 2, W = 32, S = 16) with the hotword trie in LDS and in global memory.  The last test of the module fails if an
instantiation or a row-tile count was never launched on such a head.

Margin rule (tests/test_hip_rnnt_beam.py): ids / frames are compared on every utterance whose smallest float64 decision margin
exceeds MARGIN (1e-4), score / logp on those within 1e-3 * max(1, |ref|).  The references are read from
tests/golden/rnnt_head_refs.npz (the float64 searches take minutes); tests/test_rnnt_head_cases_host.py runs them again on the CPU,
compares, and holds that at least 90 % of every set qualify."""
import pytest
import torch

import beam_common as BC
import nbest_inputs as I
import rnnt_head_cases as H
from common import report

pytestmark = pytest.mark.gpu

_ENGINES = {}       # (head, L, kind) -> HipEngine
_LAUNCHED = set()   # (LM, N-best, row tiles) of the searches that ran on a head other than 320 / 320


def _engine(name, L, kind):
    key = (name, L, kind)
    if key not in _ENGINES:
        from gigaam_amd.engine import HipEngine, build_config
        cfg, sd, _ = H.head(name, L, kind)
        _ENGINES[key] = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), sd, torch.device("cuda:0"))
    return _ENGINES[key]


def _lm(tmp_path, text, i=0):
    from gigaam_amd import lm as LM
    p = tmp_path / f"lm{i}.arpa"
    p.write_text(text, encoding="utf-8")
    return LM.NgramLM.from_arpa(str(p))


def _clear(eng):
    eng.set_lm(None)
    eng.set_hotwords([])


def _note(name, W, lm, nbest):
    assert H.sizes(name)[1:] != (320, 320)
    _LAUNCHED.add((lm, nbest, 2 if W > 16 else 1))


def _compare(h, b, ref, errs):
    return BC.compare(h, b, ref, errs, H.MARGIN, H.margin_of)


def _compare_nbest(h, b, ref, n_best, errs):
    """tests/test_hip_nbest.py _compare_nbest: the whole list of a qualifying utterance."""
    if not ref["qualifies"]:      # (nbest_ref.qualifies at n_best = W and RNNT_MARGIN, stored with the reference)
        return False
    want = ref["hyps"][:n_best]
    assert int(h["n_hyp"][b]) == len(want), (b, int(h["n_hyp"][b]), len(want))
    for r, w in enumerate(want):
        assert h["rows"][b][r] == (w["ids"], w["frames"]), (b, r, h["rows"][b][r], w)
        for k in ("score", "logp"):
            e = abs(float(h[k][b, r]) - w[k])
            errs[k] = max(errs.get(k, 0.0), e / max(1.0, abs(w[k])))
            assert e <= BC.bar(w[k]), (b, r, k, float(h[k][b, r]), w[k])
    return True


def _finish(tag, ok, n, errs):
    print(f"{tag}: qualified {ok}/{n}, worst relative error {errs}")
    report(tag, qualified=f"{ok}/{n}", **errs)
    assert ok >= 0.9 * n, (tag, ok, n)


@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("name,L", H.HEAD_L)
def test_beam_matches_float64_reference(name, L, kind):
    eng = _engine(name, L, kind)
    errs, n, ok = {}, 0, 0
    try:
        for c in H.beam_cases(name, L, kind):
            eng.set_hotwords(c["phrases"], H.BETA)
            h = BC.run_rnnt_op(eng, c["encp"], H.ENC_LEN, c["W"], c["S"])
            _note(name, c["W"], False, False)
            for b, ref in enumerate(c["refs"]):
                ok += _compare(h, b, ref, errs)
                n += 1
    finally:
        _clear(eng)
    _finish(f"rnnt_head_beam_{name}_L{L}_{kind}", ok, n, errs)


@pytest.mark.parametrize("name,L", H.LM_SETS)
def test_beam_lm_matches_float64_reference(tmp_path, name, L):
    eng = _engine(name, L, "dense")
    tok = BC.tokenizer(H.sizes(name)[0])
    errs, n, ok = {}, 0, 0
    try:
        for i, c in enumerate(H.lm_cases(name, L)):
            eng.set_hotwords(c["phrases"], H.BETA)
            eng.set_lm(_lm(tmp_path, c["arpa"], i), tok, I.LM_ALPHA, I.LM_BETA)
            h = BC.run_rnnt_op(eng, c["encp"], H.ENC_LEN, c["W"], c["S"])
            _note(name, c["W"], True, False)
            for b, ref in enumerate(c["refs"]):
                ok += _compare(h, b, ref, errs)
                n += 1
    finally:
        _clear(eng)
    _finish(f"rnnt_head_beam_lm_{name}_L{L}", ok, n, errs)


@pytest.mark.parametrize("name,L", H.LM_SETS)
def test_beam_lm_with_zero_weights_is_bit_identical_to_no_lm(tmp_path, name, L):
    """The kernel's own contract (gam_rnnt_beam.h): with alpha = beta = 0 every LM term is +0."""
    eng = _engine(name, L, "dense")
    tok = BC.tokenizer(H.sizes(name)[0])
    try:
        for i, c in enumerate(H.lm_cases(name, L)):
            eng.set_hotwords(c["phrases"], H.BETA)
            eng.set_lm(None)
            a = BC.run_rnnt_op(eng, c["encp"], H.ENC_LEN, c["W"], c["S"])
            eng.set_lm(_lm(tmp_path, c["arpa"], i), tok, 0.0, 0.0)
            z = BC.run_rnnt_op(eng, c["encp"], H.ENC_LEN, c["W"], c["S"])
            assert a["rows"] == z["rows"], (name, c["W"], c["S"])
            for k in ("score", "logp"):
                assert a[k].tobytes() == z[k].tobytes(), (name, c["W"], c["S"], k)
    finally:
        _clear(eng)


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("name,L", H.NBEST_SETS)
def test_nbest_matches_float64_reference(tmp_path, name, L, with_lm):
    eng = _engine(name, L, "dense")
    tok = BC.tokenizer(H.sizes(name)[0])
    errs, n, ok = {}, 0, 0
    try:
        eng.set_hotwords([])
        for i, c in enumerate(H.nbest_cases(name, L, with_lm)):
            if with_lm:
                eng.set_lm(_lm(tmp_path, c["arpa"], i), tok, I.LM_ALPHA, I.LM_BETA)
            else:
                eng.set_lm(None)
            h = eng.op_rnnt_beam_nbest(torch.from_numpy(c["encp"]), torch.tensor(H.ENC_LEN, dtype=torch.int32), c["W"], c["S"],
                                       c["W"]).host()
            _note(name, c["W"], with_lm, True)
            for b, ref in enumerate(c["refs"]):
                ok += _compare_nbest(h, b, ref, c["W"], errs)
                n += 1
    finally:
        _clear(eng)
    _finish(f"rnnt_head_nbest_{name}_L{L}_{'lm' if with_lm else 'plain'}", ok, n, errs)


def test_lds_limit_with_the_hotword_trie_in_lds_and_in_global_memory(tmp_path):
    """H = JH = 512, L = 2, W = 32, S = 16: 161296 of the 163840 bytes.  Six phrases (a trie below the 636 words that still fit in
    LDS) and 1024 phrases (read from global memory) against the reference given the same phrases; with the LM the call is refused
    with the byte count."""
    from gigaam_amd._lib import GigaAMHipError
    eng = _engine("A", 2, H.EDGE_KIND)
    small, big = H.edge_cases()
    assert H.trie_words(small["phrases"]) <= H.HW_LDS_WORDS < H.trie_words(big["phrases"])
    errs, n, ok = {}, 0, 0
    try:
        for c in (small, big):
            eng.set_hotwords(c["phrases"], H.BETA)
            h = BC.run_rnnt_op(eng, c["encp"], H.ENC_LEN, c["W"], c["S"])
            _note("A", c["W"], False, False)
            for b, ref in enumerate(c["refs"]):
                ok += _compare(h, b, ref, errs)
                n += 1
        eng.set_hotwords([])
        need = H.rb_lds_bytes("A", 2, *H.WS_EDGE, with_lm=True)
        eng.set_lm(_lm(tmp_path, H.lm_cases("A", 2)[0]["arpa"]), BC.tokenizer(34), 0.5, 1.0)
        with pytest.raises(GigaAMHipError, match=f"with the LM need {need} bytes"):
            BC.run_rnnt_op(eng, small["encp"], H.ENC_LEN, *H.WS_EDGE)
    finally:
        _clear(eng)
    _finish("rnnt_head_beam_lds_limit", ok, n, errs)


def test_beam_is_bit_identical_run_to_run_and_on_another_stream():
    eng = _engine("E", 1, "dense")
    c = H.beam_cases("E", 1, "dense")[-1]
    try:
        eng.set_hotwords(c["phrases"] or [[1, 2], [5], [7, 7, 3]], H.BETA)
        a = BC.run_rnnt_op(eng, c["encp"], H.ENC_LEN, c["W"], c["S"])
        b = BC.run_rnnt_op(eng, c["encp"], H.ENC_LEN, c["W"], c["S"])
        with torch.cuda.stream(torch.cuda.Stream()):
            s = BC.run_rnnt_op(eng, c["encp"], H.ENC_LEN, c["W"], c["S"])
        torch.cuda.synchronize()
    finally:
        _clear(eng)
    for o in (b, s):
        assert a["rows"] == o["rows"]
        for k in ("score", "logp"):
            assert a[k].tobytes() == o[k].tobytes(), k


def test_every_instantiation_and_row_tile_count_was_launched():
    """Runs last: all four instantiations (LM x N-best) at one and at two row tiles on a head other than 320 / 320."""
    assert _LAUNCHED, "the matrix did not run before this test"
    assert _LAUNCHED == {(lm, nb, rt) for lm in (False, True) for nb in (False, True) for rt in (1, 2)}, sorted(_LAUNCHED)
