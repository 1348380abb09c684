"""CPU: what tests/rnnt_head_cases.py promises the GPU tests of the RNN-T stack on heads other than 320 / 320 -- from the float64
references and the transcribed LDS formulas alone.  At least 90 % of every set's utterances decide by more than the op-level margin
(so the GPU tests compare them exactly); the chosen heads and widths make every member of gam_rnnt_beam.h's union region the strict
maximum once and reach the LDS limit; the hotword tries of the LDS-edge test lie on both sides of the words that still fit; the
confidence paths are valid except the rows made invalid on purpose."""
import numpy as np
import pytest

import confidence_ref as CF
import nbest_ref as N
import rnnt_beam_ref as R
import rnnt_head_cases as H


def test_margins_are_the_projects_op_level_margins():
    assert H.MARGIN == 1e-4 == N.RNNT_MARGIN       # tests/test_hip_rnnt_beam.py MARGIN


def _same(stored, computed, what):
    """The stored references are what the float64 searches give here: ids, frames, phrases and the ARPA text exactly, the values to
    1e-9 (another BLAS may order a sum differently)."""
    def near(a, b):
        return a == b or abs(a - b) <= 1e-9 * max(1.0, abs(a))
    assert len(stored) == len(computed), what
    for i, (s, c) in enumerate(zip(stored, computed)):
        assert s.get("phrases") == c.get("phrases") and s.get("arpa") == c.get("arpa"), (what, i)
        for b, (rs, rc) in enumerate(zip(s["refs"], c["refs"])):
            for hs, hc in zip(rs.get("hyps", [rs]), rc.get("hyps", [rc])):
                assert hs["ids"] == hc["ids"] and hs["frames"] == hc["frames"], (what, i, b)
                assert near(hs["score"], hc["score"]) and near(hs["logp"], hc["logp"]), (what, i, b)
            assert len(rs.get("hyps", [])) == len(rc.get("hyps", [])) and rs.get("qualifies") == rc.get("qualifies"), (what, i, b)
            if "margin" in rs:
                assert near(rs["margin"], rc["margin"]) and (rs["margin"] > H.MARGIN) == (rc["margin"] > H.MARGIN), (what, i, b)


def _tokens(cases):
    return sum(len(r["ids"]) for c in cases for r in c["refs"])


@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("name,L", H.HEAD_L)
def test_beam_sets_qualify(name, L, kind):
    cases = H.compute_beam(name, L, kind)
    _same(H.stored_refs()[H.set_key("beam", name, L, kind)], cases, (name, L, kind))
    assert len(cases) == len(H.combos(name, L))
    assert [bool(c["phrases"]) for c in cases] == [i % 2 == 1 for i in range(len(cases))]      # hotwords on every second one
    ok, n = H.share(cases)
    assert n == 4 * len(cases) and ok >= 0.9 * n, (name, L, kind, ok, n)
    tokens, frames = _tokens(cases), sum(H.ENC_LEN) * len(cases)
    if kind == "dense":       # emission-heavy: more tokens than frames; blank-dominant: some, and fewer than the dense set emits
        assert tokens > frames, (name, L, tokens, frames)
    else:
        assert 0 < tokens < _tokens(H.beam_cases(name, L, "dense")), (name, L, tokens)
    V = H.sizes(name)[0]
    assert all(0 <= t <= V - 2 for c in cases for p in c["phrases"] for t in p)


@pytest.mark.parametrize("name,L", H.LM_SETS)
def test_lm_sets_qualify_and_the_lm_changes_a_score(name, L):
    cases = H.compute_lm(name, L)
    _same(H.stored_refs()[H.set_key("lm", name, L)], cases, (name, L))
    ok, n = H.share(cases)
    assert ok >= 0.9 * n, (name, L, ok, n)
    assert any(r["score"] != r["logp"] for c in cases for r in c["refs"])
    for c, (W, S, _) in zip(cases, H.LM_WS):
        assert H.rb_lds_bytes(name, L, W, S, with_lm=True, hw_words=H.trie_words(c["phrases"])) <= H.LDS_LIMIT


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("name,L", H.NBEST_SETS)
def test_nbest_sets_qualify(name, L, with_lm):
    cases = H.compute_nbest(name, L, with_lm)
    _same(H.stored_refs()[H.set_key("nbest_lm" if with_lm else "nbest", name, L)], cases, (name, L, with_lm))
    ok, n = H.share(cases, nbest=True)
    assert ok >= 0.9 * n, (name, L, with_lm, ok, n)
    assert max(len(r["hyps"]) for c in cases for r in c["refs"]) > 16      # lists longer than one row tile
    for W, S in H.WS:
        assert H.rb_lds_bytes(name, L, W, S, with_lm=with_lm) <= H.LDS_LIMIT


def test_lds_edge_sets_qualify_and_their_tries_lie_on_both_sides_of_the_lds_room():
    cases = H.compute_edge(H.beam_cases("A", 2, H.EDGE_KIND)[-1]["refs"])
    _same(H.stored_refs()["edge"], cases, "edge")
    small, big = cases
    assert len(small["phrases"]) == 6 and len(big["phrases"]) == 1024
    assert H.trie_words(small["phrases"]) <= H.HW_LDS_WORDS == 636 < H.trie_words(big["phrases"])
    ok, n = H.share(cases)
    assert ok >= 0.9 * n, (ok, n)
    assert any(a["score"] != a["logp"] for a in small["refs"])        # a phrase was met


def test_union_region_every_member_is_the_strict_maximum_once():
    """gam_rb_union_bytes is the maximum of the joint rows, the candidates and the hidden rows; the LM state and the hotword trie are
    carved behind it.  If the kernel's carve changes, this transcription changes with it."""
    winners = {}
    for name, L in H.HEAD_L:
        V, Hh, JH = H.sizes(name)
        for W, S in H.combos(name, L):
            m = H.rb_union_members(W, min(W, V - 1), Hh, JH, L)
            top = [i for i in range(3) if m[i] == max(m)]
            if len(top) == 1:
                winners.setdefault(top[0], set()).add((name, L, W))
            assert H.rb_lds_bytes(name, L, W, S) <= H.LDS_LIMIT, (name, L, W, S)
    assert {n for n, _, _ in winners[1]} >= {"C", "D"}                           # the candidates
    assert ("C", 1, 32) in winners[1] and ("D", 1, 8) in winners[1] and ("D", 1, 4) not in winners[1]
    assert H.rb_union_members(32, 32, 48, 64, 1)[:2] == (8704, 24576)
    assert any(n == "E" and L == 1 for n, L, _ in winners[2])                    # the hidden rows at L = 1 (H > JH)
    assert all(n == "E" for n, L, _ in winners[2] if L == 1)
    assert any(n == "F" and L == 1 for n, L, _ in winners[0])                    # the joint rows


def test_lds_limit_configuration():
    """H = JH = 512, L = 2, W = 32, S = 16: the largest accepted configuration; the LM's carve does not fit beside it."""
    assert H.rb_lds_bytes("A", 2, 32, 16) == 161296
    assert H.rb_lds_bytes("A", 2, 32, 16, with_lm=True) > H.LDS_LIMIT == 163840
    assert H.rb_lds_bytes("A", 2, 32, 10) == 152048 and H.rb_lds_bytes("A", 2, 32, 10, with_lm=True) == 167072   # (tests/test_hip_rnnt_beam_lm.py)
    assert H.rb_lds_bytes("A", 2, 32, 16, hw_words=636) == H.LDS_LIMIT


@pytest.mark.parametrize("name,L", H.CONF_SETS)
def test_confidence_paths_are_valid_except_the_rows_made_invalid(name, L):
    _, _, hd, encp, lengths = H.conf_head(name, L)
    V = H.sizes(name)[0]
    paths = H.conf_paths(name, L)
    for which in ("greedy", "random"):
        assert len(paths[which]) == len(lengths)
        for b, (ids, frames) in enumerate(paths[which]):
            assert CF.valid(ids, frames, lengths[b], V, False), (name, L, which, b)
    assert sum(len(i) for i, _ in paths["greedy"]) > 16
    assert [len(i) for i, _ in paths["random"]] == H.CONF_U and {0, 1, 16, 17, 33} <= set(H.CONF_U)
    assert any(len(set(f)) < len(f) for _, f in paths["random"])                  # several tokens on one frame
    got = [int(CF.valid(i, f, lengths[b], V, False)) for b, (i, f) in enumerate(paths["invalid"])]
    assert got == H.INVALID_STATUS
    ids1, fr1 = paths["invalid"][1]
    assert CF.valid(paths["random"][1][0], fr1, lengths[1], V, False) and max(ids1) == V - 1       # row 1: only the id is wrong
    ids2, fr2 = paths["invalid"][2]
    assert all(0 <= f < lengths[2] for f in fr2) and fr2 != sorted(fr2) and ids2 == paths["random"][2][0]      # row 2: only the order
    # a width-8 beam's rows (the GPU test takes the kernel's own) are valid paths too
    for b in (1, 3):
        r = R.beam_search(hd, encp[b].astype(np.float64), 8, 3, lengths[b])
        assert CF.valid(r["ids"], r["frames"], lengths[b], V, False)


def test_joint_inputs():
    for name in H.JOINT_HEADS:
        enc, labels = H.joint_inputs(name)
        V, Hh, JH = H.sizes(name)
        assert enc.shape[:2] == (2, 5) and len(labels) == 2 and all(len(r) == 3 and max(r) <= V - 2 for r in labels)
        assert Hh % 32 == 16 and JH % 32 in (0, 16)       # the K of the pp GEMM is no multiple of 32 on these heads
