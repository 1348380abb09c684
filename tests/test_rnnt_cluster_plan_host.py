"""Host: what gam_rnnt_greedy's planner (gam_api.hip rnnt_cluster_plan, read through gam_rnnt_cluster_plan_info) does with a head,
pinned as literals, and the inputs of the GPU matrix (tests/test_hip_rnnt_cluster_matrix.py) judged by the float64 reference alone.

The plan table is NOT computed by a Python copy of the rule: a copy would follow any change of the rule.  It says which of the nine
instantiations of gam_rnnt_cluster_kernel (rnnt_cluster_kern[0..8]) a head runs at every cluster size -- the GPU matrix relies on it
to reach [4..8] -- and which slices are cached in LDS."""
import ctypes as C

import numpy as np
import pytest

from common import RNNT_MIN_MARGIN

import rnnt_cluster_cases as K

KIB = 1024

# head -> (V, H, JH), kern / wout_slice_in_lds / wpred_slice_in_lds at C = 1..8 (ncu = 256, B = 4, L = 1, exclusive = 0)
PLAN = {
    "A": ((34, 512, 512), [8, 7, 6, 5, 5, 5, 5, 4], [0] * 8, [0] * 8),
    "B": ((257, 256, 512), [7, 5, 5, 4, 4, 4, 4, 4], [0] * 8, [0] * 7 + [1]),
    "C": ((34, 48, 64), [4] * 8, [1] * 8, [1] * 8),
    "D": ((34, 16, 16), [4] * 8, [1] * 8, [1] * 8),
    "E": ((130, 496, 336), [8, 7, 6, 5, 5, 5, 5, 4], [0] * 8, [0] * 7 + [1]),
    "F": ((1025, 320, 512), [7, 6, 5, 5, 4, 4, 4, 4], [0] * 8, [0] * 8),
    "h320": ((34, 320, 320), [3, 2, 1, 1, 0, 0, 0, 0], [0, 0, 1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 1, 1, 1]),
}
NR_OF_KERN = [1, 2, 3, 5, 1, 2, 3, 5, 8]      # gate-row slots per thread of rnnt_cluster_kern[k]


def plan(ncu, cluster, exclusive, B, H, JH, V, L):
    """gam_rnnt_cluster_plan_info as a dict."""
    from gigaam_amd import _lib
    out = (C.c_int32 * 8)()
    assert _lib.load_library().gam_rnnt_cluster_plan_info(ncu, cluster, exclusive, B, H, JH, V, L, out) == 0
    return dict(zip(("C", "nr", "kern", "resident", "wout", "wpred", "lds", "grid"), (int(v) for v in out)))


def test_cluster_plan_table():
    seen_kern, seen_wout, seen_wpred = set(), set(), set()
    for name, ((V, H, JH), kern, wout, wpred) in PLAN.items():
        assert name == "h320" or K.HEADS[name][:3] == (V, H, JH)      # the GPU matrix decodes these very heads
        for c in range(1, 9):
            p = plan(256, c, 0, 4, H, JH, V, 1)
            assert p["C"] == c, (name, c, p)
            assert (p["kern"], p["wout"], p["wpred"]) == (kern[c - 1], wout[c - 1], wpred[c - 1]), (name, c, p)
            assert p["nr"] == NR_OF_KERN[p["kern"]], (name, c, p)
            assert p["resident"] == (1 if p["kern"] == 0 else 0), (name, c, p)
            assert 0 < p["lds"] <= 160 * KIB, (name, c, p)
            assert p["grid"] == 8 * 1 * c, (name, c, p)               # 8 * ceil(B / 8) * C
            seen_kern.add(p["kern"]); seen_wout.add(p["wout"]); seen_wpred.add(p["wpred"])
    assert seen_kern == set(range(9)) and seen_wout == {0, 1} and seen_wpred == {0, 1}
    assert plan(256, 1, 0, 4, 320, 512, 1025, 1)["lds"] == 149312     # F at C = 1: next to the 160 KiB limit


def test_cluster_plan_grid_and_limits():
    for B in (1, 8, 9, 16, 17, 24):
        for c in (1, 2, 3):
            p = plan(256, c, 0, B, 48, 64, 34, 1)
            assert p["C"] == c and p["grid"] == 8 * ((B + 7) // 8) * c, (B, c, p)
    assert plan(256, -1, 0, 4, 512, 512, 34, 1)["C"] == 8             # the automatic size of a small batch
    assert plan(256, -1, 0, 32, 320, 320, 34, 1)["C"] == 7            # 32 utterances: 224 of 256 CUs
    assert plan(256, 3, 0, 9, 48, 64, 34, 1)["grid"] == 48            # two rows of utterance columns
    for cluster in (-1, 8):                                           # a 64-CU partition: C <= (64 - 16) / 8
        assert plan(64, cluster, 0, 4, 320, 320, 34, 1)["C"] == 6
        assert plan(64, cluster, 0, 4, 512, 512, 34, 1)["C"] == 6
    zeros = dict(C=0, nr=0, kern=0, resident=0, wout=0, wpred=0, lds=0, grid=0)
    assert plan(16, -1, 0, 4, 320, 320, 34, 1) == zeros               # no CU to spare: the one-workgroup kernel
    assert plan(256, -1, 0, 4, 320, 320, 34, 2) == zeros              # two predictor layers: the one-workgroup kernel
    assert plan(256, 0, 0, 4, 320, 320, 34, 1) == zeros               # asked for
    for name, ((V, H, JH), _, _, _) in PLAN.items():                  # GAM_RNNT_EXCLUSIVE=1: the CU's whole LDS
        for c in (1, 8):
            p = plan(256, c, 1, 4, H, JH, V, 1)
            assert p["C"] == c and p["lds"] == 160 * KIB, (name, c, p)


@pytest.mark.parametrize("name", sorted(K.HEADS))
def test_matrix_inputs_are_clean_by_the_float64_reference(name):
    """What the head's seed and blank bias were picked for (rnnt_cluster_cases.HEADS): no utterance has a near-tie, so none is
    excused on the GPU; utterance 0 has a blank run of more than two 16-frame windows; frames hit max_symbols; tokens and blank
    frames both occur."""
    ref = K.reference(name)
    lengths = K.inputs(name)[3]
    assert lengths == [60, 33, 17, 16, 1, 0] and K.MAX_SYMBOLS == 3
    for b, r in enumerate(ref):
        assert r["margin"] > RNNT_MIN_MARGIN, (name, b, r["margin"])
        assert len(r["per_frame"]) == lengths[b] and sum(r["per_frame"]) == len(r["ids"]) == len(r["frames"])
        assert r["lp"].shape[0] == sum(n + (n < K.MAX_SYMBOLS) for n in r["per_frame"])      # joint evaluations
    assert np.isinf(ref[5]["margin"]) and ref[5]["ids"] == []         # (length 0: no joint step at all)
    assert K.longest_blank_run(ref[0]["per_frame"]) >= 33
    assert sum(1 for r in ref for n in r["per_frame"] if n == K.MAX_SYMBOLS) >= 1
    assert sum(len(r["ids"]) for r in ref) > 0 and sum(1 for r in ref for n in r["per_frame"] if n == 0) > 0
