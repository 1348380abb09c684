"""GPU: the RNN-T cluster decode (gam_decode_cluster.h) on heads other than pred_hidden = joint_hidden = 320, against the float64
greedy loop of tests/rnnt_beam_ref.py -- every cluster size C = 1..8 on the six heads of tests/rnnt_cluster_cases.py, which between
them run the five instantiations of gam_rnnt_cluster_kernel that take the sizes as arguments (gam_api.hip rnnt_cluster_kern[4..8]:
NR = 1, 2, 3, 5, 8) and the slicing edges listed there.  The last test of the module fails if one of the five was never launched.

The engines are created with GAM_RNNT_NO_REPAIR=1 (read at gam_create): no repair pass behind the cluster kernel, so a cluster that
gives up leaves counts[b] = -1 here instead of being re-decoded by the one-workgroup kernel, and gam_rnnt_last_decode says which
kernel ran and whether the runtime took the launch -- ids that came from another kernel cannot pass for the cluster kernel's.

Exactness: tests/test_rnnt_cluster_plan_host.py asserts on the CPU that every utterance's smallest top-1 / top-2 margin by the
float64 reference exceeds RNNT_MIN_MARGIN (2e-3), twice the log-prob bar, so no utterance is excused: ids, frames and counts are
compared exactly, every dumped log-prob row within TOL_LOGP of the float64 joint at that step."""
import ctypes as C

import numpy as np
import pytest
import torch

from common import TOL_LOGP, report

import rnnt_cluster_cases as K

pytestmark = pytest.mark.gpu

HEAD_NAMES = sorted(K.HEADS)
DUMP_CAP = K.T_MAX * K.MAX_SYMBOLS      # a frame takes at most max_symbols joint evaluations

_ENGINES = {}       # head -> HipEngine without the repair pass
_KERN_RUN = {}      # (head, C) -> index into rnnt_cluster_kern that gam_rnnt_last_decode reported


def _engine(name, monkeypatch):
    if name not in _ENGINES:
        from gigaam_amd.engine import HipEngine, build_config
        monkeypatch.setenv("GAM_RNNT_NO_REPAIR", "1")
        monkeypatch.delenv("GAM_RNNT_CLUSTER", raising=False)
        monkeypatch.delenv("GAM_RNNT_EXCLUSIVE", raising=False)
        cfg, sd, _, _ = K.inputs(name)
        _ENGINES[name] = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), sd, torch.device("cuda:0"))
    return _ENGINES[name]


def _plan(ncu, cluster, B, name):
    """gam_rnnt_cluster_plan_info of a head: (C, kern)."""
    from gigaam_amd import _lib
    V, H, JH = K.HEADS[name][:3]
    out = (C.c_int32 * 8)()
    assert _lib.load_library().gam_rnnt_cluster_plan_info(ncu, cluster, 0, B, H, JH, V, 1, out) == 0
    return int(out[0]), int(out[2])


def _decode(eng, encoded, lengths, dump):
    dec = eng.rnnt_greedy(torch.from_numpy(encoded), torch.tensor(lengths, dtype=torch.int32), K.MAX_SYMBOLS,
                          dump_cap=DUMP_CAP if dump else 0)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in dec]      # ids, frames, counts (+ dump, dump_count)


def _launch_checked(eng, name, c, B):
    """Set the cluster size; the (C, kern) the decode must report -- or skip when THIS device's CU count makes the planner choose
    fewer workgroups per utterance than a 256-CU device gets."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    want_c, want_kern = _plan(ncu, c, B, name)
    assert _plan(256, c, B, name)[0] == c, (name, c)          # (tests/test_rnnt_cluster_plan_host.py pins the table)
    if want_c < c:
        pytest.skip(f"{ncu} compute units: the planner gives {B} utterances C = {want_c}, not {c}")
    eng.set_rnnt_cluster(c)
    return want_c, want_kern


def _check_against_reference(tag, got, ref_of, lengths):
    """ids / frames / counts exact, the number of joint evaluations, every log-prob row; returns the largest log-prob error."""
    ids, frames, counts, dump, dcount = got
    assert int(counts.min()) >= 0, (tag, counts.tolist())     # no cluster gave up (and none was repaired: GAM_RNNT_NO_REPAIR)
    err = 0.0
    for b in range(len(lengths)):
        r = ref_of(b)
        n = int(counts[b])
        assert n == len(r["ids"]), (tag, b, n, len(r["ids"]))
        assert ids[b, :n].tolist() == r["ids"], (tag, b)
        assert frames[b, :n].tolist() == r["frames"], (tag, b)
        assert int(dcount[b]) == r["lp"].shape[0], (tag, b, int(dcount[b]), r["lp"].shape[0])
        if r["lp"].shape[0]:
            err = max(err, float(np.abs(dump[b, : r["lp"].shape[0]].astype(np.float64) - r["lp"]).max()))
    return err


@pytest.mark.parametrize("c", list(range(1, 9)))
@pytest.mark.parametrize("name", HEAD_NAMES)
def test_cluster_decode_matches_float64_reference(name, c, monkeypatch):
    eng = _engine(name, monkeypatch)
    _, _, encoded, lengths = K.inputs(name)
    ref = K.reference(name)
    want = _launch_checked(eng, name, c, len(lengths))
    got = _decode(eng, encoded, lengths, dump=True)
    ran_c, ran_kern, refused = eng.rnnt_last_decode()
    if ran_c > 0 and not refused:
        _KERN_RUN[(name, c)] = ran_kern
    assert (ran_c, ran_kern, refused) == (want[0], want[1], False), (name, c)
    err = _check_against_reference((name, c), got, lambda b: ref[b], lengths)
    print(f"rnnt cluster head {name} C={c} kern={ran_kern}: max log-prob error {err:.3e}")
    report("rnnt_cluster_matrix", head=name, C=c, kern=ran_kern, logp_err=err)
    assert err < TOL_LOGP, (name, c, err)
    # again, without the dump (two words per frame and member are exchanged instead of three): bit-identical
    again = _decode(eng, encoded, lengths, dump=False)
    assert eng.rnnt_last_decode() == (ran_c, ran_kern, False)
    for x, y in zip(got[:3], again):
        assert np.array_equal(x, y), (name, c)


@pytest.mark.parametrize("name", HEAD_NAMES)
def test_one_workgroup_decode_on_the_same_heads(name, monkeypatch):
    """The one-workgroup kernel (cluster size 0) on the matrix's inputs: its log-prob error beside the cluster kernel's."""
    eng = _engine(name, monkeypatch)
    _, _, encoded, lengths = K.inputs(name)
    ref = K.reference(name)
    eng.set_rnnt_cluster(0)
    got = _decode(eng, encoded, lengths, dump=True)
    assert eng.rnnt_last_decode() == (0, -1, False)
    err = _check_against_reference((name, 0), got, lambda b: ref[b], lengths)
    print(f"rnnt one-workgroup head {name}: max log-prob error {err:.3e}")
    report("rnnt_cluster_matrix", head=name, C=0, kern=-1, logp_err=err)
    assert err < TOL_LOGP, (name, err)


def test_cluster_decode_second_row_of_utterance_columns(monkeypatch):
    """Head C, nine utterances (the six, cycled) at C = 3: a second row of utterance columns (slot / C >= 1), the batch no
    multiple of 8 -- the workgroups of utterances 9..15 leave at once."""
    name, c, B = "C", 3, 9
    eng = _engine(name, monkeypatch)
    _, _, encoded, lengths = K.inputs(name)
    ref = K.reference(name)
    enc9 = np.stack([encoded[b % len(lengths)] for b in range(B)])
    len9 = [lengths[b % len(lengths)] for b in range(B)]
    want = _launch_checked(eng, name, c, B)
    got = _decode(eng, enc9, len9, dump=True)
    assert eng.rnnt_last_decode() == (want[0], want[1], False)
    err = _check_against_reference((name, c, B), got, lambda b: ref[b % len(lengths)], len9)
    report("rnnt_cluster_matrix", head=name, C=c, B=B, kern=want[1], logp_err=err)
    assert err < TOL_LOGP, err
    again = _decode(eng, enc9, len9, dump=False)
    for x, y in zip(got[:3], again):
        assert np.array_equal(x, y)


def test_every_general_instantiation_was_launched():
    """Runs last: the cases above record which instantiation gam_rnnt_last_decode reported.  Between them they must have launched
    all five that take the sizes as arguments -- a change of the planner or of the heads that loses one fails here."""
    assert _KERN_RUN, "the matrix did not run before this test"
    assert set(_KERN_RUN.values()) == {4, 5, 6, 7, 8}, sorted(_KERN_RUN.items())
