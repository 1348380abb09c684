"""GPU: transducer forced alignment (gam_rnnt_align / gam_op_rnnt_align / gam_op_rnnt_lattice_align, gigaam_amd/csrc/gam_rnnt_align.h)
against the float64 reference of tests/rnnt_align_ref.py.

Method (as tests/test_hip_ctc_align.py): a returned path is checked for VALIDITY and its RESCORE under the float64 lattice against the
float64 optimum, not for equality with the reference's path -- where two paths score within rounding of each other the kernel (fp32)
and the reference (fp64) may keep either, and both are right.  So near-ties need no exclusion and no utterance is left out.  Exact
paths are asserted where the arithmetic is exact: dyadic lattices through gam_op_rnnt_lattice_align.
Bars, the project's own: |score - ref| and |loglik - ref| <= 1e-3 * max(1, |ref|); stored (lb, le) within 1e-3 of the reference
(the RNN-T log-prob bar of the parity tests, common.TOL_LOGP)."""
import os

import numpy as np
import pytest
import torch

from beam_common import bar as _bar, encp as _encp, small_rnnt_model, wav_file as _wav_file
from common import ROOT, TOL_LOGP, load_case, report, split_ragged

import rnnt_align_ref as A
import rnnt_beam_ref as R

pytestmark = pytest.mark.gpu

MODES = ["f16x3", "f32"]
RNNT_CASES = ["v1_rnnt_l2", "v2_rnnt_l2", "v3_rnnt_l2", "v3_e2e_rnnt_l2", "v2_rnnt_l2_dense", "v2_rnnt_l2_lstm2", "v3_e2e_rnnt_l2_dense"]
# the cases where the reference's best path of the golden ids is the greedy decode's on at least one utterance (checked on the CPU:
# tests/test_rnnt_align_host.py::test_reference_viterbi_reproduces_golden_greedy_frames)
GREEDY_IS_BEST = ["v1_rnnt_l2", "v2_rnnt_l2", "v3_rnnt_l2", "v3_e2e_rnnt_l2"]
# the cases where, by the float64 reference alone, the symbol cap does not bind on the width-8 beam's own ids of some utterance
BEAM_BOUND = ["v2_rnnt_l2", "v3_e2e_rnnt_l2"]
POISON = 0x7fffff00     # in the targets' padding: never read

_ENGINES = {}


def _engine(V, L=1, blank_bias=None, H=320, JH=320):
    """An engine with a synthetic RNN-T head (the seeded maker of tests/test_hip_rnnt_beam.py) and its float64 weights."""
    key = (V, L, blank_bias, H, JH)
    if key not in _ENGINES:
        from gigaam_amd import synth
        from gigaam_amd.engine import HipEngine, build_config
        cfg = synth.model_cfg("v3_e2e_rnnt" if V > 34 else "v2_rnnt", n_layers=1)
        cfg["head"]["decoder"]["num_classes"] = cfg["head"]["joint"]["num_classes"] = V
        cfg["head"]["decoder"]["pred_rnn_layers"] = L
        cfg["head"]["decoder"]["pred_hidden"] = cfg["head"]["joint"]["pred_hidden"] = H
        cfg["head"]["joint"]["joint_hidden"] = JH
        sd = synth.make_state_dict(cfg, seed=V + L, rnnt_blank_bias=blank_bias)
        eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), sd, torch.device("cuda:0"))
        _ENGINES[key] = (eng, R.head_from_state_dict(sd, L), cfg)
    return _ENGINES[key]


def _targets(rows, width=None):
    um = max([len(r) for r in rows] + [0]) if width is None else width
    t = torch.full((len(rows), um), POISON, dtype=torch.int32)
    for i, r in enumerate(rows):
        if len(r):
            t[i, :len(r)] = torch.tensor(r, dtype=torch.int32)
    return t, torch.tensor([len(r) for r in rows], dtype=torch.int32)


def _check(h, b, lat, T, U, errs, what):
    """One utterance against the float64 lattice ``lat`` [T, U + 1, 2]: status, scores within the bar, a valid path whose rescore is
    the optimum.  Every figure is recorded before it is asserted."""
    score, _, ok = A.viterbi(lat)
    ll = A.forward_loglik(lat)
    fr = h["tok_frame"][b]
    assert int(h["status"][b]) == int(ok), (what, b)
    assert (fr[U:] == -1).all(), (what, b)
    if not ok:
        assert float(h["score"][b]) == -np.inf and float(h["loglik"][b]) == -np.inf and (fr == -1).all(), (what, b)
        return
    got = fr[:U].tolist()
    assert A.valid_path(got, max(T, 1)) and (T > 0 or U == 0), (what, b, got)
    res = A.rescore(lat, got) if T > 0 else 0.0
    for k, g, want in (("score", float(h["score"][b]), score), ("loglik", float(h["loglik"][b]), ll), ("rescore", res, score),
                       ("self", float(h["score"][b]), res)):
        errs[k] = max(errs.get(k, 0.0), abs(g - want) / max(1.0, abs(want)))
    assert abs(float(h["score"][b]) - score) <= _bar(score), (what, b, float(h["score"][b]), score)
    assert abs(float(h["loglik"][b]) - ll) <= _bar(ll), (what, b, float(h["loglik"][b]), ll)
    assert abs(res - score) <= _bar(score), (what, b, res, score)                        # the returned path is (near-)optimal
    assert abs(float(h["score"][b]) - res) <= _bar(res), (what, b)                       # and `score` is its log-prob
    assert float(h["loglik"][b]) >= float(h["score"][b]) - _bar(score)


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("kind", ["blank", "dense"])
@pytest.mark.parametrize("V,H,JH", [(34, 320, 320), (257, 320, 320), (1025, 320, 320), (257, 256, 512), (34, 512, 512),
                                    (34, 48, 64), (34, 16, 16), (130, 496, 336), (1025, 320, 512)])
def test_op_align_matches_float64_reference(V, H, JH, kind, L):
    """Seeded encp and targets: empty target, U = 1, U > T, T = 1, T = 0 with U = 0 and with U > 0, ragged lengths, poisoned padding.
    pred_hidden = 512 and 496 are the cases above 320: the teacher-forced predictor's eight-rows-per-thread instantiation.  The last
    four are heads of tests/rnnt_cluster_cases.py; pred_hidden = 48, 16 and 496 make the K of the pp GEMM no multiple of 32."""
    eng, head, _ = _engine(V, L, 14.0 if kind == "blank" else None, H, JH)
    rng = np.random.default_rng(V * 11 + L + H + (1 if kind == "dense" else 0))
    Tp = 40
    enc_len = [40, 33, 5, 1, 1, 0, 0, 17, 40, 2]
    ulen = [12, 0, 9, 3, 0, 0, 2, 1, 37, 20]
    rows = [rng.integers(0, V - 1, u).tolist() for u in ulen]
    encp = _encp(rng, len(rows), Tp, JH, 1.0)
    tgt, tlen = _targets(rows)
    out = eng.op_rnnt_align(torch.from_numpy(encp), torch.tensor(enc_len, dtype=torch.int32), tgt, tlen, want_lattice=True)
    h = out.host()
    assert not h["flag"]
    lat_dev = out.lattice.cpu().numpy()
    errs = {}
    for b, y in enumerate(rows):
        T, U = enc_len[b], len(y)
        lat = A.lattice(head, encp[b].astype(np.float64), y, T) if T > 0 else np.zeros((0, U + 1, 2))
        _check(h, b, lat, T, U, errs, (V, kind, L))
        if T > 0:      # stored (lb, le) of sampled nodes (all of them when there are few)
            nodes = [(t, u) for t in range(T) for u in range(U + 1)]
            for i in rng.permutation(len(nodes))[:64]:
                t, u = nodes[i]
                e = abs(float(lat_dev[b, t, u, 0]) - lat[t, u, 0])
                if u < U:
                    e = max(e, abs(float(lat_dev[b, t, u, 1]) - lat[t, u, 1]))
                else:
                    assert lat_dev[b, t, u, 1] == -np.inf
                errs["lattice"] = max(errs.get("lattice", 0.0), e)
                assert e <= TOL_LOGP, (V, kind, L, b, t, u, e)
    report(f"rnnt_align_op_{V}_{H}_{JH}_{kind}_L{L}", **errs)


def _lattice_op(eng, lat, enc_len, rows, V=None, width=None):
    tgt, tlen = _targets(rows, width)
    return eng.op_rnnt_lattice_align(torch.from_numpy(np.ascontiguousarray(lat, dtype=np.float32)),
                                     torch.tensor(enc_len, dtype=torch.int32), tgt, tlen, num_classes=V).host()


def test_lattice_op_takes_the_exact_path_under_the_tie_rule():
    """Dyadic lattice values: every sum is exact in fp32, so the path is the reference's, ties included."""
    eng, _, _ = _engine(34)
    rng = np.random.default_rng(3)
    B, Tp, Um = 24, 12, 9
    lat = rng.choice([0.0, -0.5, -1.0, -2.0], size=(B, Tp, Um + 1, 2))
    enc_len = [int(rng.integers(1, Tp + 1)) for _ in range(B)]
    rows = [rng.integers(0, 33, int(rng.integers(0, Um + 1))).tolist() for _ in range(B)]
    rows[0], enc_len[1] = [1] * Um, Tp
    h = _lattice_op(eng, lat, enc_len, rows, 34, Um)
    tied = 0
    for b, y in enumerate(rows):
        T, U = enc_len[b], len(y)
        sub = lat[b, :T, :U + 1].copy()
        score, fr, ok = A.viterbi(sub)
        assert ok and int(h["status"][b]) == 1
        assert float(h["score"][b]) == score, (b, float(h["score"][b]), score)
        assert h["tok_frame"][b, :U].tolist() == fr and (h["tok_frame"][b, U:] == -1).all(), (b, h["tok_frame"][b].tolist(), fr)
        assert abs(float(h["loglik"][b]) - A.forward_loglik(sub)) <= _bar(score)
        if T * (U + 1) <= 40 and U <= 4:
            tied += len(A.brute_force(sub)[2]) > 1
    assert tied >= 2


def test_lattice_op_beyond_the_lds_backpointer_budget():
    """T' = 4000, U = 1000: 5000 diagonals x 16 words do not fit the kernel's LDS -- the global-scratch path (two columns per thread)."""
    eng, _, _ = _engine(34)
    rng = np.random.default_rng(8)
    Tp, Um = 4000, 1000
    lat = np.log(rng.dirichlet(np.ones(3), size=(2, Tp, Um + 1))[..., :2]).astype(np.float32)
    rows = [rng.integers(0, 33, Um).tolist(), rng.integers(0, 33, 700).tolist()]
    enc_len = [Tp, 3100]
    h = _lattice_op(eng, lat, enc_len, rows, 34, Um)
    errs = {}
    for b, y in enumerate(rows):
        _check(h, b, lat[b, :enc_len[b], :len(y) + 1].astype(np.float64), enc_len[b], len(y), errs, "global bp")
    report("rnnt_align_lattice_global_bp", **errs)


def test_lattice_op_statuses_and_second_stream():
    eng, _, _ = _engine(34)
    rng = np.random.default_rng(5)
    B, Tp, Um = 6, 30, 14
    lat = np.log(rng.dirichlet(np.ones(3), size=(B, Tp, Um + 1))[..., :2]).astype(np.float32)
    lat[2, :, 3, 1] = -np.inf                      # token 3 of utterance 2 can never be emitted: no finite path
    rows = [rng.integers(0, 33, u).tolist() for u in (14, 5, 8, 4, 0, 6)]
    rows[3][2] = 33                                # the blank as a target id
    rows[5][0] = -1
    enc_len = [30, 12, 30, 30, 0, 0]               # utterance 4: T = 0 and U = 0 (status 1); utterance 5: a bad id
    a = _lattice_op(eng, lat, enc_len, rows, 34, Um)
    assert a["status"].tolist() == [1, 1, 0, 0, 1, 0]
    assert float(a["score"][4]) == 0.0 and float(a["loglik"][4]) == 0.0
    for b in (2, 3, 5):
        assert float(a["score"][b]) == -np.inf and float(a["loglik"][b]) == -np.inf and (a["tok_frame"][b] == -1).all()
    tgt, tlen = _targets(rows, Um)
    tlen[1] = Um + 1                               # target_len outside [0, Umax]
    b_ = eng.op_rnnt_lattice_align(torch.from_numpy(lat), torch.tensor(enc_len, dtype=torch.int32), tgt, tlen, num_classes=34).host()
    assert b_["status"].tolist() == [1, 0, 0, 0, 1, 0]
    c = _lattice_op(eng, lat, [30, 12, 30, 30, 0, 9], [r if i != 5 else [] for i, r in enumerate(rows)], 34, Um)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d = _lattice_op(eng, lat, [30, 12, 30, 30, 0, 9], [r if i != 5 else [] for i, r in enumerate(rows)], 34, Um)
    torch.cuda.synchronize()
    for k in ("tok_frame", "status", "score", "loglik"):
        assert c[k].tobytes() == d[k].tobytes(), k
    assert c["status"].tolist() == [1, 1, 0, 0, 1, 1]


def test_op_align_bad_ids_and_T0_statuses():
    eng, head, cfg = _engine(34)
    rng = np.random.default_rng(12)
    encp = _encp(rng, 4, 10, 320, 1.0)
    rows = [[1, 2, 3], [4, 33, 5], [6], []]
    h = eng.op_rnnt_align(torch.from_numpy(encp), torch.tensor([10, 10, 0, 0], dtype=torch.int32), *_targets(rows)).host()
    assert h["status"].tolist() == [1, 0, 0, 1]
    assert (h["tok_frame"][1:] == -1).all() and float(h["score"][3]) == 0.0 and float(h["loglik"][3]) == 0.0


def test_library_rejects_alignment_beyond_the_limits_and_slices_at_the_workspace_limit():
    from gigaam_amd._lib import GigaAMHipError
    eng, head, _ = _engine(34)
    rng = np.random.default_rng(2)
    d = torch.zeros((1, 10, 320), device="cuda:0")
    one = torch.tensor([10], dtype=torch.int32, device="cuda:0")
    o = torch.zeros(4096, dtype=torch.int32, device="cuda:0")
    p = o.data_ptr()
    rc = eng.lib.gam_op_rnnt_align(eng._h, d.data_ptr(), one.data_ptr(), 1, 8193, p, p, 4, p, p, p, p, None, None)
    assert rc != 0 and b"T'=8193" in eng.lib.gam_last_error(eng._h)
    rc = eng.lib.gam_op_rnnt_align(eng._h, d.data_ptr(), one.data_ptr(), 1, 10, p, p, 1025, p, p, p, p, None, None)
    assert rc != 0 and b"Umax=1025" in eng.lib.gam_last_error(eng._h)
    rc = eng.lib.gam_op_rnnt_lattice_align(eng._h, d.data_ptr(), one.data_ptr(), 1, 10, 1026, p, p, 4, p, p, p, p, None)
    assert rc != 0 and b"V=1026" in eng.lib.gam_last_error(eng._h)
    rc = eng.lib.gam_op_rnnt_lattice_align(eng._h, d.data_ptr(), one.data_ptr(), 1, 8193, 34, p, p, 4, p, p, p, p, None)
    assert rc != 0 and b"T'=8193" in eng.lib.gam_last_error(eng._h)
    with pytest.raises(GigaAMHipError, match="encp must be"):
        eng.op_rnnt_align(torch.zeros((1, 10, 64)), one, [[1]])
    # the workspace limit: B = 5, T' = 24, Umax = 7 -> 1536 bytes of lattice per utterance
    B, Tp = 5, 24
    encp = _encp(rng, B, Tp, 320, 1.0)
    rows = [rng.integers(0, 33, u).tolist() for u in (7, 3, 0, 5, 7)]
    enc_len = torch.tensor([24, 20, 9, 24, 1], dtype=torch.int32)
    tgt, tlen = _targets(rows)
    whole = eng.op_rnnt_align(torch.from_numpy(encp), enc_len, tgt, tlen, want_lattice=True)
    hw, lw = whole.host(), whole.lattice.cpu().numpy()
    try:
        eng.set_rnnt_align_workspace(2 * 1536 + 100)          # slices of 2, 2, 1 utterances
        part = eng.op_rnnt_align(torch.from_numpy(encp), enc_len, tgt, tlen, want_lattice=True)
        hp, lp_ = part.host(), part.lattice.cpu().numpy()
        for k in ("tok_frame", "status", "score", "loglik"):
            assert hw[k].tobytes() == hp[k].tobytes(), k
        for b, y in enumerate(rows):
            T, U = int(enc_len[b]), len(y)
            assert lw[b, :T, :U + 1, 0].tobytes() == lp_[b, :T, :U + 1, 0].tobytes()
            assert lw[b, :T, :U, 1].tobytes() == lp_[b, :T, :U, 1].tobytes()
        eng.set_rnnt_align_workspace(1535)
        with pytest.raises(GigaAMHipError, match="1536 bytes, the workspace limit is 1535 bytes"):
            eng.op_rnnt_align(torch.from_numpy(encp), enc_len, tgt, tlen)
    finally:
        eng.set_rnnt_align_workspace(0)
    errs = {}
    for b, y in enumerate(rows):
        _check(hw, b, A.lattice(head, encp[b].astype(np.float64), y, int(enc_len[b])), int(enc_len[b]), len(y), errs, "ws")


@pytest.mark.parametrize("V,L", [(34, 1), (257, 2), (1025, 1)])
def test_op_align_loglik_bounds_the_beam_logp_where_the_cap_cannot_bind(V, L):
    """Blank-dominant synthetic heads through gam_op_rnnt_beam, then gam_op_rnnt_align of the ids the beam returned.  The beam's
    logp sums SOME alignments of those ids under the capped model; with fewer ids than max_symbols no alignment can reach the cap,
    the capped model is the loss's, and log-likelihood >= logp must hold.  Every such utterance is asserted; at least half of the
    batch must qualify, and on them the gap is recorded."""
    from beam_common import run_rnnt_op
    eng, head, _ = _engine(V, L, 14.0)
    rng = np.random.default_rng(V + 5 * L)
    B, Tp, S = 8, 24, 16
    encp = _encp(rng, B, Tp, 320, 1.0)
    enc_len = [24, 24, 17, 9, 24, 1, 24, 13]
    n, gap = 0, 0.0
    for W in (1, 8):
        beam = run_rnnt_op(eng, encp, enc_len, W, S)
        ids = [r[0] for r in beam["rows"]]
        h = eng.op_rnnt_align(torch.from_numpy(encp), torch.tensor(enc_len, dtype=torch.int32), *_targets(ids)).host()
        for b, y in enumerate(ids):
            assert int(h["status"][b]) == 1
            if len(y) < S:
                n += 1
                logp = float(beam["logp"][b])
                gap = max(gap, float(h["loglik"][b]) - logp)
                assert float(h["loglik"][b]) >= logp - _bar(logp), (V, L, W, b, float(h["loglik"][b]), logp)
    report(f"rnnt_align_bounds_beam_{V}_L{L}", asserted=n, largest_gap=gap)
    assert n >= B, n


def test_engine_refuses_heads_beyond_the_alignment_limits():
    """pred_hidden / joint_hidden above 512 or not a multiple of 16 never reach the alignment: the handle is not created."""
    from gigaam_amd import synth
    from gigaam_amd._lib import GigaAMHipError
    from gigaam_amd.engine import HipEngine, build_config
    for H, JH in ((528, 320), (320, 528), (328, 320), (320, 328)):
        cfg = synth.model_cfg("v2_rnnt", n_layers=1)
        cfg["head"]["decoder"]["pred_hidden"] = cfg["head"]["joint"]["pred_hidden"] = H
        cfg["head"]["joint"]["joint_hidden"] = JH
        with pytest.raises(GigaAMHipError, match="RNN-T head shape unsupported"):
            HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), {}, torch.device("cuda:0"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", RNNT_CASES)
def test_encoded_align_on_golden_cases_matches_reference(name, mode):
    """Aligning the golden greedy ids from the golden encoder output: scores against the float64 reference, loglik >= score, and
    the greedy frames where the reference's best path is the greedy one.  Then the cross-check with the beam stack: the width-8
    beam's OWN ids are aligned too, and loglik >= the beam's logp is asserted for both sets of ids wherever the bound exists.
    logp is a lower bound of the decoders' capped model P_S (after max_symbols tokens the frame advances without a joint, with
    probability 1, where the loss's lattice pays log P(blank)), so it bounds the likelihood only where the cap does not bind; on
    the emission-heavy goldens logp lies far ABOVE the likelihood (v1_rnnt_l2, utterance 1: logp -2.94, log-likelihood -23.02
    from the kernel and from the float64 reference alike).  The reference decides per utterance: the bound is asserted where
    rnnt_align_ref.capped_loglik does not exceed the reference's log-likelihood.  With the float64 reference alone that holds
    for the beam's ids on v2_rnnt_l2 (utterances 1, 2) and v3_e2e_rnnt_l2 (0, 1): there it must have been asserted at least once."""
    from gigaam_amd.engine import HipEngine, build_config
    ck, _, _, gold = load_case(name)
    cfg = ck["cfg"]
    eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), ck["state_dict"], torch.device("cuda:0"))
    eng.set_gemm_mode(mode)
    L = cfg["head"]["decoder"]["pred_rnn_layers"]
    S = cfg["decoding"].get("max_symbols_per_step", 10)
    head = R.head_from_state_dict(ck["state_dict"], L)
    rows = split_ragged(gold["ids"], gold["frames"], gold["counts"].tolist())
    enc, elen = torch.from_numpy(gold["encoded"]), torch.from_numpy(gold["enc_len"])
    h = eng.rnnt_align(enc, elen, *_targets([ids for ids, _ in rows])).host()
    assert not h["flag"]
    beam = eng.rnnt_beam(enc, elen, 8, S).host()
    errs, same, bounded = {}, 0, 0
    for b, (ids, frames) in enumerate(rows):
        T = int(gold["enc_len"][b])
        lat = A.lattice(head, R.encoder_projection(head, gold["encoded"][b]), ids, T)
        _check(h, b, lat, T, len(ids), errs, (name, mode))
        if A.viterbi(lat)[1] == frames:
            assert h["tok_frame"][b, :len(ids)].tolist() == frames, (name, mode, b)
            same += 1
        ll = A.forward_loglik(lat)
        if beam["rows"][b][0] == ids and A.capped_loglik(lat, S) <= ll + _bar(ll):
            bounded += 1
            assert float(h["loglik"][b]) >= float(beam["logp"][b]) - _bar(float(beam["logp"][b])), (b, float(h["loglik"][b]), float(beam["logp"][b]))
    bids = [r[0] for r in beam["rows"]]
    hb = eng.rnnt_align(enc, elen, *_targets(bids)).host()
    for b, ids in enumerate(bids):
        T = int(gold["enc_len"][b])
        lat = A.lattice(head, R.encoder_projection(head, gold["encoded"][b]), ids, T)
        _check(hb, b, lat, T, len(ids), errs, (name, mode, "beam ids"))
        ll, logp = A.forward_loglik(lat), float(beam["logp"][b])
        if A.capped_loglik(lat, S) <= ll + _bar(ll):
            bounded += 1
            errs["beam_gap"] = max(errs.get("beam_gap", 0.0), float(hb["loglik"][b]) - logp)
            assert float(hb["loglik"][b]) >= logp - _bar(logp), (name, mode, b, float(hb["loglik"][b]), logp)
    report(f"rnnt_align_golden_{name}_{mode}", greedy_paths=same, beam_bounded=bounded, **errs)
    assert bounded >= 1 or name not in BEAM_BOUND, name
    assert same >= 1 or name not in GREEDY_IS_BEST, name


def test_model_rnnt_align_of_its_own_transcript(tmp_path):
    model, _ = small_rnnt_model()
    path = _wav_file(tmp_path, 6, 5)
    res = model.transcribe(path, word_timestamps=True)
    tok = model.decoding.tokenizer
    ids = tok.encode(res.text)
    al = model.rnnt_align(path, res.text)
    assert al.feasible and al.text == res.text and al.token_ids == ids and len(al.token_frames) == len(ids)
    assert A.valid_path(al.token_frames, 10 ** 6) and np.isfinite(al.score) and al.log_likelihood >= al.score - 1e-3 * max(1.0, abs(al.score))
    assert len(al.words) == len(res.words) and [w.text for w in al.words] == [w.text for w in res.words]
    by_ids = model.rnnt_align(path, ids)
    assert by_ids == al
    with pytest.raises(TypeError, match="forced alignment needs a CTC head"):
        model.align(path, res.text)
    # the same whatever set_decoding selected
    model.set_decoding(beam_size=4)
    try:
        assert model.rnnt_align(path, res.text) == al
    finally:
        model.set_decoding()
    # a batch: ragged clips, one empty text
    from gigaam_amd import synth
    wav, lens = synth.synth_audio(3, 4.0, seed=9, lengths=[64000, 30000, 64000])
    texts = [t for t, _ in model.transcribe_batch(wav, lens)]
    out = model.rnnt_align_batch(wav, lens, [texts[0], "", texts[2]])
    assert [o.feasible for o in out] == [True, True, True] and out[1].token_ids == [] and out[1].words == []
    assert out[1].log_likelihood == pytest.approx(out[1].score, abs=1e-4) and out[0].text == texts[0]


def test_model_rnnt_align_batch_with_sentencepiece_ids_and_ctc_type_error():
    import gigaam_amd
    from gigaam_amd import synth
    ck = synth.make_checkpoint("v3_e2e_rnnt", seed=2, n_layers=2, rnnt_blank_bias=12.0)
    ck["cfg"]["decoding"]["model_path"] = os.path.join(ROOT, "tests", "golden", "spm256.model")
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    wav, lens = synth.synth_audio(2, 3.0, seed=4, lengths=[48000, 31000])
    rng = np.random.default_rng(0)
    ids = [rng.integers(0, 256, 6).tolist(), rng.integers(0, 256, 2).tolist()]      # (spm256.model holds 256 pieces)
    out = model.rnnt_align_batch(wav, lens, ids)
    for o, y in zip(out, ids):
        assert o.feasible and o.token_ids == y and len(o.token_frames) == len(y) and A.valid_path(o.token_frames, 10 ** 6)
        assert np.isfinite(o.score) and o.log_likelihood >= o.score - 1e-3 * max(1.0, abs(o.score))
    ctc = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=0, n_layers=2), "cuda:0")
    with pytest.raises(TypeError, match="transducer alignment needs an RNN-T head"):
        ctc.rnnt_align_batch(wav, lens, ["а", "б"])
