"""GPU: what an 8-GPU node (or a multi-threaded host) hits first -- several library handles alive in one process and
decoding concurrently, checkpoints stored in half precision (VERDICT r3 "next" #6)."""
import threading

import pytest
import torch

from common import TOL_ENC, load_case, ragged_from_device, report, split_ragged, valid_mask
from oracle import gigaam_oracle as O

pytestmark = pytest.mark.gpu


def _engine(ck):
    from gigaam_amd.engine import HipEngine, build_config
    cfg = ck["cfg"]
    return HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg.get("head")), ck["state_dict"], torch.device("cuda:0"))


def test_two_handles_decode_concurrently_from_two_threads():
    """Three handles on cuda:0 (one CTC model, two RNN-T models), three host threads, each launching the whole path on its
    own stream 12 times: the per-process statics of the library (kernel attribute bookkeeping, tuning knobs read on first
    use) are hit from several threads at once, the cooperative cluster launches of the two RNN-T handles contend for the
    same CUs (the repair pass covers a cluster that was not co-resident), and every iteration of every thread must give
    the reference's ids and frames."""
    cases = ["v2_ctc_l2", "v2_rnnt_l2", "v3_e2e_rnnt_l2"]
    jobs = []
    for name in cases:
        ck, wav, wlen, gold = load_case(name)
        ref = split_ragged(gold["ids"], gold["frames"], gold["counts"].tolist())
        jobs.append((name, ck, wav.cuda(), wlen.cuda(), ref))
    start = threading.Barrier(len(jobs))
    errors, done = [], []

    def run(name, ck, wav, wlen, ref):
        try:
            torch.cuda.set_device(0)
            stream = torch.cuda.Stream()
            start.wait(timeout=120)                 # all threads create their handles and first-use statics together
            eng = _engine(ck)
            ms = ck["cfg"]["decoding"].get("max_symbols_per_step", 10)
            with torch.cuda.stream(stream):
                for it in range(12):
                    enc, elen = eng.encode(*eng.frontend(wav, wlen))
                    out = eng.rnnt_greedy(enc, elen, ms) if "rnnt" in name else eng.ctc_greedy(enc, elen)
                    got = ragged_from_device(*out)
                    if got != ref:
                        errors.append((name, it, "ids/frames differ from the reference"))
                        return
            done.append(name)
        except Exception as e:  # noqa: BLE001
            errors.append((name, -1, repr(e)))

    threads = [threading.Thread(target=run, args=j) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not errors, errors
    assert sorted(done) == sorted(cases)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("case", ["v2_ctc_l2", "v3_e2e_rnnt_l2"])
def test_half_precision_state_dict(case, dtype):
    """A checkpoint saved after the reference's ``load_model(fp16_encoder=True)`` (or a bf16 fine-tune) holds fp16 / bf16
    tensors: gam_set_weight widens them (gam_api.hip, GAM_DTYPE_F16 / _BF16).  Widening is exact, so the engine fed the
    narrow tensors must agree with the oracle run on the SAME values widened on the host -- at the usual fp32 bars, not
    at half-precision ones (ids and frames exact)."""
    ck, wav, wlen, _ = load_case(case)
    sd_narrow = {k: (v.to(dtype) if torch.is_floating_point(v) else v) for k, v in ck["state_dict"].items()}
    assert any(v.dtype == dtype for v in sd_narrow.values())
    ck_wide = dict(ck, state_dict={k: (v.to(torch.float32) if torch.is_floating_point(v) else v) for k, v in sd_narrow.items()})
    with torch.no_grad():
        dec_o, enc_o, elen_o = O.transcribe_ids(ck_wide, wav, wlen)
    eng = _engine(dict(ck, state_dict=sd_narrow))
    enc, elen = eng.encode(*eng.frontend(wav, wlen))
    assert elen.cpu().tolist() == elen_o.tolist()
    vm = valid_mask(enc_o.shape[2], elen_o)[:, None, :]
    err = float(((enc.cpu() - enc_o) * vm).abs().max())
    report("half_precision_state_dict", case=case, dtype=str(dtype), err=err, tol=TOL_ENC)
    assert err < TOL_ENC, err
    # decoding: the head weights are narrow too.  Decoder alone on the ORACLE's encoder output (arithmetic differences
    # ~1e-5: no near-tie can flip), and the whole path whenever the oracle's own top-1 / top-2 margins leave room for the
    # encoder's 2e-4 (the case seeds were searched for fp32 weights; rounding the weights moves the margins)
    ms = ck["cfg"]["decoding"].get("max_symbols_per_step", 10)
    want = [(list(i), list(f)) for i, f in dec_o]
    dec = (lambda e, l: eng.rnnt_greedy(e, l, ms)) if "rnnt" in case else eng.ctc_greedy
    assert ragged_from_device(*dec(enc_o, elen_o.to(torch.int32))) == want
    if "ctc" in case:
        with torch.no_grad():
            lp = O.ctc_log_probs(ck_wide["state_dict"], enc_o)
        top2 = lp.topk(2, dim=-1).values
        margin = float(((top2[..., 0] - top2[..., 1]) + (~valid_mask(lp.shape[1], elen_o)) * 1e9).min())
        report("half_precision_state_dict_margin", case=case, dtype=str(dtype), margin=margin)
        if margin > 2e-3:
            assert ragged_from_device(*dec(enc, elen)) == want


@pytest.mark.parametrize("case", ["v2_rnnt_l2", "v2_rnnt_l2_lstm2", "v3_e2e_rnnt_l2"])
def test_rnnt_per_step_entry_points(case):
    """The RNN-T head taken apart (r04: gam_rnnt_predict / gam_rnnt_joint behind ``model.head.decoder.predict`` and
    ``model.head.joint.joint``, the reference's gigaam/decoder.py:41-47,85-102) against the oracle's per-sample restatement:
    predictor output and state over a few steps (zero input first, then labels; 1 and 2 LSTM layers), joint log-probs over a
    [B, T, U] grid -- and a greedy decode DRIVEN THROUGH these entry points reproduces the reference's ids and frames."""
    import gigaam_amd
    ck, wav, wlen, gold = load_case(case)
    sd, cfg = ck["state_dict"], ck["cfg"]
    nl = cfg["head"]["decoder"]["pred_rnn_layers"]
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0", fp16_encoder=False)
    dec, jnt = model.head.decoder, model.head.joint
    # --- predictor: x = None with no state, then two label steps for B = 3 samples
    labels = [torch.tensor([[1], [5], [0]]), torch.tensor([[7], [7], [2]])]
    g, st = dec.predict(None, None, batch_size=3)
    want = [O.rnnt_predict(sd, None, None, nl) for _ in range(3)]
    worst = 0.0

    def cmp(g_, st_, want_):
        w = 0.0
        for b, (gw, (hw, cw)) in enumerate(want_):
            w = max(w, float((g_[b, -1].cpu() - gw).abs().max()), float((st_[0][:, b].cpu() - hw).abs().max()),
                    float((st_[1][:, b].cpu() - cw).abs().max()))
        return w
    with torch.no_grad():
        worst = max(worst, cmp(g, st, want))
        for lab in labels:
            g, st2 = dec.predict(lab.cuda(), st)
            want = [O.rnnt_predict(sd, int(lab[b, 0]), (want[b][1][0], want[b][1][1]), nl) for b in range(3)]
            worst = max(worst, cmp(g, st2, want))
            st = st2
    assert g.shape == (3, 1, cfg["head"]["decoder"]["pred_hidden"])
    # --- joint over a grid
    enc_ref = torch.from_numpy(gold["encoded"])[:2, :, :5].transpose(1, 2).contiguous()      # [2, 5, D]
    gs = torch.stack([want[0][0], want[1][0], want[2][0]])[:2].unsqueeze(1).repeat(1, 3, 1) * torch.tensor([1.0, 0.5, -1.0])[None, :, None]
    lp = jnt.joint(enc_ref.cuda(), gs.cuda()).cpu()
    assert lp.shape == (2, 5, 3, cfg["head"]["joint"]["num_classes"])
    jw = 0.0
    with torch.no_grad():
        for b in range(2):
            for t in range(5):
                for u in range(3):
                    jw = max(jw, float((lp[b, t, u] - O.rnnt_joint(sd, enc_ref[b, t], gs[b, u])).abs().max()))
    report("rnnt_per_step", case=case, predictor_err=worst, joint_err=jw, tol=1e-4)
    assert worst < 1e-4 and jw < 1e-3, (worst, jw)
    # --- the reference's greedy loop (decoding.py:162-205), one sample, driven through the entry points
    enc1 = torch.from_numpy(gold["encoded"])[:1]
    n = int(gold["enc_len"][0])
    blank = cfg["head"]["decoder"]["num_classes"] - 1
    ms = cfg["decoding"]["max_symbols_per_step"]
    ids, frames, label, state = [], [], None, None
    x = enc1.transpose(1, 2).cuda()
    for t in range(n):
        for _ in range(ms):
            g1, new_state = dec.predict(None if label is None else torch.tensor([[label]]).cuda(), state, batch_size=1)
            k = int(jnt.joint(x[:, t:t + 1], g1)[0, 0, 0].argmax())
            if k == blank:
                break
            ids.append(k); frames.append(t)
            label, state = k, new_state
    c0 = int(gold["counts"][0])
    assert ids == gold["ids"][:c0].tolist() and frames == gold["frames"][:c0].tolist()


def test_feeder_pipelined_without_host_syncs_and_copy_option():
    """the feeder's device slots are REUSED (two slots, views yielded).  (a) The product's usage -- every reader of
    batch n enqueued on the current stream before batch n + 1 is requested, results looked at one batch late, no
    torch.cuda.synchronize() anywhere -- over 6 ragged batches must see exactly ``collate``'s bytes; (b) ``copy=True`` lets a
    consumer keep every batch (``list(feeder)``)."""
    from gigaam_amd.feeder import BatchFeeder, batches, collate
    g = torch.Generator().manual_seed(5)
    segs = [torch.randn(int(n), generator=g) for n in torch.randint(20000, 400000, (17,), generator=g)]
    dev = torch.device("cuda:0")
    want = [collate(c) for c in batches(segs, 3)]
    assert len(want) == 6
    # (a) un-synchronised pipeline: per batch a few device ops whose (fresh) results are kept; the views themselves are not
    kept, pending = [], None
    big = torch.empty((64, 1 << 20), device=dev)
    for wav, ln in BatchFeeder(segs, 3, dev):
        big.normal_()                                       # keep the stream busy so the side-stream copies really run ahead
        res = (wav.double().sum(dim=1), wav[:, ::977].clone(), wav[:, -1].clone(), ln.clone())
        if pending is not None:
            kept.append(tuple(t.cpu() for t in pending))    # collected one batch late, like model.transcribe_longform
        pending = res
    kept.append(tuple(t.cpu() for t in pending))
    assert len(kept) == len(want)
    for (sm, strided, last, ln), (w, l) in zip(kept, want):
        assert torch.equal(ln, l) and torch.equal(strided, w[:, ::977]) and torch.equal(last, w[:, -1])
        assert torch.allclose(sm, w.double().sum(dim=1), rtol=0, atol=1e-9)
    # (b) copy=True: every batch survives being kept
    held = list(BatchFeeder(segs, 3, dev, copy=True))
    torch.cuda.synchronize()
    for (wav, ln), (w, l) in zip(held, want):
        assert torch.equal(wav.cpu(), w) and torch.equal(ln.cpu(), l)


@pytest.mark.parametrize("model_name,bias", [("v2_rnnt", 13.5), ("v3_e2e_rnnt", 14.0)])
def test_rnnt_decode_overlapped_with_the_next_encoder(model_name, bias):
    """r05: the RNN-T decode of batch n on the engine's side stream (small clusters) BESIDE the frontend + encoder of batch
    n + 1 on the launch stream, same handle -- six ragged batches launched back to back with no host sync in between, collected
    one batch late -- must give exactly the ids + frames of the serial path (decode in front of the next encoder, full-size
    clusters), through ``model.launch_batch(overlap=True)`` / ``collect_batch`` and through the engine directly."""
    import gigaam_amd
    from gigaam_amd import synth
    from gigaam_amd.engine import HipEngine
    ck = synth.make_checkpoint(model_name, seed=1, n_layers=2, rnnt_blank_bias=bias)
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    eng = model.encoder.engine
    ms = ck["cfg"]["decoding"].get("max_symbols_per_step", 10)
    batches = []
    for k in range(6):
        b = [9, 32, 5, 17, 33, 8][k]
        lens = [int(16000 * (1.0 + 0.37 * ((3 * i + k) % 11))) for i in range(b)]
        batches.append(synth.synth_audio(b, max(lens) / 16000.0, seed=300 + k, lengths=lens))
    def serial_with(cluster_of):
        out = []
        for wav, wlen in batches:
            enc, elen = eng.encode(*eng.frontend(wav, wlen))
            eng.set_rnnt_cluster(cluster_of(wav.shape[0]))
            out.append(HipEngine.collect(eng.rnnt_greedy(enc, elen, ms))[0])
        eng.set_rnnt_cluster(-1)
        return out
    full = serial_with(lambda b: -1)
    assert sum(len(i) for rows in full for i, _ in rows) > 50
    for side_cus in (32, 64, 128):
        # the serial path at the SAME cluster size: the overlapped decode must reproduce it bit for bit (same kernel, same
        # summation order; different cluster sizes differ by ~1e-6 in a logit, which a near-tie of this random head may show)
        serial = serial_with(lambda b: HipEngine.side_cluster(b, side_cus))
        pend, got = None, []
        for k, (wav, wlen) in enumerate(batches):
            enc, elen = eng.encode(*eng.frontend(wav, wlen))
            dec = eng.rnnt_greedy(enc, elen, ms, overlap=True, side_cus=side_cus)
            if pend is not None:
                got.append(HipEngine.collect(pend)[0])
            pend = dec
        got.append(HipEngine.collect(pend)[0])
        assert got == serial, side_cus
        n_same = sum(a == b for ra, rb in zip(serial, full) for a, b in zip(ra, rb))
        assert n_same >= 0.9 * sum(len(r) for r in full), (side_cus, n_same)     # and all but near-tie utterances equal the full-size clusters'
    # the package seam
    serial = serial_with(lambda b: HipEngine.side_cluster(b, 96 if eng.cfg.num_classes <= 64 else 160))
    tok = model.decoding.tokenizer
    texts_serial = [[(tok.decode(i), None) for i, _ in rows] for rows in serial]
    pend, texts = None, []
    for k, (wav, wlen) in enumerate(batches):
        h = model.launch_batch(wav, wlen, overlap=True)
        if pend is not None:
            texts.append(model.collect_batch(pend))
        pend = h
    texts.append(model.collect_batch(pend))
    assert texts == texts_serial


@pytest.mark.parametrize("exclusive", [1, 0])
def test_rnnt_decode_is_not_perturbed_by_another_streams_gemm(exclusive):
    """r05 / r06 regression (profiles/r05_overlap_investigation.txt, profiles/r06_INDEX.txt): an RNN-T cluster decode on a side stream while the
    launch stream runs the small-tile GEMM came out with a perturbed predictor state in 1-30 % of the launches.  r06 found the mechanism: hipcc
    had packed pairs of gate-row FMA chains into v_pk_fma_f32 with op_sel:[0,1,0], whose low result is wrong in lanes 48..63 whenever another
    wave on the SIMD issues MFMAs (tools/pkfma_rule.hip).  The library holds no such instruction any more (gigaam_amd/build.py), so the decode
    must be bit-identical to the one that had the GPU to itself BOTH with the r05 protection (GAM_RNNT_EXCLUSIVE=1: workgroups claim their
    CU's whole LDS) and without it (exclusive = 0, the default: decode workgroups share CUs with the GEMM's).  With the r05 library the
    exclusive = 0 leg fails with probability > 0.95 (cluster size 1: 34 of 3000 decodes differed)."""
    import os
    from gigaam_amd import synth
    from gigaam_amd.engine import HipEngine, build_config
    ck = synth.make_checkpoint("v2_rnnt", seed=1, n_layers=2, rnnt_blank_bias=13.5)
    cfg = ck["cfg"]
    os.environ["GAM_RNNT_EXCLUSIVE"] = str(exclusive)      # (read by gam_create)
    try:
        eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), ck["state_dict"], torch.device("cuda:0"))
    finally:
        del os.environ["GAM_RNNT_EXCLUSIVE"]
    lens = [int(16000 * (1.0 + 0.37 * ((3 * i + 1) % 11))) for i in range(32)]
    wav, wlen = synth.synth_audio(32, max(lens) / 16000.0, seed=301, lengths=lens)
    enc, elen = eng.encode(*eng.frontend(wav, wlen))
    xa = torch.randn(640, 768, device="cuda")
    wa = torch.randn(768, 768, device="cuda") * 0.03
    ref_gemm = eng.op_gemm(xa, wa).clone()
    for cluster, reps in ((1, 300 if exclusive == 0 else 50), (2, 100 if exclusive == 0 else 50), (4, 50)):
        eng.set_rnnt_cluster(cluster)
        alone = HipEngine.collect(eng.rnnt_greedy(enc, elen, 10))[0]
        eng.set_rnnt_cluster(-1)
        assert sum(len(i) for i, _ in alone) > 300
        bad = 0
        os.environ["GAM_DEBUG_SIDE_CLUSTER"] = str(cluster)
        try:
            for _ in range(reps):
                dec = eng.rnnt_greedy(enc, elen, 10, overlap=True)
                for _ in range(30):
                    out = eng.op_gemm(xa, wa)
                bad += HipEngine.collect(dec)[0] != alone
                assert torch.equal(out, ref_gemm)          # (and the GEMM is not perturbed by the decode either)
        finally:
            del os.environ["GAM_DEBUG_SIDE_CLUSTER"]
        assert bad == 0, (exclusive, cluster, bad)


def test_decodes_on_different_streams_are_ordered_by_the_library():
    """the decode class owns ONE set of scratch per handle (tok / encp / rnnt_x ...).  An overlapped decode (side stream) followed
    at once by a serial decode of ANOTHER batch on the launch stream -- what transcribe_longform / run_sharded do for their last batch -- used to
    have nothing ordering the second behind the first.  gam_api.hip's DecodeScope now makes every decode-class call wait for the previous one's
    completion event when the streams differ: both decodes must equal their own serial results, also for the CTC head and the joint entry point."""
    from gigaam_amd import synth
    from gigaam_amd.engine import HipEngine, build_config
    ck = synth.make_checkpoint("v2_rnnt", seed=1, n_layers=2, rnnt_blank_bias=13.5)
    cfg = ck["cfg"]
    eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), ck["state_dict"], torch.device("cuda:0"))
    lens = [int(16000 * (1.0 + 0.37 * ((3 * i + 1) % 11))) for i in range(32)]
    wav, wlen = synth.synth_audio(32, max(lens) / 16000.0, seed=301, lengths=lens)
    enc_big, elen_big = eng.encode(*eng.frontend(wav, wlen))
    enc_big, elen_big = enc_big.clone(), elen_big.clone()
    wav1, wlen1 = synth.synth_audio(1, 1.5, seed=77, lengths=[24000])
    enc_1, elen_1 = eng.encode(*eng.frontend(wav1, wlen1))
    enc_1, elen_1 = enc_1.clone(), elen_1.clone()
    eng.set_rnnt_cluster(HipEngine.side_cluster(32, 96))
    want_big = HipEngine.collect(eng.rnnt_greedy(enc_big, elen_big, 10))[0]
    eng.set_rnnt_cluster(-1)
    want_1 = HipEngine.collect(eng.rnnt_greedy(enc_1, elen_1, 10))[0]
    g, st = eng.rnnt_predict(None, None, 1)
    want_joint = eng.rnnt_joint(enc_1.transpose(1, 2).contiguous()[:, :4], g[:, None, :]).clone()
    torch.cuda.synchronize()
    eng.set_rnnt_cluster(3)      # a caller's own setting survives overlapped decodes (it used to be reset to the environment's value)
    HipEngine.collect(eng.rnnt_greedy(enc_1, elen_1, 10, overlap=True))
    assert eng.lib.gam_get_rnnt_cluster(eng._h) == 3
    eng.set_rnnt_cluster(-1)
    for rep in range(40):
        big = eng.rnnt_greedy(enc_big, elen_big, 10, overlap=True, side_cus=96)     # slow small clusters on the side stream ...
        if rep % 2 == 0:
            one = eng.rnnt_greedy(enc_1, elen_1, 10)                                 # ... and at once a B = 1 decode on the launch stream
            assert HipEngine.collect(one)[0] == want_1, rep
        else:
            got_joint = eng.rnnt_joint(enc_1.transpose(1, 2).contiguous()[:, :4], g[:, None, :])   # (rewrites encp on the launch stream)
            torch.cuda.synchronize()
            assert torch.equal(got_joint, want_joint), rep
        assert HipEngine.collect(big)[0] == want_big, rep




def test_auxiliary_streams_never_share_the_launch_streams_hardware_queue():
    """HIP maps the streams of one priority level onto four hardware queues in creation order, and two streams on one queue serialise: one
    normal-priority stream in four shares the NULL stream's queue (tools/queue_probe.py, profiles/r06_queue_probe.txt) -- an "overlapped" decode
    on such a stream silently runs behind the encoder.  The engine's decode / collect / copy streams are high-priority streams taken together:
    whatever the application created before, a spin kernel on each of them runs BESIDE one on the launch stream and beside each other."""
    import time
    dev = torch.device("cuda:0")
    mine = [torch.cuda.Stream(dev) for _ in range(5)]          # an application with streams of its own
    for s in mine:
        with torch.cuda.stream(s):
            torch.zeros(8, device=dev).add_(1)
    from gigaam_amd.engine import HipEngine
    aux = HipEngine.aux_streams(dev)
    assert len(aux) == 3 and len({s.cuda_stream for s in aux}) == 3 and all(s.priority == -1 for s in aux)
    cyc = 10_000_000

    def run(streams):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in streams:
            with torch.cuda.stream(s):
                torch.cuda._sleep(cyc)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for launch in [torch.cuda.default_stream(dev)] + mine:
        run([launch]); run([launch, *aux])
        one = min(run([launch]) for _ in range(3))
        allfour = min(run([launch, *aux]) for _ in range(3))
        report("aux_streams_beside_launch_stream", ratio=allfour / one)
        assert allfour < 1.5 * one, (allfour, one)      # serialised: 2x .. 4x
