"""GPU: the HIP path (through the C ABI) against the CPU oracle and the reference's
golden vectors, on the same seeded inputs.  Tolerances are in tests/common.py."""
import numpy as np
import pytest
import torch

from common import make_engine as _make_engine
from common import (CASES, TOL_ENC, TOL_FEAT, TOL_FEAT_WEAK, TOL_LOGP, frontend_fixture, golden_trace, load_case, logmel_err,
                    oracle_features, ragged_from_device, report, tol_pre, split_ragged, valid_mask)
from oracle import gigaam_oracle as O

pytestmark = pytest.mark.gpu

SUPPORTED = list(CASES)


# Every arithmetic mode of the dense contractions must hold the same bars: "f16x3" = the product's default (three-term split on the
# LDS-DMA kernels of gam_gemm_sp.h; the v3 conv1d stem and v1's rel-pos projection included), "f32" = exact-fp32 MFMA.
MODES = ["f16x3", "f32"]


def _engine(ck, mode="f16x3"):
    return _make_engine(ck["cfg"], ck["state_dict"], mode)


@pytest.mark.parametrize("mode", MODES)
def test_gemm_kernel_shapes_and_epilogues(mode):
    from gigaam_amd import synth
    eng = _make_engine(synth.model_cfg("v2_ctc"), {}, mode, head=False)
    g = torch.Generator().manual_seed(0)
    # asymmetric operands, ragged M/N edges, all activations (transposes / layout slips cannot hide)
    # N % 4 != 0 ((257, 34, 768), (1, 1, 32)): the exact-fp32 kernel in every mode (the LDS-DMA epilogue moves 4-column pieces)
    for (m, n, k, act) in [(128, 128, 32, 0), (300, 200, 64, 0), (1000, 768, 768, 1), (257, 34, 768, 0), (515, 1536, 96, 2), (1, 1, 32, 0),
                           (16064, 768, 64, 0), (16064, 3072, 64, 1), (33000, 1536, 32, 2),
                           # steady-state k-loop of the large-batch kernel (192x256 / 256x256 tiles, LDS-DMA)
                           (16064, 768, 768, 0), (16064, 3072, 768, 1), (8000, 768, 3072, 0), (4016, 1536, 768, 2)]:
        a = torch.randn(m, k, generator=g)
        w = torch.randn(n, k, generator=g) / k ** 0.5
        b = torch.randn(n, generator=g)
        ref = a.double() @ w.double().t() + b.double()
        ref = ref * torch.sigmoid(ref) if act == 1 else (torch.relu(ref) if act == 2 else ref)
        out = eng.op_gemm(a, w, b, act).cpu().double()
        assert float((out - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max())), (m, n, k, act)
    # race screen of the DMA / barrier pipeline: reruns of a deep-k large GEMM are bit-identical
    a = torch.randn(16064, 1536, generator=g).cuda()
    w = (torch.randn(768, 1536, generator=g) / 1536 ** 0.5).cuda()
    first = eng.op_gemm(a, w)
    for _ in range(6):
        assert torch.equal(eng.op_gemm(a, w), first)
    eye = torch.eye(64)
    w = torch.arange(96 * 64, dtype=torch.float32).reshape(96, 64) / 100.0
    got = eng.op_gemm(eye, w).cpu()
    if mode == "f32":
        assert torch.equal(got, w.t().contiguous())  # A = I, asymmetric W: exact (fmaf chain)
    else:
        assert float((got - w.t()).abs().max()) < 1e-5 * float(w.max())  # hi+lo keeps 22 bits


@pytest.mark.parametrize("mode", MODES)
def test_attention_kernel(mode):
    """Fused attention kernel alone against an fp64 softmax(QK^T/sqrt(dk))V with key masking."""
    from gigaam_amd import synth
    eng = _make_engine(synth.model_cfg("v2_ctc"), {}, mode, head=False)
    g = torch.Generator().manual_seed(3)
    for (b, t, h, lens) in [(1, 16, 1, None), (2, 70, 2, [70, 33]), (3, 203, 16, [203, 150, 1])]:
        q, k, v = (torch.randn(b, t, h * 48, generator=g) * s for s in (2.0, 2.0, 1.0))
        lt = None if lens is None else torch.tensor(lens)
        got = eng.op_attention(q, k, v, lt).cpu().double()
        qh, kh, vh = (x.double().view(b, t, h, 48).transpose(1, 2) for x in (q, k, v))
        sc = qh @ kh.transpose(-1, -2) / 48 ** 0.5
        if lt is not None:
            sc = sc.masked_fill((torch.arange(t)[None, :] >= lt[:, None])[:, None, None, :], float("-inf"))
        ref = (torch.softmax(sc, -1) @ vh).transpose(1, 2).reshape(b, t, h * 48)
        err = float((got - ref).abs().max())
        assert err < 2e-5, (mode, b, t, h, err)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", SUPPORTED)
def test_frontend_matches_oracle(case, mode):
    ck, wav, wlen, gold = load_case(case)
    eng = _engine(ck, mode)
    feat_o, flen_o = oracle_features(ck, wav, wlen)
    feat, flen = eng.frontend(wav, wlen)
    assert feat.shape == feat_o.shape and flen.dtype == torch.int64 and flen.cpu().tolist() == flen_o.tolist()
    fm = valid_mask(feat_o.shape[2], flen_o)[:, None, :]
    e_strong, e_weak = logmel_err(feat.cpu(), feat_o, fm[:, 0, :])
    assert e_strong < TOL_FEAT and e_weak < TOL_FEAT_WEAK, (e_strong, e_weak)
    report("frontend_vs_oracle", case=case, mode=mode, strong=e_strong, weak=e_weak, tol=TOL_FEAT, tol_weak=TOL_FEAT_WEAK)
    fx = frontend_fixture(case)   # torchaudio's own output, when someone has generated it (a1 is unpinned otherwise)
    if fx is not None:
        es, ew = logmel_err(feat.cpu(), torch.from_numpy(fx["feat"]), fm[:, 0, :])
        assert es < TOL_FEAT and ew < TOL_FEAT_WEAK, ("torchaudio fixture", es, ew)
    np.testing.assert_allclose(feat.cpu()[:, ::7, ::13].numpy(), gold["feat_probe"], atol=TOL_FEAT_WEAK)
    probe_o = feat_o[:, ::7, ::13]
    keep = probe_o >= feat_o.max(dim=1, keepdim=True).values[:, :, ::13] - 60.0 * 0.2302585
    assert float(((feat.cpu()[:, ::7, ::13] - torch.from_numpy(gold["feat_probe"])).abs() * keep).max()) < TOL_FEAT


@pytest.mark.parametrize("case,mode", [(c, m) for c in SUPPORTED for m in MODES])
def test_encoder_matches_reference_golden(case, mode):
    ck, wav, wlen, gold = load_case(case)
    eng = _engine(ck, mode)
    feat_o, flen_o = oracle_features(ck, wav, wlen)
    enc, elen = eng.encode(feat_o, flen_o)
    assert elen.dtype == torch.int32 and elen.cpu().tolist() == gold["enc_len"].tolist()
    assert tuple(enc.shape) == gold["encoded"].shape
    vm = valid_mask(enc.shape[2], gold["enc_len"])
    assert bool(torch.isfinite(enc).all())  # padded rows are don't-care but must stay finite
    e_enc = float(((enc.cpu() - torch.from_numpy(gold["encoded"])) * vm[:, None, :]).abs().max())
    report("encoder_vs_reference", case=case, mode=mode, err=e_enc, tol=TOL_ENC)
    assert e_enc < TOL_ENC, e_enc
    _, _, tok = eng.encode(feat_o, flen_o, n_layers_run=0, want_tokens=True)
    pre_ref = torch.from_numpy(gold["pre_encode"])
    assert float(((tok.cpu() - pre_ref) * vm[:, :, None]).abs().max()) < tol_pre(pre_ref * vm[:, :, None])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [c for c in SUPPORTED if "ctc" in c])
def test_ctc_bit_exact_ids_and_frames(case, mode):
    ck, wav, wlen, gold = load_case(case)
    eng = _engine(ck, mode)
    ref = split_ragged(gold["ids"], gold["frames"], gold["counts"].tolist())
    enc_ref = torch.from_numpy(gold["encoded"])
    elen_ref = torch.from_numpy(gold["enc_len"])
    lp = eng.ctc_head(enc_ref).cpu()
    vm = valid_mask(lp.shape[1], gold["enc_len"])
    assert float(((lp - torch.from_numpy(gold["log_probs"])) * vm[:, :, None]).abs().max()) < TOL_LOGP
    # decoder alone on the reference's encoder output
    assert ragged_from_device(*eng.ctc_greedy(enc_ref, elen_ref)) == ref
    # whole path wav -> ids on the GPU
    feat, flen = eng.frontend(wav, wlen)
    enc, elen = eng.encode(feat, flen)
    assert ragged_from_device(*eng.ctc_greedy(enc, elen)) == ref


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [c for c in SUPPORTED if "rnnt" in c])
def test_rnnt_ids_frames_and_logits(case, mode):
    ck, wav, wlen, gold = load_case(case)
    cfg, sd = ck["cfg"], ck["state_dict"]
    eng = _engine(ck, mode)
    ms = cfg["decoding"]["max_symbols_per_step"]
    ref = split_ragged(gold["ids"], gold["frames"], gold["counts"].tolist())
    enc_ref = torch.from_numpy(gold["encoded"])
    elen_ref = torch.from_numpy(gold["enc_len"])
    want = golden_trace(gold)           # the REFERENCE's joint log-probs of every step, per utterance, in order
    cap = max(w.shape[0] for w in want)

    def check(enc, elen, what):
        """ids + frames exact, step counts exact, every joint log-prob within 1e-3 (north_star) -- unconditionally:
        the fixtures hold no near-tie (top-1/top-2 margin > 2e-3 on every step, tests/golden/cases.py)."""
        ids, frames, counts, dump, dcount = eng.rnnt_greedy(enc, elen, ms, dump_cap=cap)
        assert ragged_from_device(ids, frames, counts) == ref, what
        assert dcount.cpu().tolist() == [w.shape[0] for w in want], what
        for i, w in enumerate(want):
            err = float((dump[i, : w.shape[0]].cpu() - w).abs().max())
            report("rnnt_joint_logprobs", case=case, mode=mode, what=what, utt=i, steps=int(w.shape[0]), err=err, tol=TOL_LOGP)
            assert err < TOL_LOGP, (what, i, err)

    # decoder alone on the reference's encoder output
    check(enc_ref, elen_ref, "decoder alone")
    # whole path wav -> ids on the GPU
    feat, flen = eng.frontend(wav, wlen)
    enc, elen = eng.encode(feat, flen)
    check(enc, elen, "whole path")
    # without the dump (the production call) the same ids come back
    assert ragged_from_device(*eng.rnnt_greedy(enc, elen, ms)) == ref


@pytest.mark.parametrize("mode", MODES)
def test_emotion_model_probs(mode):
    """GigaAMEmo path (model.py:272-293): encoder -> gam_emo_probs against the reference's committed
    probabilities (tests/golden/emo_l2.npz), the reference tolerance for this output is 1e-3
    (reference tests/test_loading.py:39-42)."""
    import os
    from common import EMO_CASE, ROOT, make_case_checkpoint
    from gigaam_amd import synth
    ck, wav, wlen = make_case_checkpoint(EMO_CASE)
    b = wav.shape[0]
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "emo_l2.npz")))
    eng = _engine(ck, mode)
    enc, elen = eng.encode(*eng.frontend(wav, wlen))
    # whole-axis mean (forward_for_export) on the utterance that fills the batch; shorter ones would
    # average the padded frames too, which this encoder leaves as don't-care values
    p_all = eng.emo_probs(enc).cpu()
    assert float((p_all[0] - torch.from_numpy(gold["probs_export"][0])).abs().max()) < 1e-4
    want_m = O.emo_probs(ck["state_dict"], torch.from_numpy(gold["encoded"]), torch.from_numpy(gold["enc_len"]))
    assert float((eng.emo_probs(enc, elen).cpu() - want_m).abs().max()) < 1e-4
    # head alone on the reference's encoder output, and the masked-mean variant against the oracle
    enc_ref = torch.from_numpy(gold["encoded"])
    assert float((eng.emo_probs(enc_ref).cpu() - torch.from_numpy(gold["probs_export"])).abs().max()) < 1e-5
    elen_ref = torch.from_numpy(gold["enc_len"])
    want = O.emo_probs(ck["state_dict"], enc_ref, elen_ref)
    assert float((eng.emo_probs(enc_ref, elen_ref).cpu() - want).abs().max()) < 1e-5
    for i in range(b):   # get_probs: one unpadded file
        e1, _ = eng.encode(*eng.frontend(wav[i:i + 1, : int(wlen[i])].contiguous(), wlen[i:i + 1]))
        p = eng.emo_probs(e1).cpu()[0]
        assert float((p - torch.from_numpy(gold["probs_single"][i])).abs().max()) < 1e-4


def test_batched_equals_single_and_edge_lengths():
    """reference tests/test_batching.py:35-122: features are computed per sample, then the
    zero-padded batch through the encoder must equal each sample alone on its valid frames
    (the reference allows atol 0.03; fp32 here is far tighter).  Very short inputs must run."""
    ck, wav, wlen, _ = load_case("v2_ctc_l2")
    eng = _engine(ck)
    singles = [eng.frontend(wav[i:i + 1, : int(wlen[i])].contiguous(), wlen[i:i + 1]) for i in range(wav.shape[0])]
    tmax = max(f.shape[2] for f, _ in singles)
    feat = torch.zeros(len(singles), 64, tmax, device=singles[0][0].device)
    flen = torch.cat([l for _, l in singles])
    for i, (f, _) in enumerate(singles):
        feat[i, :, : f.shape[2]] = f[0]
    enc, elen = eng.encode(feat, flen)
    for i, (f1, l1) in enumerate(singles):
        e1, el1 = eng.encode(f1, l1)
        t = int(el1[0])
        assert int(elen[i]) == t
        assert float((enc[i, :, :t] - e1[0, :, :t]).abs().max()) < 1e-3
    for n in (3200, 5000, 8000, 16000):  # 0.2 s .. 1 s
        w, l = wav[:2, :n].contiguous(), torch.tensor([n, n - 7])
        f, fl = eng.frontend(w, l)
        e, el = eng.encode(f, fl)
        ids, frames, counts = eng.ctc_greedy(e, el)
        assert bool(torch.isfinite(e).all()) and int(counts.max()) <= e.shape[2]
    # zero-length utterance inside a batch: no tokens, nothing crashes
    l0 = torch.tensor([int(wlen[0]), 0, int(wlen[2])])
    f, fl = eng.frontend(wav, l0)
    e, el = eng.encode(f, torch.tensor([int(fl[0]), 0, int(fl[2])]))
    ids, frames, counts = eng.ctc_greedy(e, el)
    assert int(el[1]) == 0 and int(counts[1]) == 0 and bool(torch.isfinite(e).all())


def test_model_api_transcribe(tmp_path):
    """load_model()/transcribe()/embed_audio() surface on a PCM16 wav (config 1 plumbing)."""
    import wave
    import gigaam_amd
    from gigaam_amd import synth
    ck = synth.make_checkpoint("v2_ctc", seed=1, n_layers=2)
    path = str(tmp_path / "model.ckpt")
    torch.save(ck, path)
    model = gigaam_amd.load_model(path, fp16_encoder=False, device="cuda:0")   # the fp32 contract of the reference's CPU path
    wav, wlen = synth.synth_audio(1, 5.0, seed=0)
    pcm = (wav[0].numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16)
    wpath = str(tmp_path / "clip.wav")
    with wave.open(wpath, "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000); wf.writeframes(pcm.tobytes())
    res = model.transcribe(wpath, word_timestamps=True)
    x = torch.from_numpy(pcm.astype(np.float32) / 32768.0)[None]
    with torch.no_grad():
        dec, enc_o, elen_o = O.transcribe_ids(ck, x, torch.tensor([x.shape[1]]))
    text = "".join(synth.CHAR_VOCAB[i] for i in dec[0][0])
    assert str(res) == text and res.words is not None
    enc, elen = model.embed_audio(wpath)
    assert enc.shape == enc_o.shape and int(elen[0]) == int(elen_o[0])
    assert float((enc.cpu() - enc_o).abs().max()) < 1e-3
    out = model.transcribe_longform(wpath, speech_regions=[(0.0, 2.4), (2.6, 5.0)], min_duration=1.0, max_duration=2.5)
    assert len(out) == 2 and all(isinstance(s.text, str) for s in out)
    # longform through the pinned double-buffered feeder == the same zero-padded batches fed by hand
    # (batched vs single may legitimately differ: the frontend reflects at the BATCH end, as the reference does)
    from gigaam_amd.vad_utils import segment_audio_file
    regs = [(0.0, 1.1), (1.2, 2.4), (2.6, 3.3), (3.5, 5.0)]
    kw = dict(speech_regions=regs, min_duration=0.5, max_duration=1.0)
    a1 = model.transcribe_longform(wpath, fr_batch_size=1, **kw)
    a3 = model.transcribe_longform(wpath, fr_batch_size=3, word_timestamps=True, **kw)
    segs, bounds = segment_audio_file(wpath, 16000, **kw)
    manual = []
    for i0 in (0, 3):
        chunk = segs[i0:i0 + 3]
        lens = torch.tensor([c.shape[0] for c in chunk])
        pad = torch.zeros(len(chunk), int(lens.max()))
        for j, c in enumerate(chunk):
            pad[j, : c.shape[0]] = c
        manual += [t for t, _ in model.transcribe_batch(pad, lens)]
    assert len(a1) == len(a3) == 4 and [s.text for s in a3] == manual and bounds == regs
    assert [s.text for s in a1] == [model.transcribe_batch(c[None], torch.tensor([c.shape[0]]))[0][0] for c in segs]
    assert [(s.start, s.end) for s in a3] == regs and a3.has_word_timestamps


def test_model_api_emotion(tmp_path):
    """load_model() -> GigaAMEmo.get_probs(wav_file) -> {name: prob} (reference model.py:272-285)."""
    import wave
    import gigaam_amd
    from gigaam_amd import synth
    ck = synth.make_checkpoint("emo", seed=1, n_layers=2)
    path = str(tmp_path / "emo.ckpt")
    torch.save(ck, path)
    model = gigaam_amd.load_model(path, fp16_encoder=False, device="cuda:0")
    assert isinstance(model, gigaam_amd.GigaAMEmo)
    wav, _ = synth.synth_audio(1, 3.0, seed=5)
    pcm = (wav[0].numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16)
    wpath = str(tmp_path / "clip.wav")
    with wave.open(wpath, "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000); wf.writeframes(pcm.tobytes())
    probs = model.get_probs(wpath)
    assert list(probs) == synth.EMO_NAMES and abs(sum(probs.values()) - 1.0) < 1e-5
    x = torch.from_numpy(pcm.astype(np.float32) / 32768.0)[None]
    with torch.no_grad():
        feat, flen = oracle_features(ck, x, torch.tensor([x.shape[1]]))
        enc, _ = O.encoder_forward(ck["state_dict"], ck["cfg"]["encoder"], feat, flen)
        want = O.emo_probs(ck["state_dict"], enc)[0]
    assert max(abs(probs[n] - float(want[i])) for i, n in enumerate(synth.EMO_NAMES)) < 1e-3   # reference bar: ±1e-3
    pb = model.get_probs_batch(x.repeat(2, 1), torch.tensor([x.shape[1], x.shape[1]])).cpu()
    assert float((pb[0] - pb[1]).abs().max()) < 1e-6 and float((pb[0] - want).abs().max()) < 1e-3


def test_energy_vad_stand_in(tmp_path):
    """vad="energy": tone bursts separated by silence come back as regions within a few frames, and the
    longform driver runs end to end on them (the detector is a labelled stand-in for pyannote)."""
    import wave
    import gigaam_amd
    from gigaam_amd import synth
    from gigaam_amd.vad_utils import EnergyVAD
    ck = synth.make_checkpoint("v2_ctc", seed=1, n_layers=2)
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    sr = 16000
    truth = [(1.0, 3.5), (4.2, 9.0), (10.5, 11.2), (13.0, 19.0)]
    tone, _ = synth.synth_audio(1, 20.0, seed=9)
    g = torch.Generator().manual_seed(1)
    audio = 1e-4 * torch.randn(20 * sr, generator=g)
    for s0, e0 in truth:
        audio[int(s0 * sr): int(e0 * sr)] += tone[0, int(s0 * sr): int(e0 * sr)]
    got = EnergyVAD(model.preprocessor)(audio, sr)
    assert len(got) == len(truth)
    assert all(abs(a - s0) < 0.12 and abs(b - e0) < 0.12 for (a, b), (s0, e0) in zip(got, truth))
    pcm = (audio.numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16)
    wpath = str(tmp_path / "bursts.wav")
    with wave.open(wpath, "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(sr); wf.writeframes(pcm.tobytes())
    out = model.transcribe_longform(wpath, vad="energy", min_duration=2.0, max_duration=6.0)
    assert len(out) >= 2 and out.segments[0].start < 1.2 and out.segments[-1].end > 18.8


@pytest.mark.parametrize("case", ["v2_ctc_l2", "v1_ctc_l2", "v3_e2e_ctc_l2"])
@pytest.mark.parametrize("mode", ["f16x3", "f32"])
def test_small_batch_graph_replay_is_bit_identical(mode, case):
    """Small batches replay the Conformer-layer launch sequence as a hipGraph from the third call of a
    shape on (first: plain launches, second: capture): every call must return the same bits, shapes may
    interleave, and a workspace growth in between must not leave a stale graph behind.  The cases are the
    forms of the captured sequence: rotary / rel_pos (linear_pos GEMM and pbuf), BatchNorm / LayerNorm conv
    module, conv2d / conv1d stem in front of it."""
    ck, wav, wlen, gold = load_case(case)
    eng = _engine(ck, mode)
    feat, flen = eng.frontend(wav, wlen)
    outs = [eng.encode(feat, flen)[0].clone() for _ in range(3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    vm = valid_mask(outs[0].shape[2], gold["enc_len"])
    assert float(((outs[2].cpu() - torch.from_numpy(gold["encoded"])) * vm[:, None, :]).abs().max()) < TOL_ENC
    # another shape in between (and a bigger one: workspaces regrow, pointers move)
    n1 = min(200, feat.shape[2])
    f1, l1 = feat[:1, :, :n1].contiguous(), torch.tensor([n1], device=feat.device)
    one = [eng.encode(f1, l1)[0].clone() for _ in range(4)]
    assert all(torch.equal(one[0], o) for o in one[1:])
    big = torch.cat([feat, feat, feat], dim=0)
    bl = torch.cat([flen, flen, flen])
    b0 = eng.encode(big, bl)[0]
    nb = feat.shape[0]
    assert torch.equal(b0[:nb], outs[0]) or float((b0[:nb] - outs[0]).abs().max()) < 1e-5
    again = [eng.encode(feat, flen)[0] for _ in range(3)]
    assert all(torch.equal(outs[0], o) for o in again)
    assert all(torch.equal(one[0], eng.encode(f1, l1)[0]) for _ in range(3))


def _reference_test_audio(duration, sr=16000, seed=0):
    """generate_test_audio of reference tests/test_batching.py:15-25 (220/440/660 Hz + noise, Tukey 0.1), seeded."""
    from scipy import signal
    rng = np.random.RandomState(seed)
    t = np.linspace(0, duration, int(sr * duration))
    audio = (0.5 * np.sin(2 * np.pi * 220 * t) + 0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 660 * t)
             + 0.1 * rng.normal(0, 0.1, len(t)))
    return torch.from_numpy((audio * signal.windows.tukey(len(audio), alpha=0.1)).astype(np.float32))


@pytest.mark.parametrize("revision", ["v3_ctc", "v3_e2e_rnnt"])
@pytest.mark.parametrize("batch_size", [1, 2, 4])
def test_model_batching_v3(revision, batch_size):
    """reference tests/test_batching.py:86-122 (v3_ctc / v3_e2e_rnnt, B in {1,2,4}, durations linspace(2.5 s, 5 s)):
    per-sample features, zero-padded into a batch, through the encoder == each sample alone, on its valid frames.
    The reference allows atol 0.03 (fp16 autocast on its GPU path); this path is fp32 and holds 1e-3."""
    from gigaam_amd import synth
    from gigaam_amd.feeder import collate
    ck = synth.make_checkpoint(revision, seed=1, n_layers=2)
    eng = _engine(ck)
    wavs = [_reference_test_audio(d, seed=i) for i, d in enumerate(np.linspace(2.5, 5.0, batch_size))]
    wav, wlen = collate(wavs)
    singles = [eng.frontend(wav[i:i + 1, : int(wlen[i])].contiguous(), wlen[i:i + 1]) for i in range(batch_size)]
    tmax = max(f.shape[2] for f, _ in singles)
    feat = torch.zeros(batch_size, 64, tmax, device=singles[0][0].device)
    for i, (f, _) in enumerate(singles):
        feat[i, :, : f.shape[2]] = f[0]
    flen = torch.cat([l for _, l in singles])
    enc, elen = eng.encode(feat, flen)
    for i, (f1, l1) in enumerate(singles):
        e1, el1 = eng.encode(f1, l1)
        t = int(el1[0])
        assert int(elen[i]) == t and enc.shape[:2] == (batch_size, 768)
        diff = float((enc[i, :, :t] - e1[0, :, :t]).abs().max())
        assert diff < 1e-3, (revision, batch_size, i, diff)
    # the decoders see the same thing: batched ids == single ids
    cfg = ck["cfg"]
    for i, (f1, l1) in enumerate(singles):
        e1, el1 = eng.encode(f1, l1)
        if revision.endswith("ctc"):
            one = ragged_from_device(*eng.ctc_greedy(e1, el1))[0]
            many = ragged_from_device(*eng.ctc_greedy(enc, elen))[i]
        else:
            ms = cfg["decoding"]["max_symbols_per_step"]
            one = ragged_from_device(*eng.rnnt_greedy(e1, el1, ms))[0]
            many = ragged_from_device(*eng.rnnt_greedy(enc, elen, ms))[i]
        # (ids can legitimately differ only through a near-tie; on these seeds there is none)
        assert one == many, (revision, batch_size, i)


@pytest.mark.parametrize("revision", ["v3_ctc", "v3_e2e_rnnt"])
def test_batching_edge_cases_v3(revision):
    """reference tests/test_batching.py:125-140: randn(2, 5000) with lengths [3200, 5000] must run."""
    from gigaam_amd import synth
    ck = synth.make_checkpoint(revision, seed=1, n_layers=2)
    eng = _engine(ck)
    g = torch.Generator().manual_seed(0)
    wav = torch.randn(2, 5000, generator=g)
    wlen = torch.tensor([3200, 5000])
    enc, elen = eng.encode(*eng.frontend(wav, wlen))
    assert enc.shape[0] == 2 and bool(torch.isfinite(enc).all()) and elen.cpu().tolist() == [5, 8]


@pytest.mark.parametrize("cluster", ["0", "1", "2", "3", "4", "5", "6", "7", "8"])
@pytest.mark.parametrize("case", ["v2_rnnt_l2", "v3_e2e_rnnt_l2_dense"])
def test_rnnt_cluster_sizes(case, cluster, monkeypatch):
    """The RNN-T decode with C workgroups per utterance (gam_decode_cluster.h) for every way of slicing the hidden
    units / joint rows / classes over the cluster, and the one-workgroup kernel (C = 0): ids, frames, number of joint
    evaluations and every log-prob against the reference's, exactly as in test_rnnt_ids_frames_and_logits.  Without the
    repair pass (GAM_RNNT_NO_REPAIR=1, read at gam_create) and with gam_rnnt_last_decode's word that the requested size ran,
    so the one-workgroup kernel cannot stand in for a cluster that gave up or a launch the runtime refused."""
    monkeypatch.setenv("GAM_RNNT_CLUSTER", cluster)
    monkeypatch.setenv("GAM_RNNT_NO_REPAIR", "1")
    ck, wav, wlen, gold = load_case(case)
    eng = _engine(ck)
    ms = ck["cfg"]["decoding"]["max_symbols_per_step"]
    ref = split_ragged(gold["ids"], gold["frames"], gold["counts"].tolist())
    want = golden_trace(gold)
    enc_ref, elen_ref = torch.from_numpy(gold["encoded"]), torch.from_numpy(gold["enc_len"])
    ids, frames, counts, dump, dcount = eng.rnnt_greedy(enc_ref, elen_ref, ms, dump_cap=max(w.shape[0] for w in want))
    ran_c, ran_kern, refused = eng.rnnt_last_decode()
    assert (ran_c, refused) == (int(cluster), False) and (ran_kern >= 0) == (ran_c > 0), (case, cluster, ran_c, ran_kern, refused)
    assert min(counts.cpu().tolist()) >= 0, (case, cluster, counts.cpu().tolist())     # no cluster gave up
    assert ragged_from_device(ids, frames, counts) == ref
    assert dcount.cpu().tolist() == [w.shape[0] for w in want]
    for i, w in enumerate(want):
        err = float((dump[i, : w.shape[0]].cpu() - w).abs().max())
        assert err < TOL_LOGP, (case, cluster, i, err)
    # reruns are bit-identical (the hand-off carries no race)
    for _ in range(3):
        again = eng.rnnt_greedy(enc_ref, elen_ref, ms)
        assert ragged_from_device(*again) == ref


@pytest.mark.parametrize("coop", ["1", "0"])
@pytest.mark.parametrize("case", ["v2_rnnt_l2", "v3_e2e_rnnt_l2_dense"])
def test_rnnt_cluster_failure_is_repaired(case, coop, monkeypatch):
    """VERDICT r2 #7 / ADVICE r2: a decode cluster that gives up (a member not resident: GPU shared with another job)
    must not surface as an exception.  GAM_RNNT_FORCE_TIMEOUT=1 makes the cluster of every odd utterance report a failed
    hand-off (counts[b] = -1, exactly what a real timeout leaves behind); the repair pass gam_rnnt_greedy launches behind
    every cluster launch re-decodes those utterances with the one-workgroup kernel.  The caller sees the reference's ids,
    frames, step counts and log-probs for ALL utterances -- under the cooperative and the plain launch."""
    monkeypatch.setenv("GAM_RNNT_FORCE_TIMEOUT", "1")
    monkeypatch.setenv("GAM_RNNT_COOP", coop)
    ck, wav, wlen, gold = load_case(case)
    eng = _engine(ck)
    ms = ck["cfg"]["decoding"]["max_symbols_per_step"]
    ref = split_ragged(gold["ids"], gold["frames"], gold["counts"].tolist())
    want = golden_trace(gold)
    assert len(ref) >= 2       # (utterance 1 goes through the repair pass, utterance 0 through the cluster)
    enc_ref, elen_ref = torch.from_numpy(gold["encoded"]), torch.from_numpy(gold["enc_len"])
    ids, frames, counts, dump, dcount = eng.rnnt_greedy(enc_ref, elen_ref, ms, dump_cap=max(w.shape[0] for w in want))
    assert min(counts.cpu().tolist()) >= 0
    assert ragged_from_device(ids, frames, counts) == ref
    assert dcount.cpu().tolist() == [w.shape[0] for w in want]
    for i, w in enumerate(want):
        assert float((dump[i, : w.shape[0]].cpu() - w).abs().max()) < TOL_LOGP, (case, coop, i)
    # through the model API: no exception, the oracle's texts
    import gigaam_amd
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    got = model.transcribe_batch(wav, wlen)
    tok = model.decoding.tokenizer
    assert [t for t, _ in got] == [tok.decode(i) for i, _ in ref]


def test_fp16_encoder_contract(tmp_path):
    """load_model(fp16_encoder=True) on a GPU (the reference's default, gigaam/__init__.py:188-189; model.py:39-55):
    ``_dtype`` is float16, prepare_wav hands the model a float16 waveform, embed_audio returns float16 -- here with
    fp32 arithmetic inside, so the result equals the fp32 path on the same (fp16-rounded) waveform, rounded once."""
    import wave
    import gigaam_amd
    from gigaam_amd import synth
    ck = synth.make_checkpoint("v2_ctc", seed=1, n_layers=2)
    path = str(tmp_path / "model.ckpt")
    torch.save(ck, path)
    m16 = gigaam_amd.load_model(path, device="cuda:0")                       # fp16_encoder defaults to True
    m32 = gigaam_amd.load_model(path, fp16_encoder=False, device="cuda:0")
    assert m16._dtype == torch.float16 and m32._dtype == torch.float32 and m16._device.type == "cuda"
    wav, _ = synth.synth_audio(1, 3.0, seed=4)
    pcm = (wav[0].numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16)
    wpath = str(tmp_path / "clip.wav")
    with wave.open(wpath, "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000); wf.writeframes(pcm.tobytes())
    w16, l16 = m16.prepare_wav(wpath)
    assert w16.dtype == torch.float16
    e16, n16 = m16.embed_audio(wpath)
    assert e16.dtype == torch.float16 and n16.dtype == torch.int32
    e32, n32 = m32.forward(w16.float(), l16)      # the same fp16-rounded samples through the fp32 contract
    assert torch.equal(n16, n32) and torch.equal(e16, e32.half())
    # the DEFAULT user path (fp16_encoder=True) must decode like the fp32 contract -- the transcribe paths feed
    # the head the kernels' fp32 output and the fp32 PCM samples; only what forward / embed_audio RETURN is rounded to fp16
    x = torch.from_numpy(pcm.astype(np.float32) / 32768.0)[None]
    with torch.no_grad():
        dec, _, _ = O.transcribe_ids(ck, x, torch.tensor([x.shape[1]]))
    want = "".join(synth.CHAR_VOCAB[i] for i in dec[0][0])
    assert m16.transcribe(wpath).text == m32.transcribe(wpath).text == want
    assert [t for t, _ in m16.transcribe_batch(x, torch.tensor([x.shape[1]]))] == [want]


def test_word_timestamps_match_oracle_derived_words(tmp_path):
    """transcribe(word_timestamps=True).words on the GPU == frames_to_words over the ORACLE's ids / frames (the function
    itself is pinned to the reference's by tests/test_host_golden.py): texts equal, start / end equal to the float."""
    import wave
    import gigaam_amd
    from gigaam_amd import synth
    from gigaam_amd.decoding import Tokenizer
    from gigaam_amd.timestamps_utils import compute_frame_shift, frames_to_words
    ck = synth.make_checkpoint("v2_ctc", seed=1, n_layers=2)
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    wav, _ = synth.synth_audio(1, 6.0, seed=24)   # (4 words in the oracle decode)
    pcm = (wav[0].numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16)
    wpath = str(tmp_path / "clip.wav")
    with wave.open(wpath, "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000); wf.writeframes(pcm.tobytes())
    res = model.transcribe(wpath, word_timestamps=True)
    x = torch.from_numpy(pcm.astype(np.float32) / 32768.0)[None]
    with torch.no_grad():
        dec, _, elen_o = O.transcribe_ids(ck, x, torch.tensor([x.shape[1]]))
    ids, frames = dec[0]
    want = frames_to_words(Tokenizer(synth.CHAR_VOCAB), ids, frames, compute_frame_shift(x.shape[1], int(elen_o[0])))
    assert len(want) >= 3
    assert [(w.text, w.start, w.end) for w in res.words] == [(w.text, w.start, w.end) for w in want]
    # longform: the same words, offset by the segment start and rounded to 3 decimals (model.py:246-250)
    lf = model.transcribe_longform(wpath, word_timestamps=True, speech_regions=[(0.0, 6.0)], min_duration=1.0, max_duration=8.0)
    assert [(w.text, w.start, w.end) for w in lf.segments[0].words] == [(w.text, round(w.start, 3), round(w.end, 3)) for w in want]


def test_batch_feeder_matches_reference_collate():
    """The pinned, double-buffered feeder hands the GPU exactly the reference's collate layout
    (gigaam/utils.py:371-380; fixture tests/golden/host_logic.json), batch after batch, on the side stream."""
    import hashlib
    import json
    import os
    from common import ROOT
    from gigaam_amd.feeder import BatchFeeder
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "host_logic.json"), encoding="utf-8"))["collate"]

    def seeded_audio(n, seed):
        g = np.random.Generator(np.random.PCG64(seed))
        return torch.from_numpy(g.standard_normal(n, dtype=np.float32) * np.float32(0.1))

    for c in fx:
        wavs = [seeded_audio(n, 1000 * c["seed"] + j) for j, n in enumerate(c["lens"])]
        got = list(BatchFeeder(wavs, len(wavs), torch.device("cuda:0")))
        assert len(got) == 1
        wav, lens = got[0]
        torch.cuda.synchronize()
        assert wav.is_cuda and list(wav.shape) == c["shape"] and lens.cpu().tolist() == c["lengths"]
        assert hashlib.sha256(wav.cpu().contiguous().numpy().tobytes()).hexdigest()[:16] == c["batch_sha"]
    # several batches, ragged tail: concatenation of the batches == the segments, in order
    segs = [seeded_audio(100 + 37 * i, i) for i in range(11)]
    out = []
    for wav, lens in BatchFeeder(segs, 4, torch.device("cuda:0")):
        torch.cuda.synchronize()
        out += [wav[j, : int(n)].cpu() for j, n in enumerate(lens.cpu().tolist())]
    assert len(out) == 11 and all(torch.equal(a, b) for a, b in zip(out, segs))


@pytest.mark.parametrize("case", ["v2_ctc_l2", "v3_ctc_l2", "v1_ctc_l2"])
def test_long_utterance_and_length_limit(case):
    """A 100 s utterance (T' = 2500: 40 key tiles per query block, 2T'-1 = 4999 relative positions for v1) batched with
    a 7 s one: lengths, encoder output and CTC log-probs against the CPU oracle at the usual bars.  (ids are not
    compared here: over 2500 frames of a random-init head the oracle's own top-2 margin falls to 1e-6..1e-4, below any
    fp32 implementation's reproducibility; the bit-exact ids checks run on the margin-selected goldens.)  Past
    pos_emb_max_len encoder frames the reference's PE slice comes up short (encoder.py:357-361, 606-607): here a clean
    error."""
    from gigaam_amd import synth
    from gigaam_amd._lib import GigaAMHipError
    ck, _, _, _ = load_case(case)
    wav, _ = synth.synth_audio(2, 100.0, seed=31)
    wlen = torch.tensor([wav.shape[1], 7 * 16000 + 123])
    eng = _engine(ck)
    feat_o, flen_o = oracle_features(ck, wav, wlen)
    feat, flen = eng.frontend(wav, wlen)
    assert flen.cpu().tolist() == flen_o.tolist()
    assert logmel_err(feat.cpu(), feat_o, valid_mask(feat_o.shape[2], flen_o))[0] < TOL_FEAT
    enc, elen = eng.encode(feat_o, flen_o)          # (the oracle's features in, as in test_encoder_matches_reference_golden)
    logp = eng.ctc_head(enc)
    with torch.no_grad():
        enc_ref, elen_ref = O.encoder_forward(ck["state_dict"], ck["cfg"]["encoder"], feat_o, flen_o)
        logp_ref = O.ctc_log_probs(ck["state_dict"], enc_ref)
    assert elen.cpu().tolist() == elen_ref.tolist()
    m = valid_mask(enc_ref.shape[2], elen_ref)
    err = float(((enc.cpu() - enc_ref).abs() * m[:, None, :]).max())
    err_lp = float(((logp.cpu() - logp_ref).abs() * m[:, :, None]).max())
    report("long_utterance", case=case, frames=int(elen_ref.max()), enc_err=err, logp_err=err_lp)
    assert err < TOL_ENC, (case, err)
    assert err_lp < TOL_LOGP, (case, err_lp)
    # 201 s -> 5026 encoder frames > pos_emb_max_len = 5000
    too_long = torch.zeros(1, 201 * 16000)
    f2, l2 = eng.frontend(too_long, torch.tensor([too_long.shape[1]]))
    with pytest.raises(GigaAMHipError, match="pos_emb_max_len"):
        eng.encode(f2, l2)


@pytest.mark.parametrize("case,seed", [("v2_rnnt_l2", 56), ("v3_e2e_rnnt_l2", 54)])
def test_rnnt_long_utterance(case, seed):
    """RNN-T greedy over a 60 s utterance (1500 frames, 300-800 tokens, ~2100-2650 joint evaluations -- 20x the
    goldens' length, so tags, parities and the 16-frame windows of the cluster decode turn over hundreds of times)
    batched with a 9 s one, against the oracle's decode: ids, frames, step counts and every joint log-prob.  The seeds
    were chosen so that the oracle's own top-1/top-2 margin stays above RNNT_MIN_MARGIN on every step (asserted)."""
    from common import RNNT_MIN_MARGIN
    from gigaam_amd import synth
    ck, _, _, _ = load_case(case)
    cfg, sd = ck["cfg"], ck["state_dict"]
    ms = cfg["decoding"]["max_symbols_per_step"]
    wav, _ = synth.synth_audio(2, 60.0, seed=seed)
    wlen = torch.tensor([wav.shape[1], 9 * 16000 + 77])
    feat_o, flen_o = oracle_features(ck, wav, wlen)
    with torch.no_grad():
        enc_o, elen_o = O.encoder_forward(sd, cfg["encoder"], feat_o, flen_o)
        trace = []
        ref = O.rnnt_greedy(sd, enc_o, elen_o, ms, cfg["head"]["decoder"]["pred_rnn_layers"], trace=trace)
    want = [torch.stack([lp for (i, _, lp) in trace if i == b]) for b in range(2)]
    margin = min(float((w.topk(2, dim=-1).values[:, 0] - w.topk(2, dim=-1).values[:, 1]).min()) for w in want)
    assert margin > RNNT_MIN_MARGIN, margin
    eng = _engine(ck)
    cap = max(w.shape[0] for w in want)

    def check(enc, elen, what):
        ids, frames, counts, dump, dcount = eng.rnnt_greedy(enc, elen, ms, dump_cap=cap)
        assert ragged_from_device(ids, frames, counts) == ref, what
        assert dcount.cpu().tolist() == [w.shape[0] for w in want], what
        for i, w in enumerate(want):
            err = float((dump[i, : w.shape[0]].cpu() - w).abs().max())
            report("rnnt_long_utterance", case=case, what=what, utt=i, steps=int(w.shape[0]), tokens=len(ref[i][0]), err=err, margin=margin)
            assert err < TOL_LOGP, (what, i, err)

    check(enc_o, elen_o, "decoder alone")
    feat, flen = eng.frontend(wav, wlen)
    check(*eng.encode(feat, flen), "whole path")
    assert ragged_from_device(*eng.rnnt_greedy(enc_o, elen_o, ms)) == ref


@pytest.mark.parametrize("copies", [14, 33, 90])
def test_rnnt_batch_sizes_and_cluster_mapping(copies):
    """The cluster decode picks its size from the batch (gam_api.hip: C = min(8, (CUs - 16) / (8 ceil(B / 8)))) and maps
    workgroup -> (utterance, member) through the XCD-aware rule of gam_decode_cluster.h.  The golden's 3 utterances
    tiled to B = 42 (C = 5), 99 (C = 2) and 270 (C = 0: the one-workgroup kernel): every copy must decode to the
    reference's ids and frames."""
    ck, _, _, gold = load_case("v2_rnnt_l2")
    eng = _engine(ck)
    ms = ck["cfg"]["decoding"]["max_symbols_per_step"]
    ref = split_ragged(gold["ids"], gold["frames"], gold["counts"].tolist())
    enc = torch.from_numpy(gold["encoded"]).repeat(copies, 1, 1)
    elen = torch.from_numpy(gold["enc_len"]).repeat(copies)
    got = ragged_from_device(*eng.rnnt_greedy(enc, elen, ms))
    assert len(got) == 3 * copies
    bad = [i for i, g in enumerate(got) if g != ref[i % 3]]
    assert not bad, bad[:10]


@pytest.mark.parametrize("max_duration", [0.5, 1.0])
def test_different_audio_lengths_v3_e2e_ctc(max_duration):
    """reference tests/test_batching.py:143-159: v3_e2e_ctc on a batch of two clips of 0.5 x and 1 x max_duration
    (0.25 s .. 1 s: a handful of encoder frames) must run and return two rows -- here also checked against the oracle."""
    from gigaam_amd import synth
    from gigaam_amd.feeder import collate
    ck = synth.make_checkpoint("v3_e2e_ctc", seed=1, n_layers=2)
    eng = _engine(ck)
    wav, wlen = collate([_reference_test_audio(d, seed=i) for i, d in enumerate(np.linspace(max_duration * 0.5, max_duration, 2))])
    feat_o, flen_o = oracle_features(ck, wav, wlen)
    enc, elen = eng.encode(*eng.frontend(wav, wlen))
    assert enc.shape[0] == 2 and bool(torch.isfinite(enc).all())
    enc2, elen2 = eng.encode(feat_o, flen_o)
    with torch.no_grad():
        enc_ref, elen_ref = O.encoder_forward(ck["state_dict"], ck["cfg"]["encoder"], feat_o, flen_o)
    assert elen.cpu().tolist() == elen_ref.tolist() == elen2.cpu().tolist()
    m = valid_mask(enc_ref.shape[2], elen_ref)
    assert float(((enc2.cpu() - enc_ref).abs() * m[:, None, :]).max()) < TOL_ENC


def test_longform_consistency(tmp_path):
    """reference tests/test_longform.py:183-205: two transcribe_longform runs over the same 30 s file give the same
    segments and boundaries (here: and the same text -- the kernels are deterministic)."""
    import wave
    import gigaam_amd
    from gigaam_amd import synth
    ck = synth.make_checkpoint("v2_ctc", seed=1, n_layers=2)
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    wav, _ = synth.synth_audio(1, 30.0, seed=12)
    pcm = (wav[0].numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16)
    wpath = str(tmp_path / "long.wav")
    with wave.open(wpath, "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000); wf.writeframes(pcm.tobytes())
    kw = dict(speech_regions=[(0.3, 7.9), (8.4, 13.0), (13.1, 21.7), (22.5, 29.6)], min_duration=3.0, max_duration=9.0)
    r1 = model.transcribe_longform(wpath, **kw)
    r2 = model.transcribe_longform(wpath, **kw)
    assert len(r1.segments) == len(r2.segments) >= 2
    for a, b in zip(r1.segments, r2.segments):
        assert (a.start, a.end) == (b.start, b.end) and a.text == b.text


def test_longform_rnnt_overlapped_pipeline_matches_per_batch_decodes(tmp_path):
    """r05: transcribe_longform of an RNN-T model runs the greedy decode of batch n on the side stream beside the encoder of batch n + 1
    (model.launch_batch(overlap=True) for every batch but the last).  Five batches of a 60 s file: the segments' texts must equal what the
    same chunks give decoded batch by batch with the decode in front (transcribe_batch), and two runs must agree."""
    import wave
    import gigaam_amd
    from gigaam_amd import synth
    from gigaam_amd.feeder import batches, collate
    from gigaam_amd.vad_utils import pack_regions
    ck = synth.make_checkpoint("v2_rnnt", seed=1, n_layers=2, rnnt_blank_bias=13.5)
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    wav, _ = synth.synth_audio(1, 60.0, seed=21)
    pcm = (wav[0].numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16)
    wpath = str(tmp_path / "long_rnnt.wav")
    with wave.open(wpath, "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000); wf.writeframes(pcm.tobytes())
    regions = [(0.2 + 4.0 * i, 3.9 + 4.0 * i) for i in range(14)]
    kw = dict(speech_regions=regions, min_duration=1.0, max_duration=4.5, fr_batch_size=3)
    r1 = model.transcribe_longform(wpath, **kw)
    r2 = model.transcribe_longform(wpath, **kw)
    assert len(r1.segments) >= 12 and [s.text for s in r1.segments] == [s.text for s in r2.segments]
    audio = torch.from_numpy(pcm.astype(np.float32) / 32768.0)
    bounds = pack_regions(regions, audio.shape[0] / 16000.0, min_duration=1.0, max_duration=4.5)
    assert [(s.start, s.end) for s in r1.segments] == [tuple(b) for b in bounds]
    chunks = [audio[int(s * 16000): int(e * 16000)] for s, e in bounds]
    want = []
    for c in batches(chunks, 3):
        want += [t for t, _ in model.transcribe_batch(*collate(c))]
    got = [s.text for s in r1.segments]
    # (the overlapped decodes use smaller clusters than the serial ones: a logit may move by 1e-6, which only a near-tie shows)
    assert sum(a == b for a, b in zip(got, want)) >= len(want) - 1 and sum(len(t) for t in want) > 20, (got, want)


@pytest.mark.parametrize("revision", ["v3_ctc", "v3_e2e_ctc"])
def test_transcribe_result_structure_v3(revision, tmp_path):
    """reference tests/test_timestamps.py:112-215 on synthetic checkpoints: the structure and ordering invariants of
    transcribe / transcribe_longform results with and without word timestamps.  v3_e2e_ctc runs with a REAL
    SentencePiece model (tests/golden/spm256.model: 256 pieces + blank = the head's 257 classes), so the e2e
    tokenizer path (decoding.py:30-44, timestamps_utils.py:29-53) is exercised end to end on the GPU."""
    import os
    import wave
    import gigaam_amd
    from common import ROOT
    from gigaam_amd import synth
    from gigaam_amd.types import LongformTranscriptionResult, Segment, TranscriptionResult, Word
    ck = synth.make_checkpoint(revision, seed=1, n_layers=2)
    if "e2e" in revision:
        ck["cfg"]["decoding"]["model_path"] = os.path.join(ROOT, "tests", "golden", "spm256.model")
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    wav, _ = synth.synth_audio(1, 12.0, seed=17)
    pcm = (wav[0].numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16)
    wpath = str(tmp_path / "clip.wav")
    with wave.open(wpath, "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000); wf.writeframes(pcm.tobytes())

    plain = model.transcribe(wpath)
    assert isinstance(plain, TranscriptionResult) and isinstance(str(plain), str) and len(str(plain)) > 0 and plain.words is None
    res = model.transcribe(wpath, word_timestamps=True)
    assert isinstance(res, TranscriptionResult) and res.text == plain.text and isinstance(res.words, list) and len(res.words) > 0
    prev_end = 0.0
    for w in res.words:
        assert isinstance(w, Word) and isinstance(w.text, str) and w.start < w.end and w.start >= prev_end - 0.01
        assert w.end <= 12.0 + 0.04
        prev_end = w.end
    assert " ".join(w.text for w in res.words) == " ".join(res.text.split())   # (runs of spaces make no empty words)

    regs = [(0.2, 5.6), (6.1, 11.8)]
    lf = model.transcribe_longform(wpath, speech_regions=regs, min_duration=2.0, max_duration=7.0)
    assert isinstance(lf, LongformTranscriptionResult) and len(lf.segments) == 2
    for seg in lf.segments:
        assert isinstance(seg, Segment) and isinstance(seg.text, str) and seg.start < seg.end and seg.words is None
    lfw = model.transcribe_longform(wpath, word_timestamps=True, speech_regions=regs, min_duration=2.0, max_duration=7.0)
    assert [s.text for s in lfw.segments] == [s.text for s in lf.segments]
    for seg in lfw.segments:
        assert seg.words is not None and all(isinstance(w, Word) for w in seg.words)
        assert all(seg.start - 1e-6 <= w.start < w.end <= seg.end + 0.05 for w in seg.words)
    assert len(lfw.words) > 0 and all(w.start < w.end for w in lfw.words)


@pytest.mark.parametrize("case", ["v2_ctc_l2", "v3_ctc_l2", "v1_ctc_l2"])
def test_fused_splitk_reduce_is_bit_identical(case, monkeypatch):
    """r03: at small grids the residual GEMMs run as split-K slices whose sum is taken by the LayerNorm that follows
    (gam_norm.h) instead of gam_splitk_reduce_kernel.  Both add the slices in slice order and apply bias, alpha and the
    residual in the same order, so the encoder output must be BIT-identical with the fusion on and off -- and identical
    from run to run (no atomics anywhere in the reduction)."""
    from gigaam_amd.engine import HipEngine, build_config
    ck, wav, wlen, gold = load_case(case)
    cfg = ck["cfg"]
    feat_o, flen_o = oracle_features(ck, wav, wlen)
    outs = []
    for fuse in ("1", "0", "1"):
        monkeypatch.setenv("GAM_FUSE_REDUCE", fuse)
        eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), ck["state_dict"], torch.device("cuda:0"))
        enc, elen = eng.encode(feat_o, flen_o)
        outs.append(enc.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    vm = valid_mask(outs[0].shape[2], gold["enc_len"])
    assert float(((outs[0] - torch.from_numpy(gold["encoded"])) * vm[:, None, :]).abs().max()) < TOL_ENC
