"""The FRONT of the pipeline against fp64: both subsampling stems (gam_stem.h, the stem GEMMs of gam_encode* with their operand modes --
the implicit-GEMM conv operand, overlapping rows, the per-utterance row mask, the output remap, skip_pad, the split / fp16 C stores with
the range guard), the packed-row index / gather / unpack kernels (gam_pack.h) and the log-mel frontend (gam_frontend.h).

References, pinned by the CPU tests of this file: the stem is ``oracle.pre_encode`` run in fp64, the frontend an fp64 DFT-by-matmul
statement of ``oracle.log_mel``.  Bars: per case the kernel's maximum error against fp64 must stay below K times the
error of an fp32 torch run of the same operation on the same inputs, that error floored at one fp32 ulp of the output's largest magnitude.
Each matrix test ends with a coverage guard: the set of kernel forms / layouts / tile classes it launched must be the set it names."""
import contextlib
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from common import TOL_FEAT, TOL_FEAT_WEAK, load_case, logmel_err, make_engine, oracle_features, report, valid_mask
from gigaam_amd import synth
from oracle import gigaam_oracle as O

# the one-term mode's relative bar (tests/test_hip_fastmode.py)
TOL_GEMM_REL = 2e-3

# K of "kernel error < K x fp32-torch error": twice the largest kernel / fp32-torch ratio measured on the MI355X, rounded up, at most 8
# (DESIGN.md 4.22).  Measured with the planner's tiles: conv2d f32 3.92, f16x3 2.13; conv1d f32 2.25, f16x3 2.26; frontend 3.18 on the
# strong bands, 1.16 on the weak ones.
K_STEM = {("conv2d", "f32"): 8, ("conv2d", "f16x3"): 5, ("conv1d", "f32"): 5, ("conv1d", "f16x3"): 5}
# the forced plans (test_stem_under_forced_plans) against the fp32 run in the SAME order of summation (stem_ref_seq32): conv2d 3.31 at
# S = 1 and 4.10 at S = 2 (twice that is 8.2: the cap), conv1d 3.73 and 2.81
K_STEM_FORCED = {"conv2d": 8, "conv1d": 8}
K_FE_STRONG = 7
K_FE_WEAK = 3

STEM_T = [1, 2, 3, 4, 5, 7, 8, 9, 61, 62, 63, 64, 65, 66, 67, 68, 127, 129]
STEM_B = 4
# (d_model, F): both widths at the published F = 64; F = 40 (not a multiple of 32) and F = 50 (odd f1 = 25) at the small width
STEM_ENGINES = [(192, 64), (768, 64), (192, 40), (192, 50)]
# two-stage tile classes of gam_launch_gemm_sp
CLASSES2 = [(2, 2), (3, 2), (2, 4), (3, 4), (4, 4)]


def ulp32(x):
    """One fp32 ulp at magnitude x."""
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x > 0 else 2.0 ** -149


# ------------------------------------------------------------------------------------------------------------ references
def stem_cfg(stem, d_model, feat_in):
    cfg = synth.model_cfg("v2_ctc" if stem == "conv2d" else "v3_ctc", n_layers=1, d_model=d_model, n_heads=d_model // 48, feat_in=feat_in)
    cfg["preprocessor"]["features"] = feat_in          # gam_create wants n_mels == feat_in
    del cfg["head"], cfg["decoding"]                   # (the synthetic head assumes d_model = 768)
    return cfg


_SD = {}


def stem_weights(stem, d_model, feat_in):
    key = (stem, d_model, feat_in)
    if key not in _SD:
        cfg = stem_cfg(stem, d_model, feat_in)
        _SD[key] = (cfg, synth.make_state_dict(cfg, seed=5))
    return _SD[key]


def stem_ref(sd, ecfg, feat, lens, dtype):
    """oracle.pre_encode on feat [B, F, T] (don't-care frames may hold anything finite: the oracle masks them) in `dtype`:
    (tokens [B, T', D], enc_len)."""
    w = {k: v.to(dtype) for k, v in sd.items() if k.startswith("encoder.pre_encode.")}
    with torch.no_grad():
        return O.pre_encode(w, ecfg, feat.transpose(1, 2).to(dtype), lens)


def _split16(x):
    """x = hi + lo with hi = fp16(x), lo = fp16(x - hi), both returned as fp32 (gam_gemm_sp.h's operand split)."""
    hi = x.half().float()
    return hi, (x - hi).half().float()


def _seq_gemm32(a, w, S, three_term=False):
    """a [M, K] . w [N, K]^T in fp32 in the split-fp16 GEMM's order of summation: S slices of K; inside a slice one accumulator
    takes the 32-wide k-tiles one after the other; the slices are added in order (gam_splitk_reduce_kernel).
    three_term: the kernel's arithmetic as well -- operands split into fp16 hi + lo (the weights scaled by a power of two to a
    maximum in [128, 256) first: gam_api.hip make_split), three MFMAs per k-tile (hi.hi, hi_a.lo_w, lo_a.hi_w; the products of fp16
    values are exact in fp32), and each 16x16x32 MFMA modelled as FOUR rounded additions into the fp32 accumulator, one per lane
    group's eight products: twelve accumulator updates per k-tile.  (The grouping is a model of the matrix core, not a documented
    fact: with one update per MFMA the model errs 2.3 times less than the MI355X, with four it is within 7 % of it -- DESIGN.md 4.22.)"""
    nk = a.shape[1] // 32
    n = nk // S
    pairs, sc, step = [(a, w)], 1.0, 32
    if three_term:
        sc = 2.0 ** max(-24, min(24, math.floor(math.log2(256.0 / float(w.abs().max())))))
        (ah, al), (wh, wl) = _split16(a), _split16(w * sc)
        pairs, step = [(ah, wh), (ah, wl), (al, wh)], 8
    out = None
    for s in range(S):
        acc = torch.zeros(a.shape[0], w.shape[0])
        for k in range(s * n, (s + 1) * n):
            for (x, y) in pairs:
                for j in range(32 * k, 32 * (k + 1), step):
                    acc += x[:, j:j + step] @ y[:, j:j + step].t()     # (one rounded addition per element)
        acc = acc * (1.0 / sc)
        out = acc if out is None else out + acc
    return out


def stem_ref_seq32(sd, ecfg, feat, lens, S, three_term=False):
    """The stem in fp32 with both GEMMs summed in the kernel's order at split-K factor S (_seq_gemm32): the K axis laid out as
    gam_api.hip lays it out -- Conv2d #2: 32-channel block outermost, the nine taps inside it; the linear: frequency-major; conv1d:
    tap-major.  Conv2d #1 (nine products per output) is torch's.  The denominator of the forced-plan bars: an fp32 run whose order
    of summation is defined up to the 32 products of a k-tile, so it does not move with the CPU or its thread count as a library
    convolution's does."""
    p = "encoder.pre_encode."
    w = {k: v.float() for k, v in sd.items() if k.startswith(p)}
    T = feat.shape[2]
    l1 = (lens.clamp(0, T) + 1) // 2
    l2 = (l1 + 1) // 2
    feat = O._mask_time(feat.float(), lens)
    if ecfg["subsampling"] == "conv2d":
        x1 = F.relu(O._mask_time(F.conv2d(feat.transpose(1, 2).unsqueeze(1), w[p + "conv.0.weight"], w[p + "conv.0.bias"], stride=2, padding=1), l1))
        B, Cc, H, W = x1.shape
        H2, W2 = (H + 1) // 2, (W + 1) // 2
        xp = F.pad(x1, (1, 1, 1, 1))
        taps = torch.stack([xp[:, :, kh:kh + 2 * H2 - 1:2, kw:kw + 2 * W2 - 1:2] for kh in range(3) for kw in range(3)], 1)   # [B, 9, C, H2, W2]
        a = taps.permute(0, 3, 4, 2, 1).reshape(B * H2 * W2, Cc // 32, 32, 9).transpose(2, 3).reshape(B * H2 * W2, 9 * Cc)
        w2 = w[p + "conv.2.weight"].reshape(Cc, Cc // 32, 32, 9).transpose(2, 3).reshape(Cc, 9 * Cc)
        x2 = (_seq_gemm32(a, w2, S, three_term) + w[p + "conv.2.bias"]).reshape(B, H2, W2, Cc)
        x2 = F.relu(x2.masked_fill((torch.arange(H2)[None, :] >= l2[:, None])[:, :, None, None], 0.0))
        wl = w[p + "out.weight"].reshape(-1, Cc, W2).transpose(1, 2).reshape(-1, W2 * Cc)
        return (_seq_gemm32(x2.reshape(B * H2, W2 * Cc), wl, S, three_term) + w[p + "out.bias"]).reshape(B, H2, -1)
    x = feat
    for s, ln in ((0, l1), (2, l2)):
        B, Cin, Tin = x.shape
        To = (Tin + 1) // 2
        xp = F.pad(x, (2, 2))
        a = torch.stack([xp[:, :, k:k + 2 * To - 1:2] for k in range(5)], 1).permute(0, 3, 1, 2).reshape(B * To, 5 * Cin)   # [rows, tap, channel]
        wk = w[p + "conv.%d.weight" % s].permute(0, 2, 1).reshape(-1, 5 * Cin)
        y = (_seq_gemm32(a, wk, S, three_term) + w[p + "conv.%d.bias" % s]).reshape(B, To, -1)
        y = F.relu(y.masked_fill((torch.arange(To)[None, :] >= ln[:, None])[:, :, None], 0.0))
        x = y.transpose(1, 2)
    return x.transpose(1, 2)


def stem_lens(i, T):
    pattern = [T, 0, 1, T - 1, (T + 1) // 2, max(1, T - 3), T + 5]
    return torch.tensor([pattern[(i + b) % len(pattern)] for b in range(STEM_B)], dtype=torch.int64)


def zero_fill(feat, lens, fill=None):
    """feat with the frames t >= lens[b] set to zero, or (fill) to NaN / +inf / -inf in turn."""
    out = feat.clone()
    T = feat.shape[2]
    bad = torch.tensor([float("nan"), float("inf"), float("-inf")])
    for b, n in enumerate(lens.tolist()):
        n = min(max(n, 0), T)
        out[b, :, n:] = bad[(torch.arange(n, T) + b) % 3] if fill else 0.0
    return out


_REF = {}


def stem_case(stem, d_model, feat_in, i, T):
    """One case of the stem matrix, computed once and shared by the modes: zero-filled features, lengths, the fp64 tokens, the
    oracle's enc_len, the fp32 run's error on the valid frames and the valid-frame mask."""
    key = (stem, d_model, feat_in, T)
    if key not in _REF:
        cfg, sd = stem_weights(stem, d_model, feat_in)
        g = torch.Generator().manual_seed(1000 * T + feat_in + d_model)
        lens = stem_lens(i, T)
        feat = zero_fill(2.0 * torch.randn(STEM_B, feat_in, T, generator=g), lens)
        ref, elen = stem_ref(sd, cfg["encoder"], feat, lens, torch.float64)
        r32, elen32 = stem_ref(sd, cfg["encoder"], feat, lens, torch.float32)
        assert elen.tolist() == elen32.tolist()
        vm = valid_mask(ref.shape[1], elen)[:, :, None]
        e32 = float(((r32.double() - ref) * vm).abs().max())
        _REF[key] = (feat, lens, ref, elen, e32, vm)
    return _REF[key]


def dft_logmel(wav, pre_cfg, window, fb, dtype):
    """oracle.log_mel as a DFT-by-matmul in `dtype` (the kernel's algorithm, not an FFT): reflect padding for center = True, frames of
    n_fft samples every hop, the window folded into a cos / sin basis built in fp64, |X|^2, the filterbank, log(clamp(., 1e-9, 1e9))."""
    fp = O.frontend_params(pre_cfg)
    n, hop = fp["n_fft"], fp["hop_length"]
    x = wav.to(dtype)
    if fp["center"]:
        x = F.pad(x[:, None, :], (n // 2, n // 2), mode="reflect")[:, 0]
    frames = x.unfold(1, n, hop)                                           # [B, Tf, n]
    k = torch.arange(n, dtype=torch.int64)
    ang = 2.0 * math.pi * ((k[:, None] * torch.arange(n // 2 + 1)[None, :]) % n).double() / n
    wd = window.double()[:, None]
    re = frames @ (torch.cos(ang) * wd).to(dtype)
    im = frames @ (torch.sin(ang) * wd).to(dtype)
    mel = (re * re + im * im) @ fb.to(dtype)                               # [B, Tf, n_mels]
    lo, hi = float(torch.tensor(1e-9, dtype=torch.float32)), float(torch.tensor(1e9, dtype=torch.float32))
    return torch.log(mel.clamp(lo, hi)).transpose(1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------- CPU: the pins
@pytest.mark.parametrize("case", ["v2_ctc_l2", "v3_ctc_l2"])
def test_stem_reference_is_the_oracle_and_the_goldens(case):
    """The fp64 run of oracle.pre_encode against its own fp32 run and against the committed pre_encode goldens, both at the goldens'
    existing tolerance (tests/test_oracle_golden.py: 2e-5)."""
    ck, wav, wlen, gold = load_case(case)
    feat, flen = oracle_features(ck, wav, wlen)
    ref, elen = stem_ref(ck["state_dict"], ck["cfg"]["encoder"], feat, flen, torch.float64)
    r32, _ = stem_ref(ck["state_dict"], ck["cfg"]["encoder"], feat, flen, torch.float32)
    assert elen.tolist() == gold["enc_len"].tolist()
    vm = valid_mask(ref.shape[1], elen)[:, :, None]
    assert float(((ref - r32.double()) * vm).abs().max()) < 2e-5
    assert float(((ref - torch.from_numpy(gold["pre_encode"]).double()) * vm).abs().max()) < 2e-5


# kernel error against fp64 at the forced-plan shape (T = 67, B = 4, d_model = 768, f16x3) as measured on the MI355X, by forced S;
# the same for all five tile classes (they are bit-identical at S = 1)
FORCED_ERR_MI355X = {("conv2d", 1): 1.2266e-05, ("conv2d", 2): 8.0796e-06, ("conv1d", 1): 7.5715e-06, ("conv1d", 2): 4.6022e-06}


@pytest.mark.parametrize("stem", ["conv2d", "conv1d"])
def test_stem_ordered_fp32_run_and_accumulation_model(stem):
    """stem_ref_seq32 (the denominator of the forced-plan bars) computes oracle.pre_encode: within the goldens' 2e-5 of the fp64 run at
    the forced-plan shape, for the slice counts used there and for a planner-like 8 / 5; the K layout it transcribes is thereby checked
    too (a permuted axis is no rounding error).  And the explanation of the forced-plan errors is pinned: the three-term model -- split
    operands, twelve rounded accumulator updates per k-tile -- lands within 10 % of what the MI355X measured at S = 1, i.e. the error of
    a forced plan is the length of one fp32 accumulator's walk along K and nothing else.  Errors go to $GAM_TEST_REPORT."""
    T = 67
    feat, lens, ref, _, e32, vm = stem_case(stem, 768, 64, STEM_T.index(T), T)
    cfg, sd = stem_weights(stem, 768, 64)
    errs = {}
    for S in (1, 2, 8 if stem == "conv2d" else 5):   # (conv1d stage 1 has ten k-tiles)
        out = stem_ref_seq32(sd, cfg["encoder"], feat, lens, S)
        assert tuple(out.shape) == tuple(ref.shape)
        errs[S] = float(((out.double() - ref) * vm).abs().max())
        assert errs[S] < 2e-5, (stem, S, errs[S])
    nt = torch.get_num_threads()
    torch.set_num_threads(1)     # thousands of small matmuls: threads only cost here (the result does not depend on them)
    try:
        model = float(((stem_ref_seq32(sd, cfg["encoder"], feat, lens, 1, three_term=True).double() - ref) * vm).abs().max())
    finally:
        torch.set_num_threads(nt)
    report("stem_ordered_fp32", stem=stem, err_by_slices=errs, err_fp32_torch=e32, err_three_term_model_s1=model)
    assert 0.9 < FORCED_ERR_MI355X[(stem, 1)] / model < 1.1, (stem, model)


def test_stem_reference_lengths_and_masking():
    """What the matrix relies on: the oracle never reads a frame behind feat_len (NaN there changes nothing), a feat_len above T is
    all of T, and enc_len follows the two halvings of the RAW length."""
    cfg, sd = stem_weights("conv1d", 192, 64)
    T = 9
    lens = torch.tensor([9, 0, 4, 14], dtype=torch.int64)
    g = torch.Generator().manual_seed(1)
    feat = 2.0 * torch.randn(4, 64, T, generator=g)
    a, elen = stem_ref(sd, cfg["encoder"], zero_fill(feat, lens), lens, torch.float64)
    b, _ = stem_ref(sd, cfg["encoder"], zero_fill(feat, lens, fill=True), lens, torch.float64)
    assert torch.equal(a, b)
    assert elen.tolist() == [3, 0, 1, 4] == [(((n + 1) // 2) + 1) // 2 for n in lens.tolist()]
    full, _ = stem_ref(sd, cfg["encoder"], feat, torch.full((4,), T), torch.float64)
    assert torch.equal(a[3], full[3])


@pytest.mark.parametrize("case", ["v2_ctc_l2", "v3_ctc_l2"])
def test_frontend_reference_is_the_oracle(case):
    """The fp64 DFT-by-matmul against oracle.log_mel (fp32, torch.stft) on a golden case, within the frontend's existing bars; its fp32
    run (the denominator of the GPU bars) within the same bars."""
    ck, wav, wlen, _ = load_case(case)
    sd, pre = ck["state_dict"], ck["cfg"]["preprocessor"]
    win, fb = sd["preprocessor.featurizer.0.spectrogram.window"], sd["preprocessor.featurizer.0.mel_scale.fb"]
    feat_o, flen_o = oracle_features(ck, wav, wlen)
    ref = dft_logmel(wav, pre, win, fb, torch.float64)
    assert ref.shape == feat_o.shape
    fm = valid_mask(ref.shape[2], flen_o)
    for got in (feat_o.double(), dft_logmel(wav, pre, win, fb, torch.float32).double()):
        e_s, e_w = logmel_err(got, ref, fm)
        assert e_s < TOL_FEAT and e_w < TOL_FEAT_WEAK, (e_s, e_w)


# ------------------------------------------------------------------------------------------------------------ GPU helpers
def _lib():
    from gigaam_amd import _lib as L
    return L.load_library()


def plan_ex(m, n, k):
    mt, nw, s, ns = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert _lib().gam_plan_sp_ex(m, n, k, 256, C.byref(mt), C.byref(nw), C.byref(s), C.byref(ns)) == 0
    return mt.value, nw.value, s.value, ns.value


@contextlib.contextmanager
def forced(mt, nw, s, ns):
    lib = _lib()
    try:
        assert lib.gam_tune_sp(mt, nw, s) == 0 and lib.gam_tune_sp_stages(ns) == 0
        yield
    finally:
        lib.gam_tune_sp(0, 0, 0)
        lib.gam_tune_sp_stages(0)


_ENG = {}


def stem_engine(stem, d_model, feat_in, mode):
    key = (stem, d_model, feat_in)
    if key not in _ENG:
        cfg, sd = stem_weights(stem, d_model, feat_in)
        _ENG[key] = make_engine(cfg, sd, mode, head=False)
    _ENG[key].set_gemm_mode(mode)
    return _ENG[key]


def stem_run(eng, feat, lens, host_lengths=None):
    """(tokens [B, T', D], enc_len, encoded [B, D, T']) of the stem alone, on the CPU."""
    enc, elen, tok = eng.encode(feat.cuda(), lens.cuda(), n_layers_run=0, want_tokens=True, host_lengths=host_lengths)
    return tok.cpu(), elen.cpu(), enc.cpu()


def stem_forms(stem, mode, feat_in):
    """The kernel form encode_impl launches in front of the stem GEMMs (transcribed from gam_api.hip): the image format of
    gam_conv2d1_kernel<FMT> follows the mode (d_model % 64 == 0 always holds), gam_feat_to_rows_kernel<1> needs a split mode and F % 32 == 0.
    The coverage guards built on this follow the TEST's lists of modes and engines through this transcription, not the launcher: they
    notice a case dropped from the matrix, not a launcher that picks another instantiation -- that shows as a failed comparison or not at all."""
    if stem == "conv2d":
        return "conv2d1_kernel<%d>" % {"f32": 0, "f16x3": 1, "f16": 2}[mode]
    return "feat_to_rows<%d>" % (1 if mode != "f32" and feat_in % 32 == 0 else 0)


# ---------------------------------------------------------------------------------------------------------- stem matrix
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f16x3", "f32", "f16"])
@pytest.mark.parametrize("stem", ["conv2d", "conv1d"])
def test_stem_matrix(stem, mode):
    """Every T of STEM_T x B = 4 rotating lengths (0, 1, T - 1, T + 5, ..) x every engine of STEM_ENGINES: enc_len is the oracle's, every
    valid token frame is within the bar of fp64, and in every second case NaN / +-inf in the don't-care frames change no valid bit and
    leave the whole output finite.

    Refused rather than computed: the conv1d stem with feat_in % 32 != 0 (F = 40, 50) -- its first GEMM has K = 5 F, no multiple of the
    32-wide k-tile of either GEMM kernel; gam_create accepts the configuration (the frontend of such a handle works) and gam_encode refuses
    with the GEMM's shape in the message.  The conv2d stem takes F = 40 and F = 50 (f1 = 25: the last tap column of a row is the next
    image row's zero border).
    One-term mode: the conv2d stem runs one-term (fastmode's relative bar, and measurably not the three-term result); the conv1d stem's two
    GEMMs read overlapping rows and stay three-term by design (gam_api.hip), so there f16 must equal f16x3 bit for bit."""
    from gigaam_amd.engine import GigaAMHipError
    launched, ratios = set(), {}
    for (d_model, feat_in) in STEM_ENGINES:
        eng = stem_engine(stem, d_model, feat_in, mode)
        if stem == "conv1d" and feat_in % 32 != 0:
            feat, lens = torch.zeros(2, feat_in, 8), torch.tensor([8, 5])
            with pytest.raises(GigaAMHipError, match=r"gemm launch \(M=\d+ N=%d K=%d\)" % (d_model, 5 * feat_in)):
                stem_run(eng, feat, lens)
            continue
        worst = 0.0
        for i, T in enumerate(STEM_T):
            feat, lens, ref, elen_o, e32, vm = stem_case(stem, d_model, feat_in, i, T)
            tok, elen, enc = stem_run(eng, feat, lens)
            assert elen.tolist() == elen_o.tolist(), (stem, mode, d_model, feat_in, T, lens.tolist())
            assert tuple(tok.shape) == tuple(ref.shape)
            err = float(((tok.double() - ref) * vm).abs().max())
            scale = float((ref * vm).abs().max())
            floor = max(e32, ulp32(scale))
            tag = (stem, mode, d_model, feat_in, T, lens.tolist())
            if mode == "f16":
                eng.set_gemm_mode("f16x3")
                tok3, _, _ = stem_run(eng, feat, lens)
                eng.set_gemm_mode("f16")
                err3 = float(((tok3.double() - ref) * vm).abs().max())
                report("stem_matrix", stem=stem, mode=mode, d_model=d_model, F=feat_in, T=T, err=err, err_f16x3=err3, scale=scale)
                if stem == "conv2d":
                    assert err < TOL_GEMM_REL * scale and err > 20 * err3, (tag, err, err3, scale)
                else:
                    assert torch.equal(tok, tok3), tag
            else:
                ratio = err / floor
                worst = max(worst, ratio)
                report("stem_matrix", stem=stem, mode=mode, d_model=d_model, F=feat_in, T=T, err=err, err_fp32_torch=e32, scale=scale, ratio=ratio)
                assert err < K_STEM[(stem, mode)] * floor, (tag, err, e32, floor, ratio)
            if i % 2 == 1:   # don't-care input
                tok_d, elen_d, enc_d = stem_run(eng, zero_fill(feat, lens, fill=True), lens)
                assert elen_d.tolist() == elen.tolist()
                assert bool(torch.isfinite(tok_d).all()) and bool(torch.isfinite(enc_d).all()), tag
                for b, n in enumerate(elen.clamp(max=tok.shape[1]).tolist()):
                    assert torch.equal(tok_d[b, :n], tok[b, :n]) and torch.equal(enc_d[b, :, :n], enc[b, :, :n]), (tag, b)
            launched.add(stem_forms(stem, mode, feat_in))
        ratios["%d/%d" % (d_model, feat_in)] = worst
        assert not eng.range_flag()
    report("stem_matrix_ratios", stem=stem, mode=mode, worst_ratio=ratios)
    assert launched == {stem_forms(stem, mode, 64)}, launched


def test_stem_forms_cover_every_instantiation():
    """The coverage guard over the whole matrix: the three modes x two stems of test_stem_matrix name all three gam_conv2d1_kernel and both
    gam_feat_to_rows_kernel instantiations (feat_to_rows<0> through the exact-fp32 mode: with F % 32 != 0 the conv1d stem is refused).
    Pure bookkeeping over stem_forms (see there): it guards the matrix's lists, it does not observe a launch."""
    got = {stem_forms(stem, mode, f) for stem in ("conv2d", "conv1d") for mode in ("f16x3", "f32", "f16") for (_, f) in STEM_ENGINES
           if not (stem == "conv1d" and f % 32)}
    assert got == {"conv2d1_kernel<0>", "conv2d1_kernel<1>", "conv2d1_kernel<2>", "feat_to_rows<0>", "feat_to_rows<1>"}


# ------------------------------------------------------------------------------------------------------------ packed rows
PACK_CASES = [(67, [67, 30, 1, 45], [67, 41, 9, 60]), (129, [129, 5, 64, 0], [129, 13, 72, 8])]


@pytest.mark.gpu
@pytest.mark.parametrize("stem", ["conv2d", "conv1d"])
def test_stem_packed_rows(stem, monkeypatch):
    """gam_pack_index / gam_gather_rows / gam_unpack_rows and the skip_pad tile drop of Conv2d #2, against the padded run of the same handle
    (which test_stem_matrix holds to fp64): host lengths equal to the device's, and an upper bound.  Lengths 1 and 64 -> 1 and 16 frames: an
    utterance that ends inside the first row tile and one that ends on a 16-frame tile edge."""
    from gigaam_amd.engine import GigaAMHipError
    monkeypatch.setenv("GAM_PACK", "2")            # read by gam_create: packed rows at any batch size
    cfg, sd = stem_weights(stem, 768, 64)
    eng = make_engine(cfg, sd, "f16x3", head=False)
    layouts = set()
    for mode in ("f16x3", "f32", "f16"):
        eng.set_gemm_mode(mode)
        for (T, dev, bound) in PACK_CASES:
            g = torch.Generator().manual_seed(T)
            lens = torch.tensor(dev, dtype=torch.int64)
            feat = zero_fill(2.0 * torch.randn(4, 64, T, generator=g), lens)
            l2 = [(((n + 1) // 2) + 1) // 2 for n in dev]
            tok_p, elen_p, enc_p = stem_run(eng, feat, lens)                       # no host lengths: padded rows
            rows, rows_pad = eng.last_encode_rows()
            assert rows == rows_pad
            layouts.add("padded")
            assert elen_p.tolist() == l2
            for host in (dev, bound):
                tok_k, elen_k, enc_k = stem_run(eng, feat, lens, host_lengths=host)
                rows, rows_pad2 = eng.last_encode_rows()
                assert rows_pad2 == rows_pad and rows == sum((((n + 1) // 2) + 1) // 2 for n in host) < rows_pad
                layouts.add("packed")
                assert elen_k.tolist() == l2
                for b, n in enumerate(l2):
                    assert torch.equal(tok_k[b, :n], tok_p[b, :n]) and torch.equal(enc_k[b, :, :n], enc_p[b, :, :n]), (stem, mode, T, host, b)
                    assert not bool(tok_k[b, n:].any()) and not bool(enc_k[b, :, n:].any()), (stem, mode, T, host, b)
                assert not eng.range_flag()
    # a device length above the host's: bit 1 of the flag word (HipEngine.range_flag turns it into an error)
    eng.set_gemm_mode("f16x3")
    T, dev, _ = PACK_CASES[0]
    feat = 2.0 * torch.randn(4, 64, T, generator=torch.Generator().manual_seed(3))
    short = [dev[0], dev[1] - 9, dev[2], dev[3]]
    stem_run(eng, feat, torch.tensor(dev, dtype=torch.int64), host_lengths=short)
    word = C.c_int(0)
    assert eng.lib.gam_range_flag(eng._h, C.byref(word), eng._stream()) == 0
    assert word.value & 2, word.value
    stem_run(eng, feat, torch.tensor(dev, dtype=torch.int64), host_lengths=short)
    with pytest.raises(GigaAMHipError, match="host length is shorter"):
        eng.range_flag()
    assert layouts == {"padded", "packed"}


# ----------------------------------------------------------------------------------------------------------- forced plans
def stem_gemm_shapes(stem, B, T, d_model=768, feat_in=64):
    """(M, N, K) of the stem's two GEMMs as encode_impl launches them (gam_api.hip, transcribed)."""
    t1 = (T + 1) // 2
    tv = (t1 + 1) // 2
    if stem == "conv2d":
        ta = max(tv + 1, (t1 + 3) // 2)
        f2 = ((feat_in + 1) // 2 + 1) // 2
        return [(B * ta * f2, d_model, 9 * d_model), (B * ta, d_model, f2 * d_model)]
    ta = max(tv, (t1 + 5) // 2)
    t1a = max(t1, (T + 5) // 2)
    return [(B * t1a, d_model, 5 * feat_in), (B * ta, d_model, 5 * d_model)]


@pytest.mark.gpu
@pytest.mark.parametrize("stem,mode", [("conv2d", "f16x3"), ("conv2d", "f16"), ("conv1d", "f16x3")])
def test_stem_under_forced_plans(stem, mode):
    """T = 67, B = 4, ragged, d_model = 768: every two-stage tile class forced at S = 1 (bit-identical among themselves) and at split-K 2,
    each against fp64.  Read from the launcher (gam_gemm_sp_plan / gam_api.hip gemm()): the implicit-GEMM (a_mode = 1),
    masked and remapped launches take the planner's (mt, nw, S) like any other, so a force on these is honoured -- confirmed per GEMM shape
    with gam_plan_sp_ex; the only force an a_mode = 1 launch does not take is three LDS stages (it degrades to two), which is why only the
    two-stage classes are named here.  (conv1d in the f16 mode is the f16x3 launch: test_stem_matrix.)
    The bar: with S forced, one accumulator per output walks K / S of both GEMMs, and the error follows that length, the same for every
    tile class (conv2d f16x3: 1.23e-5 at S = 1, 8.1e-6 at S = 2, at most 3.7e-6 with the planner's S = 6 / 8).  torch's convolution sums in
    an order of its own that moves with the CPU and its thread count, so the denominator here is the fp32 run in the forced order,
    stem_ref_seq32(S) -- the same function on the same inputs, pinned on the CPU -- floored at one ulp as everywhere: K_STEM_FORCED."""
    T, i = 67, STEM_T.index(67)
    eng = stem_engine(stem, 768, 64, mode)
    feat, lens, ref, elen_o, e32, vm = stem_case(stem, 768, 64, i, T)
    scale = float((ref * vm).abs().max())
    cfg, sd = stem_weights(stem, 768, 64)
    floor = {S: max(float(((stem_ref_seq32(sd, cfg["encoder"], feat, lens, S).double() - ref) * vm).abs().max()), ulp32(scale)) for S in (1, 2)}
    tok3, ratios = None, {}
    if mode == "f16":
        eng.set_gemm_mode("f16x3")
        tok3, _, _ = stem_run(eng, feat, lens)
        eng.set_gemm_mode("f16")
        err3 = float(((tok3.double() - ref) * vm).abs().max())
    launched, s1, errs = set(), None, {}
    for (mt, nw) in CLASSES2:
        for S in (1, 2):
            with forced(mt, nw, S, 2):
                for (m, n, k) in stem_gemm_shapes(stem, STEM_B, T):
                    kk = k // 2 if mode == "f16" else k
                    assert plan_ex(m, n, kk) == (mt, nw, S, 2), (stem, mode, m, n, k, mt, nw, S)
                tok, elen, _ = stem_run(eng, feat, lens)
            launched.add((mt, nw, S))
            assert elen.tolist() == elen_o.tolist()
            err = float(((tok.double() - ref) * vm).abs().max())
            errs["%dx%d S=%d" % (mt, nw, S)] = err
            if mode == "f16":
                assert err < TOL_GEMM_REL * scale and err > 20 * err3, (stem, mode, mt, nw, S, err, err3)
            else:
                ratios[S] = max(ratios.get(S, 0.0), err / floor[S])
                assert err < K_STEM_FORCED[stem] * floor[S], (stem, mode, mt, nw, S, err, floor[S])
            if S == 1:
                if s1 is None:
                    s1 = tok
                else:
                    assert torch.equal(tok, s1), ("S = 1 classes differ", stem, mode, mt, nw, float((tok - s1).abs().max()))
    assert not eng.range_flag()
    report("stem_forced_plans", stem=stem, mode=mode, err=errs, err_fp32_torch=e32, err_fp32_ordered=floor, ratio_by_slices=ratios,
           s1_classes_bit_identical=True)
    assert launched == {(mt, nw, S) for (mt, nw) in CLASSES2 for S in (1, 2)}


# ------------------------------------------------------------------------------------------------------------ range guard
def _guard_case(which, over):
    """(stem, cfg, unscaled weights, scaled weights, unscaled features, features, lens) whose guarded tensor `which` has its largest magnitude at 1.05 x (over) or 0.95 x 60000 while the
    stem computes the same function: the factor on the guarded tensor's producer is divided out of the weights that consume it (ReLU is
    positively homogeneous), so every OTHER stem tensor keeps its O(1) values."""
    stem = "conv2d" if which in ("image", "conv2_out") else "conv1d"
    cfg, sd0 = stem_weights(stem, 192, 64)
    sd = {k: v.clone() for k, v in sd0.items()}
    p = "encoder.pre_encode."
    g = torch.Generator().manual_seed(23)
    T = 37
    lens = torch.tensor([37, 20], dtype=torch.int64)
    feat = zero_fill(2.0 * torch.randn(2, 64, T, generator=g), lens)
    with torch.no_grad():
        if stem == "conv2d":
            x1 = F.relu(O._mask_time(F.conv2d(feat.transpose(1, 2).unsqueeze(1), sd[p + "conv.0.weight"], sd[p + "conv.0.bias"], stride=2, padding=1),
                                     (lens + 1) // 2))
            x2 = F.relu(O._mask_time(F.conv2d(x1, sd[p + "conv.2.weight"], sd[p + "conv.2.bias"], stride=2, padding=1), (lens + 3) // 4))
        else:
            x1 = F.relu(O._mask_time(F.conv1d(feat, sd[p + "conv.0.weight"], sd[p + "conv.0.bias"], stride=2, padding=2), (lens + 1) // 2))
            x2 = None
    target = 60000.0 * (1.05 if over else 0.95)
    feat0 = feat
    if which == "feat":
        s = target / float(feat.abs().max())
        feat = feat * s
        sd[p + "conv.0.weight"] /= s
    elif which in ("image", "conv1_out"):
        s = target / float(x1.max())
        sd[p + "conv.0.weight"] *= s
        sd[p + "conv.0.bias"] *= s
        sd[p + "conv.2.weight"] /= s
    else:
        s = target / float(x2.max())
        sd[p + "conv.2.weight"] *= s
        sd[p + "conv.2.bias"] *= s
        sd[p + "out.weight"] /= s
    return stem, cfg, sd0, sd, feat0, feat, lens


@pytest.mark.gpu
@pytest.mark.parametrize("over", [True, False])
@pytest.mark.parametrize("which", ["image", "conv2_out", "feat", "conv1_out"])
def test_stem_range_guard(which, over):
    """The four guarded stores of the stem -- the Conv2d #1 image, the Conv2d #2 output (c_guard), gam_feat_to_rows and the conv1d stage-1
    output (c_guard) -- each raised through that store alone (tests/test_hip_range.py holds none of them): 5 % above 60000 the handle's
    flag is set, 5 % below it stays clear, and below it the tokens are still those of the unscaled stem."""
    stem, cfg, sd0, sd, feat0, feat, lens = _guard_case(which, over)
    eng = make_engine(cfg, sd, "f16x3", head=False)
    tok, elen, _ = stem_run(eng, feat, lens)
    assert eng.range_flag() is over, (which, over)
    if not over:
        ref, elen_o = stem_ref(sd, cfg["encoder"], feat, lens, torch.float64)     # the rescaled stem itself ...
        r32, _ = stem_ref(sd, cfg["encoder"], feat, lens, torch.float32)
        ref0, _ = stem_ref(sd0, cfg["encoder"], feat0, lens, torch.float64)       # ... which is the unscaled one up to the rounding of its weights
        vm = valid_mask(ref.shape[1], elen_o)[:, :, None]
        err, e32 = float(((tok.double() - ref) * vm).abs().max()), float(((r32.double() - ref) * vm).abs().max())
        assert elen.tolist() == elen_o.tolist()
        assert float(((ref - ref0) * vm).abs().max()) < 2e-5
        assert err < K_STEM[(stem, "f16x3")] * max(e32, ulp32(float((ref * vm).abs().max()))), (which, err, e32)
    eng.set_gemm_mode("f32")     # the exact mode has no range limit: no flag either way
    stem_run(eng, feat, lens)
    assert eng.range_flag() is False


# --------------------------------------------------------------------------------------------------------------- frontend
FE_TF = [1, 2, 63, 64, 65, 128, 129]
SENT = 12345.0


def _fe_engine(name):
    from gigaam_amd.engine import HipEngine, build_config
    cfg = synth.model_cfg(name)
    sd = synth.make_state_dict({"preprocessor": cfg["preprocessor"], "encoder": dict(cfg["encoder"], n_layers=0)}, seed=0)
    sd = {k: v for k, v in sd.items() if k.startswith("preprocessor.")}
    eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], None), sd, torch.device("cuda:0"))
    return eng, cfg["preprocessor"], sd["preprocessor.featurizer.0.spectrogram.window"], sd["preprocessor.featurizer.0.mel_scale.fb"]


def _fe_run(eng, wav, wlen):
    """gam_frontend on buffers of the test's own, with sentinels behind feat and behind feat_len: (feat [B, M, Tf], feat_len) on the CPU."""
    from gigaam_amd.engine import _ptr
    b, l = wav.shape
    tf, m = eng.feat_frames(l), eng.cfg.n_mels
    feat = torch.full((b * m * tf + 64,), SENT, dtype=torch.float32, device="cuda")
    flen = torch.full((b + 8,), -777, dtype=torch.int64, device="cuda")
    wav_d, wlen_d = wav.cuda().contiguous(), wlen.to(torch.int64).cuda()
    rc = eng.lib.gam_frontend(eng._h, _ptr(wav_d), _ptr(wlen_d), b, l, _ptr(feat), _ptr(flen), eng._stream())
    eng._check(rc, "gam_frontend")
    torch.cuda.synchronize()
    assert bool((feat[b * m * tf:] == SENT).all()) and bool((flen[b:] == -777).all()), "sentinel overwritten"
    return feat[:b * m * tf].view(b, m, tf).cpu(), flen[:b].cpu()


def _fe_signal(kind, b, l, n_fft, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "bin":       # exactly bin 37: bins 36 .. 38 only, every band away from them is clamped in fp64 and round-off in fp32
        t = torch.arange(l, dtype=torch.float64)
        return (0.5 * torch.sin(2.0 * math.pi * 37.0 * t / n_fft)).float()[None, :].repeat(b, 1)
    if kind == "tone":      # one sine, a third of a bin off bin 37 (on the bin a periodic Hann window leaks into bins 36 .. 38 only and every
        t = torch.arange(l, dtype=torch.float64)   # other band is clamped): the window's side lobes fill the bands down to -120 dB
        return (0.5 * torch.sin(2.0 * math.pi * 37.3 * t / n_fft)).float()[None, :].repeat(b, 1)
    return float(kind) * torch.randn(b, l, generator=g)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["v2_ctc", "v3_ctc"])
def test_frontend_matrix(name):
    """Both preprocessor configurations synth has (n_fft 400 / hop 160 / center, and 320 / 160 / no centring).  L chosen so that Tf is 1, 2,
    63, 64, 65, 128, 129 (the 64-frame block of gam_powmel_kernel on both sides; centred input cannot give Tf = 1: reflect padding needs
    L > n_fft / 2 >= hop), the shortest accepted input, B = 3 with wav_len around a hop boundary, noise at 1e-3 / 1 / 30 and a one-bin tone
    in turn; silence and overload at Tf = 65.  The WHOLE [B, n_mels, Tf] tensor is compared (kernel and reference both run on the padded
    batch), strong and weak bands apart (common.logmel_err); feat_len is the oracle's."""
    from gigaam_amd.engine import GigaAMHipError
    eng, pre, win, fb = _fe_engine(name)
    fp = O.frontend_params(pre)
    n, hop, center = fp["n_fft"], fp["hop_length"], fp["center"]
    kinds = ["0.001", "1.0", "30.0", "tone"]
    ls = [((tf - 1) * hop + 80 if center else n + (tf - 1) * hop + 80, tf) for tf in FE_TF if not (center and tf == 1)]
    if center:
        ls.append((n // 2 + 1, (n // 2 + 1) // hop + 1))        # the shortest input reflect padding accepts
    else:
        ls.append((n, 1))                                       # exactly one window
    seen_tf, worst = set(), {"strong": 0.0, "weak": 0.0}

    def compare(wav, wlen, tag, weak=True):
        feat, flen = _fe_run(eng, wav, wlen)
        ref = dft_logmel(wav, pre, win, fb, torch.float64)
        r32 = dft_logmel(wav, pre, win, fb, torch.float32).double()
        assert tuple(feat.shape) == tuple(ref.shape), (tag, feat.shape, ref.shape)
        want_len = O.feat_out_len(wlen, fp)
        assert flen.tolist() == want_len.tolist(), (tag, flen.tolist(), want_len.tolist())
        # gam_feat_frames sizes buffers: the same count, floored at no frames (the oracle's formula goes negative below one window)
        assert [eng.feat_frames(int(v)) for v in wlen.tolist()] == [max(0, int(v)) for v in want_len.tolist()], tag
        assert bool(torch.isfinite(feat).all()), tag
        e_s, e_w = logmel_err(feat.double(), ref)
        d_s, d_w = logmel_err(r32, ref)
        u = ulp32(float(ref.abs().max()))
        r_s, r_w = e_s / max(d_s, u), e_w / max(d_w, u)
        report("frontend_matrix", model=name, case=tag, err_strong=e_s, err_weak=e_w, fp32_strong=d_s, fp32_weak=d_w, ratio_strong=r_s, ratio_weak=r_w)
        assert e_s < K_FE_STRONG * max(d_s, u), (tag, e_s, d_s, r_s)
        if weak:
            assert e_w < K_FE_WEAK * max(d_w, u), (tag, e_w, d_w, r_w)
            worst["weak"] = max(worst["weak"], r_w)
        worst["strong"] = max(worst["strong"], r_s)
        return feat, ref

    for ci, (l, tf) in enumerate(ls):
        assert eng.feat_frames(l) == tf
        seen_tf.add(tf)
        k = max(1, (l // hop + 1) // 2)
        lens = [max(0, k * hop - 1), k * hop, min(l, k * hop + 1)]
        wav = _fe_signal(kinds[ci % 4], 3, l, n, seed=100 + ci)
        compare(wav, torch.tensor(lens), (kinds[ci % 4], l, tf, lens))
        if ci % 4 == 3:     # every L also sees noise at one amplitude
            compare(_fe_signal("1.0", 3, l, n, seed=200 + ci), torch.tensor(lens), ("1.0", l, tf, lens))
    if not center:
        l = n + 64 * hop + 80
        compare(_fe_signal("1.0", 3, l, n, seed=7), torch.tensor([n - 1, n, 0]), ("1.0", l, 65, [n - 1, n, 0]))
    # exact silence: every value is logf(1e-9f), bit for bit; overload: every band whose fp64 power is well past 1e9 is logf(1e9f)
    l = (64 * hop + 80) if center else (n + 64 * hop + 80)
    lo = torch.log(torch.tensor(1e-9, dtype=torch.float32).double()).float()
    hi = torch.log(torch.tensor(1e9, dtype=torch.float32).double()).float()
    feat, _ = compare(torch.zeros(3, l), torch.tensor([l, l // 2, 0]), ("silence", l, 65))
    assert bool((feat == lo).all()), (float(feat.min()), float(feat.max()), float(lo))
    # (a constant through a periodic Hann window has bins 0 and 1 only: every other band is an exact cancellation whose fp64 value is
    #  zero and whose fp32 value is round-off -- the weak bands of this one signal compare noise with noise and are left out)
    feat, ref = compare(torch.full((3, l), 1.0e4), torch.tensor([l, l // 2, 0]), ("overload", l, 65), weak=False)
    clamped = ref == ref.max()
    assert float(ref.max()) == pytest.approx(float(hi), abs=1e-6) and int(clamped.sum()) >= feat.shape[0] * feat.shape[2]
    assert bool((feat[clamped] == hi).all()), (float(feat[clamped].min()), float(hi))
    # a tone exactly on a bin: the almost-all-clamped frame; as for the constant, its weak bands are noise against noise and left out
    compare(_fe_signal("bin", 3, l, n, seed=0), torch.tensor([l, l // 2, 0]), ("bin", l, 65), weak=False)
    # refusals
    short = (n // 2) if center else (n - 1)
    with pytest.raises(GigaAMHipError, match="too short for reflect padding" if center else "yields no frames"):
        _fe_run(eng, torch.zeros(2, short), torch.tensor([short, short]))
    report("frontend_matrix_ratios", model=name, worst_ratio=worst)
    assert seen_tf == set(FE_TF) - ({1} if center else set()), seen_tf
