"""GPU: every instantiation of the split-fp16 GEMM (gam_gemm_sp.h) and of the fused attention (gam_attn16.h, gam_attn.h), each one
FORCED and compared with fp64 -- not only the plans the planner happens to pick at a few shapes.

GEMM: 8 tile classes (MT x NW / LDS stages) x {three-term, one-term} x {S = 1, split-K}; a force goes through gam_tune_sp /
gam_tune_sp_stages (process-wide: always reset) and is first confirmed with gam_plan_sp_ex, since a force the planner cannot take
degrades.  Attention: {rotary-style, rel-pos} x {64-, 128-query workgroups} x {three-term, one-term, exact fp32} through
gam_op_attention_ex.  Each test ends with a coverage guard: the set of instantiations it launched must be the full set."""
import contextlib
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from common import TOL_ENC, load_case, oracle_features, ragged_from_device, report, split_ragged, valid_mask

# the one-term mode's bars (tests/test_hip_fastmode.py)
TOL_GEMM_REL = 2e-3
TOL_ATT_F16 = 5e-3

# (MT, NW, LDS stages): every tile class gam_launch_gemm_sp instantiates
CLASSES = [(2, 2, 2), (2, 2, 3), (3, 2, 2), (3, 2, 3), (2, 4, 2), (2, 4, 3), (3, 4, 2), (4, 4, 2)]


def _lib():
    from gigaam_amd import _lib as L
    return L.load_library()


def _engine(mode):
    from gigaam_amd import synth
    from gigaam_amd.engine import HipEngine, build_config
    cfg = synth.model_cfg("v2_ctc")
    eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], None), {}, torch.device("cuda:0"))
    eng.set_gemm_mode(mode)
    return eng


def plan_ex(m, n, k):
    lib = _lib()
    mt, nw, s, ns = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert lib.gam_plan_sp_ex(m, n, k, 256, C.byref(mt), C.byref(nw), C.byref(s), C.byref(ns)) == 0
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


def _act(ref, act):
    return ref * torch.sigmoid(ref) if act == 1 else (ref.clamp_min(0) if act == 2 else ref)


def _operands(m, n, k, bias, seed, row_range=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(m, k, generator=g, device="cuda")
    if row_range:   # every row at its own power-of-two scale, 2^-20 (fp16 subnormals) .. 2^17 (beyond 65504)
        a = a * torch.exp2(torch.randint(-20, 18, (m, 1), generator=g, device="cuda").float())
    w = torch.randn(n, k, generator=g, device="cuda") / k ** 0.5
    b = torch.randn(n, generator=g, device="cuda") if bias else None
    return a, w, b


def _ref(a, w, b, act):
    r = a.double() @ w.double().t()
    if b is not None:
        r = r + b.double()
    return _act(r, act)


# (M, N, K, act, bias).  Every M and N leaves a partial last tile in every class (M % 64 != 0 or M = 1; N % 128 != 0 and N a multiple
# of 4 but not of 64 NW); K at 1 .. 3 k-tiles (at or below the stage count: the prologue fetches past the end) and deep K for split-K.
# One-term (f16): the kernel sees K / 2 -- K = 64 / 128 / 192 are 1 / 2 / 3 of its k-tiles (K = 32 or 96 would run three-term).
GEMM_SHAPES = {
    "f16x3": [(1, 772, 32, 0, True), (517, 1540, 96, 1, False), (1000, 1540, 64, 2, True), (2008, 772, 768, 2, True),
              (300, 200, 3072, 1, True), (129, 772, 768, 0, False)],
    "f16": [(1, 772, 64, 0, True), (517, 1540, 128, 1, False), (1000, 1540, 192, 2, True), (2008, 772, 768, 2, True),
            (300, 200, 3072, 1, True), (129, 772, 768, 0, False)],
}
RANGE_SHAPE = (517, 772, 768)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f16x3", "f16"])
def test_gemm_instantiation_matrix(mode):
    """Each tile class forced at every shape (S = 1) and at every split-K factor in {2, 3, 4, 8} the K allows, against fp64.
    At S = 1 all classes must give BIT-identical C: a lane's accumulator sums the same k-tiles in the same order (k16 step 0, then
    1; terms hi.hi, lo.hi, hi.lo) whatever MT and NW are -- the tile shape only decides WHICH outputs a lane owns -- and the
    epilogue is the same per element."""
    h16 = mode == "f16"
    eng = _engine(mode)
    launched = set()
    worst = {}
    for (m, n, k, act, bias) in GEMM_SHAPES[mode]:
        kk = k // 2 if h16 else k                   # the reduction length the planner and the kernel see
        nk = kk // 32
        a, w, b = _operands(m, n, k, bias, seed=m * 7 + n + k)
        ref = _ref(a, w, b, act)
        scale = max(1.0, float(ref.abs().max()))
        if h16:   # the three-term result of the same shape: the one-term kernels must be measurably NOT that
            eng.set_gemm_mode("f16x3")
            err3 = float((eng.op_gemm(a, w, b, act).double() - ref).abs().max()) / scale
            eng.set_gemm_mode("f16")
        s1 = None
        for (mt, nw, ns) in CLASSES:
            for S in [1] + [s for s in (2, 3, 4, 8) if nk % s == 0 and nk // s >= 4]:
                with forced(mt, nw, S, ns):
                    assert plan_ex(m, n, kk) == (mt, nw, S, ns), (mode, m, n, k, mt, nw, S, ns)
                    out = eng.op_gemm(a, w, b, act)
                torch.cuda.synchronize()
                launched.add((mt, nw, ns, S > 1, h16))
                err = float((out.double() - ref).abs().max()) / scale
                key = f"{mt}x{nw}/{ns}"
                worst[key] = max(worst.get(key, 0.0), err)
                if h16:
                    assert err < TOL_GEMM_REL and err > 20 * err3, (mode, m, n, k, act, mt, nw, ns, S, err, err3)
                else:
                    assert err < 2e-5, (mode, m, n, k, act, mt, nw, ns, S, err)
                if S == 1:
                    if s1 is None:
                        s1 = out
                    else:
                        assert torch.equal(out, s1), ("S = 1 classes differ", mode, m, n, k, mt, nw, ns,
                                                      float((out - s1).abs().max()))
    # rows of any magnitude, one shape per class: the per-row power-of-two scale keeps every row's bits; the range flag stays clear
    m, n, k = RANGE_SHAPE
    a, w, b = _operands(m, n, k, True, seed=17, row_range=True)
    ref = _ref(a, w, b, 0)
    rowmax = ref.abs().max(dim=1, keepdim=True).values.clamp(min=1.0)
    for (mt, nw, ns) in CLASSES:
        with forced(mt, nw, 1, ns):
            assert plan_ex(m, n, k // 2 if h16 else k) == (mt, nw, 1, ns)
            out = eng.op_gemm(a, w, b, 0)
        err = float(((out.double() - ref).abs() / rowmax).max())
        report("gemm_matrix_row_range", mode=mode, cls=f"{mt}x{nw}/{ns}", rel_err=err)
        assert bool(torch.isfinite(out).all()) and err < (TOL_GEMM_REL if h16 else 2e-5), (mode, mt, nw, ns, err)
    assert not eng.range_flag()
    report("gemm_matrix", mode=mode, s1_classes_bit_identical=True, worst_rel_err=worst)
    want = {(mt, nw, ns, sk, h16) for (mt, nw, ns) in CLASSES for sk in (False, True)}
    assert launched == want, sorted(want ^ launched)


def _f32_splitk(m, n, k):
    """The exact-fp32 kernel's split-K rule (gam_api.hip gemm()), transcribed: grids of at most half the chip in 128 x 128 tiles."""
    tiles, nk = math.ceil(m / 128) * math.ceil(n / 128), k // 32
    if tiles * 2 > 256 or nk < 4 or k % 32:      # (a partly filled last k-tile is never split)
        return 1
    s = min(16, 256 // tiles, nk // 2)
    while s > 1 and nk % s:
        s -= 1
    return s


@pytest.mark.gpu
def test_exact_fp32_kernel_splitk_rule_and_unaligned_n():
    """The exact-fp32 kernel in the f32 mode at shapes on both sides of its split-K rule (S = 2, 12, 16; S = 1 from too many tiles
    and from stepping nk % S down to 1), and in the f16x3 mode at the N % 4 != 0 shapes the LDS-DMA kernel cannot take.  The last
    four f32 shapes have K % 32 == 16 -- the pp and output GEMMs of RNN-T heads with pred_hidden / joint_hidden = 16, 48, 496, 336
    (tests/rnnt_cluster_cases.py): one k-tile that is half zeros, one and a half, fifteen and a half, ten and a half."""
    cases = {"f32": [(100, 100, 224, 1, True), (60, 300, 160, 2, False), (100, 100, 768, 0, True), (1000, 2000, 768, 2, True),
                     (1000, 2050, 768, 1, True), (129, 129, 3072, 0, True), (1, 772, 32, 1, True),
                     (7, 16, 16, 0, True), (61, 64, 48, 0, False), (200, 336, 496, 2, True), (40, 130, 336, 1, True)],
             "f16x3": [(257, 34, 768, 0, True), (300, 771, 96, 1, True), (1, 1, 32, 0, False), (16, 770, 3072, 2, True)]}
    assert {_f32_splitk(m, n, k) for (m, n, k, _, _) in cases["f32"]} == {1, 2, 12, 16}
    assert [_f32_splitk(m, n, k) for (m, n, k, _, _) in cases["f32"][:2]] == [1, 1]   # nk = 7, 5: S steps down to 1
    assert [k % 32 for (_, _, k, _, _) in cases["f32"][-4:]] == [16] * 4
    for mode, shapes in cases.items():
        eng = _engine(mode)
        for (m, n, k, act, bias) in shapes:
            a, w, b = _operands(m, n, k, bias, seed=m + 3 * n + k)
            ref = _ref(a, w, b, act)
            err = float((eng.op_gemm(a, w, b, act).double() - ref).abs().max())
            assert err < 2e-5 * max(1.0, float(ref.abs().max())), (mode, m, n, k, act, _f32_splitk(m, n, k), err)


# --------------------------------------------------------------------------------------------------------------- attention
DK = 48


def attention_ref(q, k, v, Tv, H, klen, pvec=None, pos_u=None, pos_v=None):
    """fp64 softmax attention of the first Tv queries of each utterance over keys < klen[b].  q, k, v [B, >= Tv, H*48].
    Rel-pos: pvec [2Tv-1, H*48] in the ORACLE's row order (row p = relative position (Tv-1) - p, oracle.rel_pos_emb) and the
    oracle's rel-shift (oracle.gigaam_oracle.self_attention), so the convention is the reference's, not the kernel's."""
    B = q.shape[0]
    qh = q[:, :Tv].double().reshape(B, Tv, H, DK)
    kh, vh = (x[:, :Tv].double().reshape(B, Tv, H, DK).transpose(1, 2) for x in (k, v))
    if pvec is None:
        scores = qh.transpose(1, 2) @ kh.transpose(-1, -2)
    else:
        p = pvec.double().reshape(1, 2 * Tv - 1, H, DK).transpose(1, 2)
        q_u = (qh + pos_u.double().reshape(H, DK)).transpose(1, 2)
        q_v = (qh + pos_v.double().reshape(H, DK)).transpose(1, 2)
        bd = q_v @ p.transpose(-2, -1)
        bb, hh, ql, pl = bd.shape
        bd = F.pad(bd, (1, 0)).view(bb, hh, -1, ql)[:, :, 1:].reshape(bb, hh, ql, pl)[..., :Tv]
        scores = q_u @ kh.transpose(-1, -2) + bd
    scores = scores / math.sqrt(DK)
    keymask = torch.arange(Tv, device=q.device)[None, :] >= klen.to(q.device)[:, None]
    scores = scores.masked_fill(keymask[:, None, None, :], float("-inf"))
    attn = torch.nan_to_num(torch.softmax(scores, -1), nan=0.0)
    return (attn @ vh).transpose(1, 2).reshape(B, Tv, H * DK)


def test_attention_reference_follows_the_oracle():
    """CPU: attention_ref's rel-pos path IS the oracle's self_attention (projections applied around it): position convention and
    rel-shift are pinned to the reference's code, not restated."""
    from oracle import gigaam_oracle as O
    g = torch.Generator().manual_seed(11)
    B, T, H = 2, 37, 2
    D = H * DK
    x = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    a = "layers.0.self_attn."
    sd = {a + f"linear_{nm}.weight": torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5 for nm in ("q", "k", "v", "out", "pos")}
    sd.update({a + f"linear_{nm}.bias": torch.randn(D, generator=g, dtype=torch.float64) for nm in ("q", "k", "v", "out")})
    sd[a + "pos_bias_u"] = torch.randn(H, DK, generator=g, dtype=torch.float64)
    sd[a + "pos_bias_v"] = torch.randn(H, DK, generator=g, dtype=torch.float64)
    pos = O.rel_pos_emb(T, D, 5000).double()
    lens = torch.tensor([T, 20])
    mask = torch.arange(T)[None, None, :] >= lens[:, None, None]
    want = O.self_attention(sd, "layers.0.", {"self_attention_model": "rel_pos", "n_heads": H}, x, pos, mask.expand(B, T, T))
    lin = lambda nm, t: F.linear(t, sd[a + f"linear_{nm}.weight"], sd.get(a + f"linear_{nm}.bias"))
    ctx = attention_ref(lin("q", x), lin("k", x), lin("v", x), T, H, lens, pvec=lin("pos", pos[0]),
                        pos_u=sd[a + "pos_bias_u"].reshape(-1), pos_v=sd[a + "pos_bias_v"].reshape(-1))
    got = lin("out", ctx)
    assert float(((got - want) * (torch.arange(T)[None, :, None] < lens[:, None, None])).abs().max()) < 1e-10


ATT_T = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257, 501]


def _att_cases():
    """(B, Tv, H, Ta, lens, packed, interleaved, rel).  Per T: a small grid (64-query workgroups) and one of >= 256 128-query
    workgroups (128-query kernel), each with and without rel-pos; Ta = Tv + 1 (padded queries beyond the keys), packed rows, the
    interleaved [rows, 3 D] q | k | v buffer and lens NULL rotate over the T list; lens hold 0, 1, 64 and T."""
    out = []
    for i, T in enumerate(ATT_T + [1030]):
        for big in (False, True):
            for rel in (False, True):
                if T == 1030 and not rel:   # (the long case is for the rel-pos window: 80 positions per tile, turned over ~13 times)
                    continue
                packed = i % 3 == 2
                ta = T + 1 if (i % 2 == 1 and not packed) else T
                H = 16 if big else 2
                B = max(2, math.ceil(256 / (H * math.ceil(ta / 128)))) if big else 2
                pattern = [T, 0, 1, 64, T - 1, max(1, T // 2)]
                lens = None if (i % 4 == 0 and not packed) else [pattern[(b + i) % len(pattern)] for b in range(B)]
                out.append((B, T, H, ta, lens, packed, (i + big) % 2 == 0, rel))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f16x3", "f16", "f32"])
def test_attention_variant_matrix(mode):
    """gam_op_attention_ex against fp64 on the valid query rows (t < klen), exact zeros for an utterance with klen = 0."""
    eng = _engine(mode)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    tol = TOL_ATT_F16 if mode == "f16" else 2e-5
    # q, k at std 2 (scores of std 4) where the bar is 2e-5; std 1 in the one-term mode, the inputs TOL_ATT_F16 was set on
    # (test_attention_one_term): at std 2 an fp16 emulation of the kernel's own arithmetic (q, k, P, V rounded once, fp32
    # sums) already errs by 6-7e-3 over 256 heads, and the kernel measured 6.2e-3
    qk_std = 1.0 if mode == "f16" else 2.0
    launched, worst = set(), {}
    for ci, (B, Tv, H, Ta, lens, packed, inter, rel) in enumerate(_att_cases()):
        g = torch.Generator(device="cuda").manual_seed(1000 + ci)
        D = H * DK
        q, k, v = (torch.randn(B, Ta, D, generator=g, device="cuda") * s for s in (qk_std, qk_std, 1.0))
        klen = torch.full((B,), Tv) if lens is None else torch.tensor(lens).clamp(max=Tv)
        pvec = pos_u = pos_v = pbuf = None
        if rel:
            pvec = torch.randn(2 * Tv - 1, D, generator=g, device="cuda")
            pos_u, pos_v = (0.5 * torch.randn(D, generator=g, device="cuda") for _ in range(2))
            # the kernel's pbuf is what gam_encode hands it: row n = relative position n - (Tv-1), i.e. the oracle's rows reversed
            pbuf = pvec.flip(0).contiguous()
        ref = attention_ref(q, k, v, Tv, H, klen.cuda(), pvec, pos_u, pos_v)
        if packed:
            rows = [x[b, :int(klen[b])] for x in (q, k, v) for b in range(B)]
            qkv = [torch.cat(rows[j * B:(j + 1) * B]) for j in range(3)]
            cu = torch.tensor([0] + torch.cumsum(klen, 0).tolist()[:-1], dtype=torch.int32)
        else:
            qkv = [x.reshape(B * Ta, D) for x in (q, k, v)]
            cu = None
        if inter:   # one [rows, 3 D] buffer, q | k | v column blocks (gam_encode's layout)
            buf = torch.cat(qkv, 1).contiguous()
            qkv = [buf[:, j * D:(j + 1) * D] for j in range(3)]
        lt = None if lens is None else torch.tensor(lens, dtype=torch.int32)
        got = eng.op_attention_ex(*qkv, B, Ta, Tv, H, lens=lt, cu=cu, pbuf=pbuf, pos_u=pos_u, pos_v=pos_v).double()
        err = 0.0
        for b in range(B):
            n = int(klen[b])
            r0 = int(cu[b]) if packed else b * Ta
            if n == 0 and not packed:
                assert bool((got[r0:r0 + Ta] == 0).all()), (mode, ci, b)
            if n:
                err = max(err, float((got[r0:r0 + n] - ref[b, :n]).abs().max()))
        if not packed:
            assert bool(torch.isfinite(got).all()), (mode, ci)
        nj = 2 if math.ceil(Ta / 128) * H * B >= ncu else 1
        variant = (rel, "f32") if mode == "f32" else (rel, 1 if mode == "f16" else 3, nj)
        launched.add(variant)
        worst[str(variant)] = max(worst.get(str(variant), 0.0), err)
        assert err < tol, (mode, B, Tv, H, Ta, lens, packed, inter, rel, err)
    report("attention_matrix", mode=mode, worst_err=worst, tol=tol)
    if mode == "f32":
        want = {(rel, "f32") for rel in (False, True)}
    else:
        want = {(rel, 1 if mode == "f16" else 3, nj) for rel in (False, True) for nj in (1, 2)}
    assert launched == want, sorted(map(str, want ^ launched))


# ------------------------------------------------------------------------------------------------- encoder under forced plans
ENC_PLANS = [(mt, nw, 1, ns) for (mt, nw, ns) in CLASSES] + [(2, 2, 4, 3), (3, 2, 4, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["v1_ctc_l2", "v2_ctc_l2", "v3_ctc_l2"])
def test_encoder_under_every_forced_plan(case):
    """The epilogues only the encoder reaches (residual with alpha = 0.5, sp32 C, the QKV operand switch, the implicit-GEMM stem,
    split-K reduced inside the LayerNorm) under every tile class at S = 1 and two three-stage classes at S = 4: the golden bar of
    test_encoder_matches_reference_golden, exact CTC ids, and bit-identical outputs across the S = 1 classes."""
    from gigaam_amd.engine import HipEngine, build_config
    ck, wav, wlen, gold = load_case(case)
    cfg = ck["cfg"]
    eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), ck["state_dict"], torch.device("cuda:0"))
    assert eng.gemm_mode == "f16x3"
    feat_o, flen_o = oracle_features(ck, wav, wlen)
    ids_ref = split_ragged(gold["ids"], gold["frames"], gold["counts"].tolist())
    vm = valid_mask(gold["encoded"].shape[2], gold["enc_len"])
    s1, errs = None, {}
    for plan in ENC_PLANS:
        with forced(*plan):
            enc, elen = eng.encode(feat_o, flen_o)
            dec = ragged_from_device(*eng.ctc_greedy(enc, elen))
            enc = enc.cpu()
        err = float(((enc - torch.from_numpy(gold["encoded"])) * vm[:, None, :]).abs().max())
        errs["%dx%d/%d S=%d" % (plan[0], plan[1], plan[3], plan[2])] = err
        assert elen.cpu().tolist() == gold["enc_len"].tolist()
        assert err < TOL_ENC, (case, plan, err)
        assert dec == ids_ref, (case, plan)
        if plan[2] == 1:
            if s1 is None:
                s1 = enc
            else:
                assert torch.equal(enc, s1), (case, plan, float((enc - s1).abs().max()))
    report("encoder_forced_plans", case=case, err=errs, tol=TOL_ENC)
