"""GPU: every launcher-reachable form of the LayerNorm family (gam_norm.h) and every instantiation of the fused conv-module
middle (gam_convmod.h), each one launched in isolation through gam_op_layernorm / gam_op_convmod and compared with an fp64 torch
reference of the same operation -- not behind two GEMMs and a residual at d_model = 768 only.

The bars are not invented: inside the test an fp32 torch implementation of the same operation runs on the same inputs, and the
kernel is held to K x that implementation's error against fp64 plus one fp32 ulp of the output scale (K_LN / K_CM below: measured
kernel / fp32-torch ratios).  The split-fp16 store formats are held to the bounds that follow from the formats.
Each matrix ends with a coverage guard: the set of instantiations implied by the launcher's rule (transcribed here) must be the
full set."""
import pytest
import torch
import torch.nn.functional as F

from common import report

EPS32 = 2.0 ** -23
# kernel error <= K x (fp32 torch error) + EPS32 x max|reference|; K is at most twice the largest kernel / fp32-torch ratio
# measured on the MI355X and never above 8 (every run reports the ratios; DESIGN.md 4.21 lists them).
K_LN = 8.0     # largest measured 5.06 (MODE 0, EARLY); every other form <= 2.33
K_CM = 4.0     # largest measured 2.45 (ln4_kernel<5>)

SENT = -7.25      # sentinel of every output buffer (exact in fp32 and fp16)
EXTRA = 3         # sentinel rows behind the rows a launch owns
ROPE_BASE = 5000


def _engine():
    from gigaam_amd import synth
    from gigaam_amd.engine import HipEngine, build_config
    cfg = synth.model_cfg("v2_ctc")
    return HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], None), {}, torch.device("cuda:0"))


def _err():
    from gigaam_amd._lib import GigaAMHipError
    return GigaAMHipError


# ------------------------------------------------------------------------------------------------------------ store formats
def decode_rows(buf, rows, d, fmt):
    """The first `rows` rows of a [*, d] fp32 buffer written in store format fmt (gam_common.h gam_store4), as fp64.
    0: fp32.  1 (sp32): every 32 columns are [hi x32 | lo x32] halfs in the 128 bytes of the fp32 values, value = hi + lo.
    2: dense fp16, row r at halfs r d .. r d + d - 1 of the buffer (the first half of the bytes)."""
    if fmt == 0:
        return buf[:rows].double()
    if fmt == 1:
        h = buf[:rows].view(torch.float16).view(rows, d // 32, 2, 32).double()
        return (h[:, :, 0] + h[:, :, 1]).reshape(rows, d)
    return buf.view(torch.float16).reshape(-1)[:rows * d].view(rows, d).double()


def untouched(buf, rows, d, fmt):
    """Everything behind the bytes the launch owns still holds the sentinel (bit compare)."""
    used = rows * d // 2 if fmt == 2 else rows * d
    words = buf.view(torch.int32).reshape(-1)[used:]
    return bool((words == torch.full_like(buf, SENT).view(torch.int32).reshape(-1)[used:]).all())


def format_ok(dec, want, fmt):
    """Bound of the format: sp32 keeps 22 bits (hi = fp16(x), lo = fp16(x - hi): 2^-11 of 2^-11, or half an fp16 subnormal step
    2^-25 once lo is subnormal); fp16 keeps 11 bits."""
    rel = 2.0 ** -22 if fmt == 1 else 2.0 ** -11
    return bool(((dec - want).abs() <= rel * want.abs() + 2.0 ** -25).all())


def sbuf(rows, d):
    return torch.full((rows + EXTRA, d), SENT, device="cuda")


# ------------------------------------------------------------------------------------------------------- LayerNorm references
def rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], dim=-1)


def rotary_ref(y, t, cos, sin, dk):
    """y [rows, d] -> per head of dk columns y cos[t] + rotate_half(y) sin[t]; cos / sin [R, dk] (oracle.rotary_cos_sin), t [rows]
    frame indices (already clamped to R - 1).  Runs in y's dtype."""
    rows, d = y.shape
    yh = y.reshape(rows, d // dk, dk)
    c, s = cos[t].to(y.dtype)[:, None, :], sin[t].to(y.dtype)[:, None, :]
    return (yh * c + rotate_half(yh) * s).reshape(rows, d)


def test_rotary_reference_follows_the_oracle():
    """CPU: rotary_ref IS the rotary branch of oracle.self_attention's pre-projection step (the projections and the attention core
    of the oracle applied around it), so the rotation convention is pinned to the reference's code, not restated."""
    from oracle import gigaam_oracle as O
    g = torch.Generator().manual_seed(5)
    B, T, H, dk = 2, 19, 3, 48
    D = H * dk
    x = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    a = "layers.0.self_attn."
    sd = {a + f"linear_{nm}.weight": torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5 for nm in ("q", "k", "v", "out")}
    sd.update({a + f"linear_{nm}.bias": torch.randn(D, generator=g, dtype=torch.float64) for nm in ("q", "k", "v", "out")})
    cos, sin = O.rotary_cos_sin(T, dk, ROPE_BASE)
    lens = torch.tensor([T, 11])
    mask = (torch.arange(T)[None, None, :] >= lens[:, None, None]).expand(B, T, T)
    want = O.self_attention(sd, "layers.0.", {"self_attention_model": "rotary", "n_heads": H}, x, (cos.double(), sin.double()), mask)
    lin = lambda nm, t: F.linear(t, sd[a + f"linear_{nm}.weight"], sd[a + f"linear_{nm}.bias"])
    t_idx = torch.arange(T).repeat(B)
    xr = rotary_ref(x.reshape(B * T, D), t_idx, cos[:, 0, 0, :].double(), sin[:, 0, 0, :].double(), dk).reshape(B, T, D)
    heads = lambda t: t.view(B, T, H, dk).transpose(1, 2)
    ctx = O._attention_core(heads(lin("q", xr)), heads(lin("k", xr)), heads(lin("v", x)), mask)
    got = lin("out", ctx.transpose(1, 2).reshape(B, T, D))
    assert float(((got - want) * (torch.arange(T)[None, :, None] < lens[:, None, None])).abs().max()) < 1e-10


def ln_inputs(rows, d, g, const_row):
    """randn sigma + mu with a per-row sigma in 2^-10 .. 2^10 and |mu| <= 16 sigma; row `const_row` (if any) is the constant 4:
    a power of two, so that the kernel's fp32 row sum 4 d and its mean 4 d / d are exact and the row normalises to exact zeros."""
    sigma = torch.exp2(torch.rand(rows, 1, generator=g, device="cuda") * 20 - 10)
    mu = sigma * (torch.rand(rows, 1, generator=g, device="cuda") * 32 - 16)
    x = torch.randn(rows, d, generator=g, device="cuda") * sigma + mu
    if const_row is not None:
        x[const_row] = 4.0
    return x, sigma


def ln_variant(mode, rows, part):
    """gam_launch_layernorm's rule, transcribed: (MODE, PART, EARLY).  The fused reduce always takes the EARLY form; a plain
    launch takes it up to GAM_LN_EARLY_ROWS = 1024 rows and the lean form above."""
    return (mode, 1, 1) if part else (mode, 0, 1 if rows <= 1024 else 0)


LN_ROWS = [1, 3, 4, 5, 37, 1024, 1025, 1030]
LN_D = [192, 256, 768, 960, 1024]
LN_NSPLIT = [1, 2, 3, 4, 5, 6, 8, 12, 16]


def _ln_cases(mode):
    """dicts of one mode: every rows x d plain (EARLY up to 1024 rows, lean above), every slice count of the fused reduce.  Store
    formats, the rotary options, the zero-bias constant row, in-place residuals and alpha rotate over the list."""
    out = []
    i = 0
    for rows in LN_ROWS:
        for d in LN_D:
            out.append(dict(rows=rows, d=d, ns=0, i=i))
            i += 1
    part_rows = [1, 3, 5, 37, 4]
    for j, ns in enumerate(LN_NSPLIT):
        for dd in sorted({LN_D[j % 5], 192}):      # every slice count also at d = 192: lanes past d read column 0
            out.append(dict(rows=part_rows[(j + (dd == 192)) % 5], d=dd, ns=ns, i=i))
            i += 1
    out.append(dict(rows=1030, d=768, ns=2, i=i))        # the fused reduce above GAM_LN_EARLY_ROWS (still the EARLY form)
    out.append(dict(rows=1025, d=192, ns=3, i=i + 1))
    for c in out:
        k = c["i"]
        c["alpha"] = (1.0, 0.5)[k % 2]
        c["fmt"] = ((1, 2), (2, 1), (0, 1), (1, 0), (2, 2), (1, 1))[k % 6] if c["d"] % 32 == 0 else (0, 0)
        c["zero_b"] = k % 3 == 0
        c["resid_inplace"] = k % 4 < 2
        dks = [q for q in (48, 64) if c["d"] % q == 0]
        c["dk"] = dks[k % len(dks)]
        c["row_t"] = k % 2 == 1
        c["clamp"] = k % 5 == 2
    return out


def _ln_run(eng, mode, c, fails, ratios):
    rows, d, ns = c["rows"], c["d"], c["ns"]
    tag = (mode, rows, d, ns, c["i"])
    g = torch.Generator(device="cuda").manual_seed(100000 * mode + 17 * c["i"] + rows + d)
    const_row = rows // 2 if c["zero_b"] else None
    x, sigma = ln_inputs(rows, d, g, const_row)
    rnd = lambda *shape: torch.randn(*shape, generator=g, device="cuda")
    w1, w2 = rnd(d), rnd(d)
    b1, b2 = (torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")) if c["zero_b"] else (rnd(d), rnd(d))
    kw = dict(w2=w2, b2=b2) if mode == 2 else {}
    var = ln_variant(mode, rows, ns > 0)
    key = "%d/%s" % (mode, "part" if var[1] else ("early" if var[2] else "lean"))

    # ---- the row the LayerNorm sees: x, or the fused reduce's resid + alpha (sum of slices + bias)
    part = pbias = resid = None
    x64, x32 = x.double(), x
    if ns:
        part = rnd(ns, rows, d) * sigma
        if const_row is not None:   # the constant row stays the constant 4: zero slices, zero bias, residual 4
            part[:, const_row] = 0.0
        pbias = torch.zeros(d, device="cuda") if c["zero_b"] else rnd(d)
        resid = x
        x64 = resid.double() + c["alpha"] * (part.double().sum(0) + pbias.double())
        acc = torch.zeros(rows, d, device="cuda")
        for s in range(ns):
            acc = acc + part[s]
        x32 = (acc + pbias) * c["alpha"] + resid
    ln = lambda t, w, b: F.layer_norm(t, (d,), w.to(t.dtype), b.to(t.dtype), 1e-5)
    ref1, t1 = ln(x64, w1, b1), ln(x32, w1, b1)
    ref2 = t2 = None
    rope = {}
    if mode == 1:
        from oracle import gigaam_oracle as O
        dk = c["dk"]
        R = 7 if c["clamp"] else 64
        cos, sin = (t[:, 0, 0, :].cuda() for t in O.rotary_cos_sin(R, dk, ROPE_BASE))
        if c["row_t"]:   # packed rows: an explicit, non-monotone frame index per row (beyond the table in the clamp case)
            row_t = torch.randint(0, 2 * R if c["clamp"] else R, (rows,), generator=g, device="cuda", dtype=torch.int32)
            t_idx = row_t.long()
            rope = dict(row_t=row_t)
        else:            # padded rows: row % ta (ta beyond the table in the clamp case)
            ta = 37
            t_idx = torch.arange(rows, device="cuda") % ta
            rope = dict(ta=ta)
        rope.update(rcos=cos[:, :dk // 2].contiguous(), rsin=sin[:, :dk // 2].contiguous(), dk=dk)
        t_idx = t_idx.clamp(max=R - 1)
        ref2, t2 = rotary_ref(ref1, t_idx, cos, sin, dk), rotary_ref(t1, t_idx, cos, sin, dk)
    elif mode == 2:
        ref2, t2 = ln(ref1, w2, b2), ln(t1, w2, b2)

    def launch(fmt, with_rs):
        """One launch on fresh sentinel buffers -> (out1 buffer, out2 buffer, rs buffer, residual-row buffer)."""
        xb = sbuf(rows, d)
        o2 = sbuf(rows, d) if mode else None
        rs = torch.full((rows + EXTRA,), SENT, device="cuda") if with_rs else None
        pk = {}
        if ns:
            # xstore == x as in the encoder; the residual is that same buffer (read, then overwritten) or a separate tensor
            if c["resid_inplace"]:
                xb[:rows] = resid
            pk = dict(part=part, nsplit=ns, pbias=pbias, presid=xb if c["resid_inplace"] else resid.contiguous(), palpha=c["alpha"],
                      xstore=xb)
        else:
            xb[:rows] = x
        o1 = xb if mode == 2 else sbuf(rows, d)     # MODE 2: out1 == x in place, as the encoder's norm_out
        eng.op_layernorm(mode, rows, d, xb, o1, w1, b1, out2=o2, split1=fmt[0], split2=fmt[1], rs=rs, **kw, **rope, **pk)
        return o1, o2, rs, xb

    def acc(what, got, ref, t32, per_row=False):
        ek, et = (got - ref).abs(), (t32.double() - ref).abs()
        scale = ref.abs().max()
        if per_row:   # the residual row keeps the input's per-row magnitude: errors relative to each row's largest element
            n = ref.abs().amax(1, keepdim=True).clamp_min(1e-30)
            ek, et, scale = ek / n, et / n, torch.ones(())
        ek, et, fl = float(ek.max()), float(et.max()), EPS32 * float(scale)
        if max(et, fl) > 0:     # (an all-zero reference -- a lone constant row -- has no ratio)
            ratios[key] = max(ratios.get(key, 0.0), ek / max(et, fl))
        if not ek <= K_LN * et + fl:
            fails.append((tag, what, "err %.3g > %g x %.3g + %.3g" % (ek, K_LN, et, fl)))

    # ---- 1. fp32 stores, no row scale: against fp64
    o1, o2, _, xb = launch((0, 0), False)
    base1 = o1[:rows].clone()
    base2 = o2[:rows].clone() if mode else None
    acc("out1", base1.double(), ref1, t1)
    if mode:
        acc("out2", base2.double(), ref2, t2)
    if ns and mode != 2:
        acc("stored row", xb[:rows].double(), x64, x32, per_row=True)
    if c["zero_b"]:
        zero = [base1[const_row]] + ([base2[const_row]] if mode else [])
        if not all(bool((z == 0).all()) for z in zero):
            fails.append((tag, "the constant row did not normalise to zeros"))
    for b_ in (o1, o2) if mode else (o1,):
        if not untouched(b_, rows, d, 0):
            fails.append((tag, "a format-0 launch wrote behind its rows"))

    # ---- 2. the row-scale contract, fp32 stores: rs a power of two, the scaled operand's row maximum in [128, 256), exact undo
    o1, o2, rs, _ = launch((0, 0), True)
    r = rs[:rows]
    scaled, unscaled_ok = (o2, torch.equal(o1[:rows], base1)) if mode == 2 else (o1, True)   # MODE 2: out1 is never scaled
    sbase = base2 if mode == 2 else base1
    mant, _ = torch.frexp(r.cpu())
    mx = scaled[:rows].abs().amax(1)
    nz = sbase.abs().amax(1) > 0
    ok = (bool((mant == 0.5).all()) and bool(torch.isfinite(r).all()) and bool(((mx >= 128) & (mx < 256))[nz].all()) and bool((r[~nz] == 1).all())
          and torch.equal(scaled[:rows] * r[:, None], sbase) and unscaled_ok and bool((rs[rows:] == SENT).all()))
    if mode == 1:   # one scale for the plain and the rotated copy
        ok = ok and torch.equal(o2[:rows] * r[:, None], base2)
    if c["zero_b"]:
        ok = ok and float(r[const_row]) == 1.0
    if not ok:
        fails.append((tag, "row-scale contract", float(mx.min()), float(mx.max())))

    # ---- 3. the split-fp16 store formats against the format-0 output of the same inputs (scaled where rs is given)
    fmt = c["fmt"] if mode else (c["fmt"][0], 0)
    if mode == 2:
        fmt = (0, fmt[1] or 1)      # out1 == x in place stays fp32 (a dense-fp16 row would land in another row's input bytes)
    if fmt != (0, 0):
        with_rs = c["i"] % 2 == 0
        o1, o2, rs, _ = launch(fmt, with_rs)
        s = (1.0 / rs[:rows].double())[:, None] if with_rs else 1.0
        s1 = 1.0 if mode == 2 else s
        if not format_ok(decode_rows(o1, rows, d, fmt[0]), base1.double() * s1, fmt[0]) or not untouched(o1, rows, d, fmt[0]):
            fails.append((tag, "out1 in format %d" % fmt[0]))
        if mode and (not format_ok(decode_rows(o2, rows, d, fmt[1]), base2.double() * s, fmt[1]) or not untouched(o2, rows, d, fmt[1])):
            fails.append((tag, "out2 in format %d" % fmt[1]))
    return var


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_layernorm_variant_matrix(mode):
    """gam_op_layernorm at every rows x d of the issue's lists in the plain forms and at every slice count of the fused reduce,
    against fp64 (K_LN x the fp32 torch error); row-scale contract, store formats and sentinels per case."""
    eng = _engine()
    fails, ratios, launched = [], {}, set()
    for c in _ln_cases(mode):
        launched.add(_ln_run(eng, mode, c, fails, ratios))
    torch.cuda.synchronize()
    report("layernorm_matrix", mode=mode, kernel_over_fp32_torch=ratios, K=K_LN, cases=len(_ln_cases(mode)))
    print("layernorm_matrix mode", mode, "kernel / fp32-torch error ratios", ratios)
    assert not fails, (len(fails), fails[:12])
    want = {(mode, p, e) for (p, e) in ((0, 1), (0, 0), (1, 1))}
    assert launched == want, sorted(want ^ launched)
    assert {c["ns"] for c in _ln_cases(mode)} == set(LN_NSPLIT) | {0}


def test_layernorm_matrix_covers_every_reachable_triple():
    """CPU: the three parametrised matrices together reach the 9 (MODE, PART, EARLY) triples gam_launch_layernorm can pick, which
    are the 9 instantiations the library holds (a PART launch never takes the lean form: DESIGN.md 4.21)."""
    got = {ln_variant(mode, c["rows"], c["ns"] > 0) for mode in (0, 1, 2) for c in _ln_cases(mode)}
    assert got == {(m, p, e) for m in (0, 1, 2) for (p, e) in ((0, 1), (0, 0), (1, 1))} and len(got) == 9


@pytest.mark.gpu
def test_layernorm_refusals_launch_nothing():
    """Shapes the launcher refuses come back as errors with a message; no output byte is written."""
    eng = _engine()
    Err = _err()
    g = torch.Generator(device="cuda").manual_seed(3)
    rnd = lambda *shape: torch.randn(*shape, generator=g, device="cuda")

    def refused(mode, rows, d, **kw):
        x, o1, o2 = rnd(rows, d), sbuf(rows, d), sbuf(rows, d)
        with pytest.raises(Err) as e:
            eng.op_layernorm(mode, rows, d, x, o1, rnd(d), rnd(d), out2=o2 if mode else None, **kw)
        torch.cuda.synchronize()
        assert "layernorm" in str(e.value), str(e.value)
        assert bool((o1 == SENT).all()) and bool((o2 == SENT).all()), (mode, rows, d)

    refused(0, 5, 1028)                                       # d > 1024
    refused(0, 5, 190)                                        # d % 4 != 0
    refused(0, 5, 100, split1=1)                              # a split output with d % 32 != 0
    refused(2, 5, 100, w2=rnd(100), b2=rnd(100), split2=2)
    cs = rnd(64, 6)
    refused(1, 5, 192, rcos=cs, rsin=cs, dk=12, ta=8)         # rotary with dk % 8 != 0
    refused(1, 5, 192, rcos=rnd(64, 40), rsin=rnd(64, 40), dk=80, ta=8)   # d % dk != 0
    part = rnd(2, 5, 192)
    refused(0, 5, 192, part=part, nsplit=2, presid=rnd(5, 192), xstore=sbuf(5, 192))      # part without bias
    refused(0, 5, 192, part=part, nsplit=2, pbias=rnd(192), xstore=sbuf(5, 192))          # part without residual
    refused(0, 5, 192, part=part, nsplit=0, pbias=rnd(192), presid=rnd(5, 192), xstore=sbuf(5, 192))


@pytest.mark.gpu
def test_layernorm_early_and_lean_forms_give_the_same_bits():
    """The EARLY form (parameters and rotary rows fetched before the row) and the lean form differ in WHEN they load, not in what
    they compute: the first 1000 rows of a 1030-row launch (lean) against a 1000-row launch (EARLY) of the same rows."""
    from oracle import gigaam_oracle as O
    eng = _engine()
    g = torch.Generator(device="cuda").manual_seed(9)
    same = {}
    for mode in (0, 1, 2):
        for d in (192, 768, 1024):
            x, _ = ln_inputs(1030, d, g, None)
            w1, b1, w2, b2 = (torch.randn(d, generator=g, device="cuda") for _ in range(4))
            kw = dict(w2=w2, b2=b2) if mode == 2 else {}
            if mode == 1:
                cos, sin = (t[:, 0, 0, :32].cuda().contiguous() for t in O.rotary_cos_sin(64, 64, ROPE_BASE))
                kw = dict(rcos=cos, rsin=sin, dk=64, ta=50)     # (1000 and 1030 rows see the same row % ta)
            outs = []
            for rows in (1030, 1000):
                o1, o2 = sbuf(rows, d), sbuf(rows, d)
                eng.op_layernorm(mode, rows, d, x[:rows].contiguous(), o1, w1, b1, out2=o2 if mode else None, **kw)
                outs.append((o1[:1000].clone(), o2[:1000].clone()))
            same["%d/%d" % (mode, d)] = torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    report("layernorm_early_vs_lean", bit_identical=same)
    print("layernorm EARLY vs lean bit-identical:", same)
    assert all(same.values()), same


# ------------------------------------------------------------------------------------------------------------- conv module
def convmod_middle(u, pad_mask, dw_w, dw_b, n_scale, n_shift, layer_norm):
    """The element-wise middle of oracle.conv_module between its two pointwise convs, in u's dtype and on u's device: u [B, T, 2d]
    (pointwise_conv1's output) -> GLU over channels -> masked_fill of padded frames -> depthwise conv (groups = d, zero padding) ->
    BatchNorm as the folded affine y n_scale + n_shift, or LayerNorm over channels -> SiLU; [B, T, d].  pad_mask [B, T] True =
    padded.  The depthwise conv is written as its sum over taps k = 0 .. ks - 1 (any device, any dtype, no vendor conv library);
    test_convmod_reference_follows_the_oracle pins the whole function to oracle.conv_module's F.conv1d(groups = d)."""
    d, ks = u.shape[-1] // 2, dw_w.shape[-1]
    T = u.shape[1]
    y = u.transpose(1, 2)
    y = y[:, :d] * torch.sigmoid(y[:, d:])
    y = y.masked_fill(pad_mask.unsqueeze(1), 0.0)
    yp = F.pad(y, ((ks - 1) // 2, (ks - 1) // 2))
    acc = torch.zeros_like(yp[:, :, :T])
    for k in range(ks):
        acc = acc + dw_w[None, :, k, None] * yp[:, :, k:k + T]
    y = acc + dw_b[None, :, None]
    if layer_norm:
        y = F.layer_norm(y.transpose(1, 2), (d,), n_scale, n_shift, 1e-5).transpose(1, 2)
    else:
        y = y * n_scale[None, :, None] + n_shift[None, :, None]
    return F.silu(y).transpose(1, 2)


@pytest.mark.parametrize("norm", ["batch_norm", "layer_norm"])
def test_convmod_reference_follows_the_oracle(norm):
    """CPU: convmod_middle with the oracle's pointwise convs around it IS oracle.conv_module, for both norm types; the BatchNorm
    scale / shift are folded from the running statistics exactly as gam_finalize folds them."""
    from oracle import gigaam_oracle as O
    g = torch.Generator().manual_seed(23)
    B, T, d, ks = 3, 29, 24, 9
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    c = "layers.0.conv."
    sd = {c + "pointwise_conv1.weight": rnd(2 * d, d, 1) / d ** 0.5, c + "pointwise_conv1.bias": rnd(2 * d),
          c + "depthwise_conv.weight": rnd(d, 1, ks) / ks ** 0.5, c + "depthwise_conv.bias": rnd(d),
          c + "batch_norm.weight": rnd(d), c + "batch_norm.bias": rnd(d),
          c + "batch_norm.running_mean": rnd(d), c + "batch_norm.running_var": torch.rand(d, generator=g, dtype=torch.float64) + 0.1,
          c + "pointwise_conv2.weight": rnd(d, d, 1) / d ** 0.5, c + "pointwise_conv2.bias": rnd(d)}
    x = rnd(B, T, d)
    lens = torch.tensor([T, 0, 13])
    pad = torch.arange(T)[None, :] >= lens[:, None]
    want = O.conv_module(sd, "layers.0.", {"conv_kernel_size": ks, "conv_norm_type": norm}, x, pad)
    u = F.conv1d(x.transpose(1, 2), sd[c + "pointwise_conv1.weight"], sd[c + "pointwise_conv1.bias"]).transpose(1, 2)
    if norm == "batch_norm":   # gam_finalize: inv = 1 / sqrt(var + 1e-5); scale = gamma inv; shift = beta - mean scale
        inv = 1.0 / torch.sqrt(sd[c + "batch_norm.running_var"] + 1e-5)
        scale = sd[c + "batch_norm.weight"] * inv
        shift = sd[c + "batch_norm.bias"] - sd[c + "batch_norm.running_mean"] * scale
    else:
        scale, shift = sd[c + "batch_norm.weight"], sd[c + "batch_norm.bias"]
    z = convmod_middle(u, pad, sd[c + "depthwise_conv.weight"].reshape(d, ks), sd[c + "depthwise_conv.bias"], scale, shift,
                       norm == "layer_norm")
    got = F.conv1d(z.transpose(1, 2), sd[c + "pointwise_conv2.weight"], sd[c + "pointwise_conv2.bias"]).transpose(1, 2)
    assert float((got - want).abs().max()) < 1e-10


def cm_variant(layer_norm, ks, d):
    """gam_launch_convmod's rule, transcribed: which kernel a (norm, ks, d) launch takes."""
    if not layer_norm:
        return ("bn", ks)
    if ks in (5, 9) and d % 4 == 0:
        return ("ln4", ks)
    return ("ln", ks)


CM_ALL = {("bn", 5), ("bn", 9), ("bn", 31), ("ln4", 5), ("ln4", 9), ("ln", 5), ("ln", 9), ("ln", 31)}
CM_TILE = {"bn": 128, "ln4": 16, "ln": 8}
# (layer_norm, ks, d): every instantiation at the issue's sizes
CM_SHAPES = ([(False, ks, d) for ks in (5, 9, 31) for d in (64, 768)] + [(True, ks, d) for ks in (5, 9) for d in (36, 192, 1024)]
             + [(True, 31, d) for d in (768, 1024)] + [(True, ks, d) for ks in (5, 9) for d in (50, 1023)])
CM_B = 4


def cm_formats(layer_norm, ks, d):
    """Store formats a shape is checked in besides fp32."""
    kind = cm_variant(layer_norm, ks, d)[0]
    if d % 32 != 0 or (kind == "ln" and d != 768):
        return []
    return [1] if kind == "ln" else [1, 2]


def cm_weights(layer_norm, ks, d, g):
    rnd = lambda *shape: torch.randn(*shape, generator=g, device="cuda")
    return dict(dw_w=rnd(d, ks) / ks ** 0.5, dw_b=0.1 * rnd(d), n_scale=rnd(d), n_shift=rnd(d))


def cm_launch(eng, u_rows, lens, cu, B, Ta, Tv, d, ks, layer_norm, w, fmt):
    """-> z buffer [rows + EXTRA, d], sentinel-filled before the launch."""
    z = sbuf(u_rows.shape[0], d)
    eng.op_convmod(u_rows.contiguous(), z, w["dw_w"], w["dw_b"], w["n_scale"], w["n_shift"], lens, B, Ta, Tv, d, ks, layer_norm,
                   z_split=fmt, cu=cu)
    return z


@pytest.mark.gpu
def test_convmod_variant_matrix():
    """gam_op_convmod: all instantiations, Tv straddling each kernel's frame tile, lens of Tv / 0 / 1 / below the halo, padded
    (Ta = Tv and Tv + 3, NaN / inf in every second case's don't-care frames) and packed rows, against the fp64 middle of
    oracle.conv_module on t < klen; store formats against the fp32 store; sentinels; the range flag stays clear."""
    eng = _engine()
    assert not eng.range_flag()
    fails, ratios, launched = [], {}, set()
    ci = 0
    for (layer_norm, ks, d) in CM_SHAPES:
        kind = cm_variant(layer_norm, ks, d)
        launched.add(kind)
        T, PAD = CM_TILE[kind[0]], (ks - 1) // 2
        g = torch.Generator(device="cuda").manual_seed(1000 * ks + d)
        w = cm_weights(layer_norm, ks, d, g)
        wargs = [w[k] for k in ("dw_w", "dw_b", "n_scale", "n_shift")]
        fmts = cm_formats(layer_norm, ks, d)
        junk = torch.tensor([float("nan"), float("inf"), float("-inf")], device="cuda")[torch.arange(2 * d, device="cuda") % 3]
        for Tv in sorted({1, PAD, PAD + 1, T - 1, T, T + 1, 2 * T + 1}):
            ci += 1
            pattern = [Tv, 0, 1, max(1, PAD - 1), Tv // 2, Tv - 1]
            lens = [pattern[(b + ci) % 6] for b in range(CM_B)] if ci % 3 else pattern[:CM_B]
            klen = [min(n, Tv) for n in lens]       # (lens above Tv reach the kernel as they are: it clamps them itself)
            uv = 2.0 * torch.randn(CM_B, Tv, 2 * d, generator=g, device="cuda")
            pad = torch.arange(Tv, device="cuda")[None, :] >= torch.tensor(klen, device="cuda")[:, None]
            # one reference per (shape, Tv, lens), shared by the layouts and formats: the valid frames, utterance-major
            ref = convmod_middle(uv.double(), pad, *(t.double() for t in wargs), layer_norm)[~pad]
            t32 = convmod_middle(uv, pad, *wargs, layer_norm)[~pad].double()
            et, scale = float((t32 - ref).abs().max()), float(ref.abs().max())
            fl = EPS32 * scale
            lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
            for li, layout in enumerate(("pad", "pad+3", "packed")):
                tag = (kind, d, Tv, lens, layout)
                if layout == "packed":     # cu = exclusive prefix of the lengths: rows of different utterances are adjacent
                    Ta, cu = Tv, [0]
                    for n in klen[:-1]:
                        cu.append(cu[-1] + n)
                    u_rows = uv[~pad]
                    cu_d = torch.tensor(cu, dtype=torch.int32, device="cuda")
                    vrows = torch.arange(sum(klen), device="cuda")
                else:
                    Ta, cu_d = Tv + (3 if layout == "pad+3" else 0), None
                    ub = torch.randn(CM_B, Ta, 2 * d, generator=g, device="cuda")
                    ub[:, :Tv] = uv
                    if (ci + li) % 2 == 0:    # don't-care frames (t >= klen) hold NaN / inf / -inf
                        for b in range(CM_B):
                            ub[b, klen[b]:] = junk
                    u_rows = ub.reshape(CM_B * Ta, 2 * d)
                    vrows = torch.cat([b * Ta + torch.arange(klen[b], device="cuda") for b in range(CM_B)])
                nrows = u_rows.shape[0]
                z0 = cm_launch(eng, u_rows, lens_d, cu_d, CM_B, Ta, Tv, d, ks, layer_norm, w, 0)
                got = z0[vrows].double()
                ek = float((got - ref).abs().max()) if bool(torch.isfinite(got).all()) else float("inf")
                rkey = "%s%d" % kind
                ratios[rkey] = max(ratios.get(rkey, 0.0), ek / max(et, fl))
                if not ek <= K_CM * et + fl:
                    fails.append((tag, "err %.3g > %g x %.3g + %.3g" % (ek, K_CM, et, fl)))
                if not untouched(z0, nrows, d, 0):
                    fails.append((tag, "wrote behind the launch's rows"))
                if fmts:
                    fmt = fmts[(ci + li) % len(fmts)]
                    zf = cm_launch(eng, u_rows, lens_d, cu_d, CM_B, Ta, Tv, d, ks, layer_norm, w, fmt)
                    if not format_ok(decode_rows(zf, nrows, d, fmt)[vrows], got, fmt):
                        fails.append((tag, "format %d" % fmt))
                    if not untouched(zf, nrows, d, fmt):
                        fails.append((tag, "format %d wrote behind the launch's rows" % fmt))
    flag = eng.range_flag()
    report("convmod_matrix", kernel_over_fp32_torch=ratios, K=K_CM, shape_tv_cases=ci)
    print("convmod_matrix kernel / fp32-torch error ratios", ratios)
    assert not fails, (len(fails), fails[:12])
    assert not flag, "the range flag was raised by O(1) outputs"
    assert launched == CM_ALL, sorted(CM_ALL ^ launched)


def _cm_flag_case(eng, layer_norm, ks, d, packed_dont_care):
    """-> (the handle's range flag after one sp32 launch, the same launch's outputs from an fp32 store).  Channel 0 is an identity through the
    depthwise conv (centre tap 1, bias 0, gate +40: sigmoid = 1).
    BatchNorm, valid: a = 1 at (utterance 0, frame 5) and 0 elsewhere, n_scale[0] = 1e5: one valid output of 1e5.
    BatchNorm, packed_dont_care: a = -1e5 at every valid frame, n_scale[0] = 1, n_shift[0] = 1e5: the valid outputs of channel 0
    are 0 and only frames >= klen -- no rows of the packed layout, never stored -- would hold SiLU(1e5).
    LayerNorm: the weight of channel 0 is 1e6 (the normalised channel is O(1) in every frame)."""
    B, Tv, klen = 2, 20, [20, 7]
    g = torch.Generator(device="cuda").manual_seed(77)
    w = cm_weights(layer_norm, ks, d, g)
    uv = torch.randn(B, Tv, 2 * d, generator=g, device="cuda")
    w["dw_w"][0] = 0.0
    w["dw_w"][0, (ks - 1) // 2] = 1.0
    w["dw_b"][0] = 0.0
    uv[:, :, d] = 40.0
    if layer_norm:
        w["n_scale"][0] = 1e6
    elif packed_dont_care:
        uv[:, :, 0] = -1e5
        w["n_scale"][0], w["n_shift"][0] = 1.0, 1e5
    else:
        uv[:, :, 0] = 0.0
        uv[0, 5, 0] = 1.0
        w["n_scale"][0], w["n_shift"][0] = 1e5, 0.0
    lens_d = torch.tensor(klen, dtype=torch.int32, device="cuda")
    if packed_dont_care:
        u_rows = torch.cat([uv[b, :klen[b]] for b in range(B)])
        cu_d = torch.tensor([0, klen[0]], dtype=torch.int32, device="cuda")
    else:
        u_rows, cu_d = uv.reshape(B * Tv, 2 * d), None
    cm_launch(eng, u_rows, lens_d, cu_d, B, Tv, Tv, d, ks, layer_norm, w, 1)
    flag = eng.range_flag()
    z = cm_launch(eng, u_rows, lens_d, cu_d, B, Tv, Tv, d, ks, layer_norm, w, 0)    # the values, from an fp32 store (1e5 is inf in sp32)
    eng.range_flag()
    return flag, z[:u_rows.shape[0]]


@pytest.mark.gpu
def test_convmod_range_flag_and_refusals():
    """The range flag is raised by one valid output beyond 60000 and is not raised when such a value would sit only in a frame
    >= klen of the packed layout; refused shapes are errors that write nothing."""
    eng = _engine()
    assert not eng.range_flag()
    for (ks, d) in ((5, 64), (31, 768)):
        flag, dec = _cm_flag_case(eng, False, ks, d, False)
        assert flag and int((dec.abs() > 60000).sum()) == 1, (ks, d, flag)
        flag, dec = _cm_flag_case(eng, False, ks, d, True)
        assert not flag and float(dec[:, 0].abs().max()) == 0.0, (ks, d, flag)
    for (ks, d) in ((5, 192), (9, 1024), (31, 768)):    # ln4 x 2 and the 8-frame LayerNorm kernel
        flag, dec = _cm_flag_case(eng, True, ks, d, False)
        assert flag and float(dec.abs().max()) > 60000, (ks, d, flag)
    Err = _err()
    g = torch.Generator(device="cuda").manual_seed(1)
    for (layer_norm, ks, d) in ((False, 5, 96), (False, 7, 64), (True, 7, 192), (True, 5, 1028), (True, 31, 1028)):
        w = cm_weights(layer_norm, ks, d, g)
        u = torch.randn(2 * 10, 2 * d, generator=g, device="cuda")
        z = sbuf(20, d)
        with pytest.raises(Err) as e:
            eng.op_convmod(u, z, w["dw_w"], w["dw_b"], w["n_scale"], w["n_shift"], torch.tensor([10, 4], dtype=torch.int32, device="cuda"),
                           2, 10, 10, d, ks, layer_norm)
        torch.cuda.synchronize()
        assert "conv" in str(e.value) and bool((z == SENT).all()), (layer_norm, ks, d, str(e.value))
    assert not eng.range_flag()
