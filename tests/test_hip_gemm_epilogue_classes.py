"""GPU: the epilogue classes of the split-fp16 GEMM (gam_gemm_sp.h, template parameter EPI) -- one case set per class the launcher can
select (gam_launch_gemm_sp) plus the generic class, through gam_op_gemm_fmt, each against a float64 product of the same operands at the
bar of the tile-plan matrix test (test_hip_kernel_matrix.test_gemm_instantiation_matrix: 2e-5 of max(1, max |ref|) three-term,
TOL_GEMM_REL one-term).

Shapes: M in {1, 15, 17, 193} (a lane's rows partly and wholly beyond M; a 192-row tile plus one), K in {32, 96} (one and three
k-tiles; 256 for split-K: a slice needs four), N in {4, 8, 12, 36, 260}: N % 8 == 4 takes the half-group tail, which only the generic
class carries, so the SAME options at N = 8 / 260 run the class and at N = 4 / 12 / 36 the generic code -- both are held to the same
reference.  C lies in a wider buffer (pitch > N, two rows more than M) filled with a canary: nothing outside [M, N] may change.  The
residual is read from C itself, as every encoder caller does.

The masked / remapped class (ReLU, sp32, guard, rows) has no raw entry: it runs through the two stems (test_hip_front_matrix holds them
to fp64 over many more lengths); here one ragged batch per stem, with NaN in the don't-care frames."""
import pytest
import torch

from test_hip_kernel_matrix import CLASSES, TOL_GEMM_REL, _engine, forced, plan_ex

TOL_X3_REL = 2e-5          # test_gemm_instantiation_matrix: "assert err < 2e-5"
CANARY = 777.0
SAFE_MAX = 60000.0         # GAM_F16_SAFE_MAX (gam_common.h)
MS, KS, NS_ = [1, 15, 17, 193], [32, 96], [4, 8, 12, 36, 260]

# name -> (act, c_split, residual, alpha, guard, bias): the classes of gam_launch_gemm_sp a raw launch reaches at N % 8 == 0 (the split-K
# slice class runs in front of the reduce pass of every option set in test_tile_plans_agree_and_splitk_reduces_the_same) ...
CLASS_CASES = {
    "none|fp32": (0, 0, False, 1.0, False, True),
    "none|fp32+R": (0, 0, True, 1.0, False, True),
    "none|fp32+R,alpha": (0, 0, True, 0.5, False, False),
    "none|fp32,guard": (0, 0, False, 1.0, True, True),
    "silu|sp32,guard": (1, 1, False, 1.0, True, True),
}
# ... and option sets that no class has: the generic code whatever N is
GENERIC_CASES = {
    "relu|fp32": (2, 0, False, 1.0, False, True),
    "silu|fp32+R,alpha": (1, 0, True, 0.5, False, True),
    "relu|fp32+R,guard": (2, 0, True, 1.0, True, False),
    "none|sp32": (0, 1, False, 1.0, False, False),
    "relu|sp32,guard": (2, 1, False, 1.0, True, True),
}

_ENG = {}


def engine(mode="f16x3"):
    if mode not in _ENG:
        _ENG[mode] = _engine(mode)
    _ENG[mode].set_gemm_mode(mode)
    return _ENG[mode]


def operands(m, n, k, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(m, k, generator=g, device="cuda")
    w = torch.randn(n, k, generator=g, device="cuda") / k ** 0.5
    b = torch.randn(n, generator=g, device="cuda")
    r = torch.randn(m, n, generator=g, device="cuda")
    return a, w, b, r


def reference(a, w, b, r, act, alpha):
    x = a.double() @ w.double().t()
    if b is not None:
        x = x + b.double()
    x = x * torch.sigmoid(x) if act == 1 else (x.clamp_min(0) if act == 2 else x)
    x = alpha * x
    return x + r.double() if r is not None else x


def pitch(n):
    return (n + 31) // 32 * 32 + 32


def launch(eng, a, w, b, r, act, alpha, c_split, guard):
    """One gam_op_gemm_fmt call into a canary-filled buffer [M + 2, pitch]; the residual, if any, sits in C.  Returns the raw buffer."""
    m, n, ldc = a.shape[0], w.shape[0], pitch(w.shape[0])
    if c_split:
        out = torch.full((m + 2, 2 * ldc), CANARY, dtype=torch.float16, device="cuda").view(torch.float32)
    else:
        out = torch.full((m + 2, ldc), CANARY, dtype=torch.float32, device="cuda")
    if r is not None:
        out[:m, :n] = r
    eng.op_gemm_fmt(a, w, out, b, act, resid=out if r is not None else None, alpha=alpha, c_split=c_split, c_guard=guard)
    return out


def decode(out, m, n, c_split):
    """(values fp64 [M, N], hi plane or None, lo plane or None, untouched: bool) of a raw buffer."""
    ldc = out.shape[1]
    if c_split == 0:
        keep = out.clone()
        keep[:m, :n] = CANARY
        return out[:m, :n].double(), None, None, bool((keep == CANARY).all())
    h = out.view(torch.float16)
    if c_split == 1:   # row: 32-column blocks of [hi x32 | lo x32]
        blk = h.view(m + 2, ldc // 32, 2, 32)
        hi = blk[:, :, 0, :].reshape(m + 2, ldc)
        lo = blk[:, :, 1, :].reshape(m + 2, ldc)
        keep_h, keep_l = hi.clone(), lo.clone()
        keep_h[:m, :n] = CANARY
        keep_l[:m, :n] = CANARY
        ok = bool((keep_h == CANARY).all()) and bool((keep_l == CANARY).all())
        return hi[:m, :n].double() + lo[:m, :n].double(), hi[:m, :n], lo[:m, :n], ok
    hv = h.view(-1)[: (m + 2) * ldc].view(m + 2, ldc)      # plain fp16 rows of pitch ldc HALFS: the first half of the buffer
    vals = hv[:m, :n].clone()
    keep = h.view(-1).clone()
    keep[: (m + 2) * ldc].view(m + 2, ldc)[:m, :n] = CANARY
    return vals.double(), vals, None, bool((keep == CANARY).all())


def check_case(eng, name, opts, m, n, k, tol):
    act, c_split, resid, alpha, guard, bias = opts
    a, w, b, r = operands(m, n, k, seed=1000 * m + 10 * n + k)
    b = b if bias else None
    r = r if resid else None
    ref = reference(a, w, b, r, act, alpha)
    out = launch(eng, a, w, b, r, act, alpha, c_split, guard)
    val, hi, lo, untouched = decode(out, m, n, c_split)
    tag = (name, m, n, k)
    assert untouched, ("canary overwritten outside [M, N]", tag)
    err = float((val - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    assert err < tol, (tag, err)
    if c_split:   # the planes are the split of the fp32 result of the same launch without a format: hi = fp16(x), lo = fp16(x - hi)
        x = decode(launch(eng, a, w, b, r, act, alpha, 0, guard), m, n, 0)[0].float()
        assert torch.equal(hi, x.half()), ("hi plane is not fp16(x)", tag)
        if lo is not None:
            assert torch.equal(lo, (x - x.half().float()).half()), ("lo plane is not fp16(x - hi)", tag)
    return err


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CLASS_CASES) + list(GENERIC_CASES))
def test_every_class_at_the_edge_shapes(name):
    """Every M x K x N of the lists above under one option set.  N % 8 == 4 (4, 12, 36) runs the generic class whatever the options."""
    eng = engine()
    opts = CLASS_CASES.get(name) or GENERIC_CASES[name]
    worst = 0.0
    for m in MS:
        for k in KS:
            for n in NS_:
                worst = max(worst, check_case(eng, name, opts, m, n, k, TOL_X3_REL))
    assert not eng.range_flag()
    print(f"epilogue class {name}: worst relative error {worst:.3e} (bar {TOL_X3_REL:g})")


@pytest.mark.gpu
def test_fp16_rows_in_the_one_term_mode():
    """C as plain fp16 rows exists in the one-term mode only (generic class there): K = 64 / 192 are 1 / 3 of its k-tiles."""
    eng = engine("f16")
    try:
        for m in MS:
            for k in (64, 192):
                for n in NS_:
                    check_case(eng, "f16 silu|fp16,guard", (1, 2, False, 1.0, True, True), m, n, k, TOL_GEMM_REL)
                    check_case(eng, "f16 none|fp32+R", (0, 0, True, 1.0, False, True), m, n, k, TOL_GEMM_REL)
        assert not eng.range_flag()
    finally:
        eng.set_gemm_mode("f16x3")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CLASS_CASES) + ["relu|fp32", "none|sp32"])
def test_tile_plans_agree_and_splitk_reduces_the_same(name):
    """M = 193, N = 260 (and 36: the tail): every single-slice tile plan gives the same bytes; forced into two slices at K = 256 (a slice needs four k-tiles)
    (the split-K slice class in front of the reduce pass, which applies the options) the result stays inside the bar."""
    eng = engine()
    act, c_split, resid, alpha, guard, bias = CLASS_CASES.get(name) or GENERIC_CASES[name]
    for n in (260, 36):
        m, k = 193, 256
        a, w, b, r = operands(m, n, k, seed=n)
        b, r = (b if bias else None), (r if resid else None)
        ref = reference(a, w, b, r, act, alpha)
        first = None
        for (mt, nw, ns) in CLASSES:
            for S in (1, 2):
                with forced(mt, nw, S, ns):
                    assert plan_ex(m, n, k) == (mt, nw, S, ns)
                    out = launch(eng, a, w, b, r, act, alpha, c_split, guard)
                val, _, _, untouched = decode(out, m, n, c_split)
                assert untouched, (name, n, mt, nw, ns, S)
                err = float((val - ref).abs().max()) / max(1.0, float(ref.abs().max()))
                assert err < TOL_X3_REL, (name, n, mt, nw, ns, S, err)
                if S == 1:
                    if first is None:
                        first = out
                    else:
                        assert torch.equal(out.view(torch.int32), first.view(torch.int32)), ("single-slice plans differ", name, n, mt, nw, ns)
    assert not eng.range_flag()


def _flag_after(eng, opts, value=None, bias_value=None):
    """M = 193, N = 264 under the 192 x 256 tile: element (191, 255) is the last row and the last column of the last lane of the
    tile's last wave.  `value`: A and W are one-hot so that exactly that output is `value`; `bias_value`: column 255 of the bias."""
    act, c_split, resid, alpha, guard, _ = opts
    m, n, k = 193, 264, 32
    a = torch.zeros(m, k, device="cuda")
    w = torch.zeros(n, k, device="cuda")
    b = torch.zeros(n, device="cuda")
    if value is not None:
        a[191, 0] = value
        w[255, 0] = 1.0
    if bias_value is not None:
        b[255] = bias_value
    with forced(3, 4, 1, 2):
        assert plan_ex(m, n, k) == (3, 4, 1, 2)
        out = launch(eng, a, w, b, None, act, alpha, c_split, guard)
    if value is not None:   # (SiLU rounds: 60001 sigmoid(60001) within one fp16-split step of 60001)
        want = max(value, 0.0) if act == 2 else value
        assert abs(float(decode(out, m, n, c_split)[0][191, 255]) - want) <= (0.01 if act == 1 else 0.0)
    return eng.range_flag()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["none|fp32,guard", "silu|sp32,guard", "relu|sp32,guard"])
def test_range_guard_flag(name):
    """Bit 0 of the flag word is set iff a stored value exceeds 60000 in magnitude: 60001 in the last element of a lane sets it, 59999
    there leaves it clear; a NaN alone leaves it clear and an Inf sets it (fmaxf drops a NaN operand and `>` is false on one -- the
    per-piece test this replaced behaved the same: profiles/gemm_epilogue_classes.md).  Without c_guard nothing sets it."""
    eng = engine()
    opts = CLASS_CASES.get(name) or GENERIC_CASES[name]
    assert _flag_after(eng, opts, value=SAFE_MAX + 1.0) is True
    assert _flag_after(eng, opts, value=SAFE_MAX - 1.0) is False
    assert _flag_after(eng, opts, bias_value=float("nan")) is False
    assert _flag_after(eng, opts, bias_value=float("inf")) is True
    if name != "silu|sp32,guard":     # (SiLU of a large negative value is 0)
        assert _flag_after(eng, opts, value=-(SAFE_MAX + 1.0)) is (name == "none|fp32,guard")
    unguarded = opts[:4] + (False,) + opts[5:]
    assert _flag_after(eng, unguarded, value=SAFE_MAX + 1.0) is False


@pytest.mark.gpu
@pytest.mark.parametrize("stem", ["conv2d", "conv1d"])
def test_masked_and_remapped_class_through_the_stems(stem):
    """ReLU | sp32, guard, rows: Conv2d #2 (implicit GEMM, row mask) and the conv1d stem's first stage (row mask + remap into the
    zero-bordered buffer of the second), d_model = 192, T = 67, ragged lengths: valid frames at the stem bar of test_stem_matrix, and
    NaN / Inf in the frames behind each length change no valid bit -- a masked row that was not written as exactly 0, or a remapped row
    written beyond rows_valid, would reach the next GEMM's taps."""
    from test_hip_front_matrix import K_STEM, STEM_T, stem_case, stem_engine, stem_run, ulp32, zero_fill
    eng = stem_engine(stem, 192, 64, "f16x3")
    T = 67
    feat, lens, ref, elen_o, e32, vm = stem_case(stem, 192, 64, STEM_T.index(T), T)
    tok, elen, enc = stem_run(eng, feat, lens)
    assert elen.tolist() == elen_o.tolist()
    err = float(((tok.double() - ref) * vm).abs().max())
    assert err < K_STEM[(stem, "f16x3")] * max(e32, ulp32(float((ref * vm).abs().max()))), (stem, err, e32)
    tok_d, elen_d, enc_d = stem_run(eng, zero_fill(feat, lens, fill=True), lens)
    assert bool(torch.isfinite(tok_d).all())
    for b, n in enumerate(elen.clamp(max=tok.shape[1]).tolist()):
        assert torch.equal(tok_d[b, :n], tok[b, :n]), (stem, b)
    assert not eng.range_flag()
