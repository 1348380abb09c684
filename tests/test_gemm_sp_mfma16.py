"""GPU: the split-fp16 GEMM's main loop on v_mfma_f32_16x16x32_f16 (gam_gemm_sp.h) -- lane, row and column mapping of the fragment
reads and of the epilogue, checked EXACTLY, and its accuracy on random operands at the same shapes.

Exact-integer test: operands are integers |a|, |w| <= 8, so hi = fp16(x) is exact, lo = 0, the per-row power-of-two scale of A is
exact and every partial sum (|sum| <= 64 K <= 2^15) is exact in fp32 whatever the summation order: C must EQUAL an int64 matmul done
on the CPU.  Integer bias and residual and alpha = 0.5 keep the epilogue exact too; only SiLU rounds.  One wrong lane, row, column,
k-slot or LDS swizzle key anywhere changes some output by at least 1/2.

Every tile class (MT x NW / LDS stages) is forced through gam_tune_sp / gam_tune_sp_stages, confirmed with gam_plan_sp_ex and
reset in a finally (test_hip_kernel_matrix.forced).  M = 2 * 64 MT + 37 leaves a partial row tile, N = 64 NW + 36 a partial
column tile that ends inside an 8-column group (N % 8 == 4); K = 32 / 96 / 160 are 1 / 3 / 5 k-tiles (fewer than the stages; odd).
Split-K into 3 slices: the planner takes a forced S only with at least 4 whole k-tiles per slice (gam_gemm_sp_plan), so those
cases run at K = 384 (12 k-tiles), in addition to the three K above at S = 1.  The one-term mode sees K / 2: K = 64 / 192 (1 / 3 of
its k-tiles) and K = 768 for S = 3."""
import pytest
import torch

from test_hip_kernel_matrix import CLASSES, TOL_GEMM_REL, _engine, _operands, _ref, forced, plan_ex

# the three-term kernel's bar against fp64, relative to max(1, max |ref|): tests/test_hip_kernel_matrix.py,
# test_gemm_instantiation_matrix ("assert err < 2e-5"); the one-term bar is its TOL_GEMM_REL
TOL_X3_REL = 2e-5

# (bias, residual with alpha = 0.5, act)   act: 0 none, 1 SiLU, 2 ReLU
EPILOGUES = [(False, False, 0), (True, False, 0), (True, False, 2), (True, False, 1), (True, True, 0), (False, True, 2)]
K_BY_MODE = {"f16x3": ([32, 96, 160], 384), "f16": ([64, 192], 768)}


def _shape(mt, nw):
    return 2 * 64 * mt + 37, 64 * nw + 36


def _cases(mode):
    """(mt, nw, ns, S, K): every class at every K with one slice, and at the deep K with three."""
    ks, k_split = K_BY_MODE[mode]
    return [(mt, nw, ns, 1, k) for (mt, nw, ns) in CLASSES for k in ks] + [(mt, nw, ns, 3, k_split) for (mt, nw, ns) in CLASSES]


def _int_operands(m, n, k, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-8, 9, (m, k), generator=g)
    w = torch.randint(-8, 9, (n, k), generator=g)
    b = torch.randint(-8, 9, (n,), generator=g)
    r = torch.randint(-8, 9, (m, n), generator=g)
    return a, w, b, r


def _silu_bound(pre):
    """|error| allowed on silu(x) = x sigmoid(x) for an EXACT fp32 x: 8 fp32 ulp of the result (2^-24 relative each) -- exp,
    reciprocal and product each round: <= 2 + 1 + 0.5 ulp, doubled for slack.  The rounding of the exponential's argument changes
    exp(-x) by the RELATIVE amount |x| 2^-24 (exp(-x (1 + e)) = exp(-x) (1 - x e)).  For x < 0 sigmoid(x) ~ exp(x), so the result
    takes that relative error in full: there, and only there, the 8 ulp scale with max(1, |x|).  For x >= 0 it moves sigmoid =
    1 / (1 + exp(-x)) by at most x exp(-x) 2^-24 < 2^-24 relative: inside the plain bound.  A sigmoid below the normal range (x <
    -87) may flush to zero BEFORE it is multiplied by x, an error of up to |x| 2^-126."""
    ref = pre * torch.sigmoid(pre)
    scale = torch.where(pre < 0, pre.abs().clamp(min=1.0), torch.ones_like(pre))
    return ref, 8 * 2.0 ** -24 * ref.abs() * scale + 2.0 ** -126 * pre.abs().clamp(min=1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f16x3", "f16"])
def test_integer_operands_give_the_exact_product(mode):
    eng = _engine(mode)
    h16 = mode == "f16"
    launched = set()
    for (mt, nw, ns, S, k) in _cases(mode):
        m, n = _shape(mt, nw)
        kk = k // 2 if h16 else k
        a, w, b, r = _int_operands(m, n, k, seed=1000 * mt + 100 * nw + k)
        prod = a @ w.t()                                        # int64, on the CPU
        ad, wd, bd, rd = a.float().cuda(), w.float().cuda(), b.float().cuda(), r.float().cuda()
        for (bias, resid, act) in EPILOGUES:
            with forced(mt, nw, S, ns):
                assert plan_ex(m, n, kk) == (mt, nw, S, ns), (mode, m, n, k, mt, nw, S, ns)
                out = eng.op_gemm(ad, wd, bd if bias else None, act, resid=rd if resid else None, alpha=0.5 if resid else 1.0)
            out = out.cpu().double()
            pre = (prod + b if bias else prod).double()
            tag = (mode, mt, nw, ns, S, k, bias, resid, act)
            if act == 1:
                ref, bound = _silu_bound(pre)
                excess = ((out - ref).abs() - bound).max()
                assert float(excess) <= 0.0, (tag, float((out - ref).abs().max()))
                continue
            ref = pre.clamp_min(0) if act == 2 else pre
            if resid:
                ref = 0.5 * ref + r
            bad = (out != ref).nonzero()
            assert bad.numel() == 0, (tag, "first wrong (row, col)", bad[0].tolist(), "of", int(bad.shape[0]),
                                      float(out[tuple(bad[0])]), float(ref[tuple(bad[0])]))
        launched.add((mt, nw, ns, S > 1))
    assert not eng.range_flag()
    assert launched == {(mt, nw, ns, sk) for (mt, nw, ns) in CLASSES for sk in (False, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f16x3", "f16"])
def test_random_operands_against_fp64(mode):
    """N(0, 1) activations (weights N(0, 1) / sqrt(K), as in test_hip_kernel_matrix._operands) at the shapes of the integer test,
    against fp64, at the bars test_gemm_instantiation_matrix applies: 2e-5 three-term, TOL_GEMM_REL one-term, relative to
    max(1, max |ref|)."""
    eng = _engine(mode)
    h16 = mode == "f16"
    tol = TOL_GEMM_REL if h16 else TOL_X3_REL
    worst = 0.0
    for i, (mt, nw, ns, S, k) in enumerate(_cases(mode)):
        m, n = _shape(mt, nw)
        bias, _, act = EPILOGUES[i % 4]
        a, w, b = _operands(m, n, k, bias, seed=31 * i + k)
        ref = _ref(a, w, b, act)
        with forced(mt, nw, S, ns):
            assert plan_ex(m, n, k // 2 if h16 else k) == (mt, nw, S, ns)
            out = eng.op_gemm(a, w, b, act)
        err = float((out.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
        worst = max(worst, err)
        assert err < tol, (mode, mt, nw, ns, S, k, bias, act, err)
    print(f"gemm_sp_mfma16 random operands, {mode}: worst relative error {worst:.3e} (bar {tol:g})")
