#!/usr/bin/env python3
"""Single launches of the split-fp16 GEMM in a chosen epilogue class (gam_gemm_sp.h EPI), through gam_op_gemm_fmt: kernel-only timing
(HIP events around the launch) and fp64 error, or -- with an instrumented library (-DGAM_SP_INSTRUMENT=1) and GAM_SP_TLOG=1 -- the
launcher's per-workgroup timeline of each launch.  tools/gemm_sp_test.py does the same for the plain gam_op_gemm entry;
tools/tlog_summary.py condenses the timeline blocks of a whole model run.

A shape is "M,N,K,act,resid,alpha,c_split,guard" (act: 0 none, 1 SiLU, 2 ReLU; c_split: 0 fp32, 1 sp32); the default list is the
headline's five launches at M = 16064: FFN up (SiLU, sp32, guard), FFN down (residual in place, alpha 0.5), attention out /
pointwise-conv2 (residual), q|k|v (guard), pointwise-conv1.

    python tools/gemm_epilogue_launch.py ["M,N,K,act,resid,alpha,c_split,guard;..."]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gigaam_amd import synth  # noqa: E402
from gigaam_amd.engine import HipEngine, build_config  # noqa: E402

HEADLINE = "16064,3072,768,1,0,1.0,1,1;16064,768,3072,0,1,0.5,0,0;16064,768,768,0,1,1.0,0,0;16064,2304,768,0,0,1.0,0,1;16064,1536,768,0,0,1.0,0,0"


def main():
    spec = sys.argv[1] if len(sys.argv) > 1 else HEADLINE
    shapes = [tuple(float(v) if "." in v else int(v) for v in t.split(",")) for t in spec.split(";") if t]
    cfg = synth.model_cfg("v2_ctc")
    e = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], None), {}, torch.device("cuda:0"))
    tlog = bool(os.environ.get("GAM_SP_TLOG"))
    torch.manual_seed(0)
    for (m, n, k, act, resid, alpha, c_split, guard) in shapes:
        a = torch.randn(m, k, device="cuda")
        w = torch.randn(n, k, device="cuda") / k ** 0.5
        b = torch.randn(n, device="cuda")
        r0 = torch.randn(m, n, device="cuda") if resid else None
        ref = a.double() @ w.double().t() + b.double()
        ref = ref * torch.sigmoid(ref) if act == 1 else (ref.clamp_min(0) if act == 2 else ref)
        ref = float(alpha) * ref + (r0.double() if resid else 0.0)
        c = r0.clone() if resid else torch.empty(m, n, device="cuda")

        def call():   # residual in place, as in the encoder (the repeats accumulate into it)
            return e.op_gemm_fmt(a, w, c, b, act, resid=c if resid else None, alpha=float(alpha), c_split=c_split, c_guard=bool(guard))
        out = call().clone()
        if c_split == 1:    # sp32 planes -> values
            pl = out.view(torch.float16).view(m, n // 32, 2, 32).float()
            out = (pl[:, :, 0] + pl[:, :, 1]).reshape(m, n)
        err = float((out.double() - ref).abs().max())
        line = f"M={m:6d} N={n:5d} K={k:6d} act={act} resid={resid} alpha={alpha} c_split={c_split} guard={guard}"
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        if tlog:
            print(f"==== {line} err {err:.1e}: the LAST [tlog] block above this line is the warm one", file=sys.stderr, flush=True)
            continue
        e.profile_enable(2)
        reps = 10
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
        ms = e.profile_read()["gemm"]["ms"] / reps
        e.profile_enable(0)
        print(f"{line} | {ms*1e3:8.1f} us {2.0*m*n*k/ms/1e9:6.1f} TF err {err:.1e} flag {e.range_flag()}", flush=True)


if __name__ == "__main__":
    main()
