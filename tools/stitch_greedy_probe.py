"""The two kernels of the windowed longform path at recording size: gam_op_ctc_stitch and gam_op_ctc_greedy_long on one hour of
encoder frames (T = 90 000) cut as the default plan cuts it (windows of 500 frames, 83 dropped at each inner edge), for a char-level
and a subword vocabulary (V = 34 and V = 1025 by default).  Checks both results against numpy, then times them with events and
prints one JSON line per vocabulary with the achieved bandwidth (input bytes T x V x 4 plus the outputs).  A tool, not a test: no
threshold.  For kernel times run it under ``rocprofv3 --kernel-trace --stats -- python tools/stitch_greedy_probe.py``.

    python tools/stitch_greedy_probe.py [--frames T] [--classes V [V ...]] [--repeat N]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ctc_greedy_long_ref import greedy_ref  # noqa: E402


def timed(fn, repeat):
    best = None
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=90000)
    ap.add_argument("--classes", type=int, nargs="+", default=[34, 1025])
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    from gigaam_amd import synth
    from gigaam_amd.engine import HipEngine, build_config
    from gigaam_amd.windows import plan_windows
    cfg = synth.model_cfg("v2_ctc")
    eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], None), {}, torch.device("cuda:0"))
    T = args.frames
    plan = plan_windows((T - 1) * 640, 640, lambda n: (n // 160 + 1 + 3) // 4)       # centred frontend: T' = ceil((n / 160 + 1) / 4)
    assert plan.t_total == T, (plan.t_total, T)
    ws = plan.windows
    B, Tp = len(ws), plan.chunk_frames + 1
    lo = torch.tensor([w.lo for w in ws], dtype=torch.int32).cuda()
    hi = torch.tensor([w.hi for w in ws], dtype=torch.int32).cuda()
    dst = torch.tensor([w.dst for w in ws], dtype=torch.int64).cuda()
    enc_len = torch.tensor([Tp] * (B - 1) + [ws[-1].hi], dtype=torch.int32).cuda()
    for V in args.classes:
        g = torch.Generator(device="cuda:0").manual_seed(V)
        lp = torch.randn((B, Tp, V), generator=g, device="cuda:0")
        lab = torch.randint(0, V, (B, (Tp + 1) // 2), generator=g, device="cuda:0").repeat_interleave(2, dim=1)[:, :Tp]
        lp.scatter_add_(2, lab[:, :, None], torch.full((B, Tp, 1), 6.0, device="cuda:0"))
        out = torch.empty((T, V), dtype=torch.float32, device="cuda:0")
        status = eng.op_ctc_stitch(lp, enc_len, lo, hi, dst, out)
        assert bool(status.cpu().all())
        lp_h = lp.cpu().numpy()
        want = np.concatenate([lp_h[k, w.lo:w.hi] for k, w in enumerate(ws)])
        assert (out.cpu().numpy().view(np.int32) == want.view(np.int32)).all()
        rows, _ = HipEngine.collect(eng.op_ctc_greedy_long(out))
        assert rows[0] == greedy_ref(want)
        n_tok = len(rows[0][0])
        stitch_ms = timed(lambda: eng.op_ctc_stitch(lp, enc_len, lo, hi, dst, out), args.repeat)
        greedy_ms = timed(lambda: eng.op_ctc_greedy_long(out), args.repeat)
        stitch_bytes = 2.0 * T * V * 4                              # every kept row read once and written once
        greedy_bytes = T * V * 4.0 + T * 4 * 2 + n_tok * 8.0        # the rows, the label workspace written and read, ids + frames
        print(json.dumps({"probe": "stitch_greedy", "T": T, "V": V, "windows": B, "tokens": n_tok,
                          "stitch_ms": round(stitch_ms, 4), "stitch_GBps": round(stitch_bytes / stitch_ms / 1e6, 1),
                          "greedy_long_ms": round(greedy_ms, 4), "greedy_long_GBps": round(greedy_bytes / greedy_ms / 1e6, 1),
                          "note": "event times of the whole call (greedy: three launches); kernel times: rocprofv3 --kernel-trace --stats"}),
              flush=True)


if __name__ == "__main__":
    main()
