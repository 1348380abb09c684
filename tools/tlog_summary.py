#!/usr/bin/env python3
"""Summarise the per-workgroup timeline an instrumented library prints (-DGAM_SP_INSTRUMENT=1, GAM_SP_TLOG=1; gam_gemm_sp.h): the [tlog]
blocks of the LAST step of a model run, grouped by launch shape -- median over the launches of a shape of each block's p50 / p90.

    GAM_GRAPH=0 GAM_SP_TLOG=1 GIGAAM_HIP_LIB=<instrumented .so> python bench.py --gpus 1 --steps 1 --warmup 1 --no-profile --no-power 2> tl.err
    python tools/tlog_summary.py tl.err [launches per step: default half of the blocks]
"""
import re
import statistics
import sys

HEAD = re.compile(r"^\[tlog\] M=(\d+) N=(\d+) K=(\d+) MT=(\d) NW=(\d) tiles=(\d+): first entry -> last exit ([\d.]+) us")
STAT = re.compile(r"^\s+(.+?)\s+min\s+([\d.]+)\s+p50\s+([\d.]+)\s+p90\s+([\d.]+)\s+max\s+([\d.]+)")


def blocks(path):
    out, cur = [], None
    for ln in open(path, errors="replace"):
        m = HEAD.match(ln)
        if m:
            cur = {"shape": tuple(int(v) for v in m.groups()[:6]), "wall": float(m.group(7)), "stat": {}}
            out.append(cur)
            continue
        m = STAT.match(ln)
        if m and cur is not None:
            cur["stat"][m.group(1).strip()] = tuple(float(v) for v in m.groups()[1:])
    return out


def main():
    bl = blocks(sys.argv[1])
    per_step = int(sys.argv[2]) if len(sys.argv) > 2 else len(bl) // 2
    bl = bl[-per_step:]
    groups = {}
    for b in bl:
        groups.setdefault(b["shape"], []).append(b)
    med = statistics.median
    print("| M x N x K | tile | tiles (rounds of 256) | launches | wall us | prologue p50 | loop p50 | per k-tile p10..p90 | epilogue p50 | epilogue p90 |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for (m, n, k, mt, nw, tiles), g in sorted(groups.items(), key=lambda kv: -len(kv[1])):
        s = lambda name, j: med([b["stat"][name][j] for b in g])
        # p10 is not printed by the launcher: min .. p90 of the per-k-tile time stands in for it
        print(f"| {m} x {n} x {k} | {64 * mt} x {64 * nw} | {tiles} ({tiles / 256:.2f}) | {len(g)} | {med([b['wall'] for b in g]):.1f} | "
              f"{s('prologue (2 k-tiles land)', 1):.2f} | {s('main loop', 1):.2f} | {s('per k-tile', 0):.3f}..{s('per k-tile', 2):.3f} | "
              f"{s('epilogue', 1):.2f} | {s('epilogue', 2):.2f} |")


if __name__ == "__main__":
    main()
