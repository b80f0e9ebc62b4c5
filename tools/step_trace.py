#!/usr/bin/env python
"""One timed step of bench.py out of a `rocprofv3 --kernel-trace --output-format csv` run, as a markdown table: every launch between
two consecutive pose -> camera launches (the first kernel of a step) with its start offset, duration, grid and the gap to the end
of the launch before it.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --steps 6 --warmup 2
    python tools/step_trace.py DIR [--step -2] > profiles/<name>.md

--step counts the steps found in the trace (negative: from the end; the default, -2, is the last step that is followed by another
one, i.e. bounded on both sides)."""
import argparse
import csv
import sys
from pathlib import Path

FIRST = "k_pose_camera_fwd"
BIG = ("k_trilinear_fwd", "k_trilinear_splat_b16", "k_siddon_slab", "k_siddon_gather_vol2", "k_siddon_splat")


def short(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    cut = name.find("(")
    name = name[:cut] if cut > 0 else name
    return name if len(name) <= 70 else name[:67] + "..."


def load(trace_dir):
    files = sorted(Path(trace_dir).rglob("*kernel_trace.csv"))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                grid = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
                wg = int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 1)
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], grid // max(wg, 1), wg))
    rows.sort()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace_dir")
    ap.add_argument("--step", type=int, default=-2)
    a = ap.parse_args()
    rows = load(a.trace_dir)
    starts = [i for i, r in enumerate(rows) if FIRST in r[2]]
    if len(starts) < 3:
        raise SystemExit(f"fewer than three {FIRST} launches in the trace")
    k = a.step if a.step >= 0 else len(starts) - 1 + a.step   # (the last start has no step behind it)
    lo, hi = starts[k], starts[k + 1]
    step = rows[lo:hi]
    t0, period = step[0][0], rows[hi][0] - step[0][0]
    print(f"step {k} of {len(starts) - 1} in the trace: {len(step)} launches, {period / 1e6:.3f} ms from its first launch to the next step's\n")
    print("| # | kernel | workgroups x threads | start (ms) | duration (ms) | gap to previous end (ms) |")
    print("|---|---|---|---|---|---|")
    busy = big = 0.0
    prev_end = None
    for i, (s, e, name, wgs, wg) in enumerate(step):
        gap = "" if prev_end is None else f"{(s - prev_end) / 1e6:.4f}"
        print(f"| {i} | `{short(name)}` | {wgs} x {wg} | {(s - t0) / 1e6:.4f} | {(e - s) / 1e6:.4f} | {gap} |")
        busy += (e - s) / 1e6
        if any(b in name for b in BIG):
            big += (e - s) / 1e6
        prev_end = e if prev_end is None else max(prev_end, e)
    print(f"\nsummed kernel time {busy:.3f} ms; forward march + voxel-gradient kernel {big:.3f} ms; every other launch {busy - big:.3f} ms; "
          f"step period minus the two big kernels {period / 1e6 - big:.3f} ms (other launches + gaps)")


if __name__ == "__main__":
    sys.exit(main())
