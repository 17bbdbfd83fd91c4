#!/usr/bin/env python3
"""Where the card stands between the measuring passes of consecutive chunks, out of a rocprofv3 kernel trace
(`--kernel-trace --output-format csv`: `*_kernel_trace.csv`).

    python tools/chunk_gaps.py <kernel_trace.csv> [kernel-name substring, default "k_tile2<true, true, true>"]

The launches of the named kernel in start order; per consecutive pair start(i + 1) - end(i): positive = nothing of that
kernel on the card for that long (a gap), negative = the two launches shared the card (an overlap).  Printed: the
launch count, the kernel's own duration, median / mean gap or overlap, and the span per launch (first start to last end
of each uninterrupted run of launches, divided by its launches) -- the figure that sets the step time."""
import csv
import statistics
import sys


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "k_tile2<true, true, true>"
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if want in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    if len(rows) < 2:
        sys.exit(f"fewer than two launches of {want!r} in {path}")
    dur = [(e - s) / 1e3 for s, e in rows]
    # a step is a run of launches less than 1 ms apart (between steps the host synchronises)
    runs, cur = [], [rows[0]]
    for prev, nxt in zip(rows, rows[1:]):
        if nxt[0] - prev[1] > 1_000_000:
            runs.append(cur)
            cur = []
        cur.append(nxt)
    runs.append(cur)
    gaps = []
    for run in runs:
        gaps += [(b[0] - a[1]) / 1e3 for a, b in zip(run, run[1:])]
    per_launch = [(max(e for _s, e in run) - run[0][0]) / 1e3 / len(run) for run in runs if len(run) > 1]
    print(f"{want}: {len(rows)} launches in {len(runs)} runs")
    print(f"  duration per launch: median {statistics.median(dur):.1f} us, mean {statistics.mean(dur):.1f} us")
    print(f"  start(i+1) - end(i): median {statistics.median(gaps):+.1f} us, mean {statistics.mean(gaps):+.1f} us, "
          f"min {min(gaps):+.1f}, max {max(gaps):+.1f}  (positive: gap, negative: overlap)")
    print(f"  span per launch within a run: median {statistics.median(per_launch):.1f} us")


if __name__ == "__main__":
    main()
