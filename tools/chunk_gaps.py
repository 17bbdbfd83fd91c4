#!/usr/bin/env python3
"""Where the card stands between the measuring passes of consecutive chunks, out of a rocprofv3 kernel trace
(`--kernel-trace --output-format csv`: `*_kernel_trace.csv`).

    python tools/chunk_gaps.py <kernel_trace.csv> [kernel-name substring, default "k_tile2<true, true, true>"]
                               [--alone-us D]

The launches of the named kernel in start order; per consecutive pair start(i + 1) - end(i): positive = nothing of that
kernel on the card for that long (a gap), negative = the two launches shared the card (an overlap).  Printed: the
launch count, the kernel's own duration, median / mean gap or overlap, and the span per launch (first start to last end
of each uninterrupted run of launches, divided by its launches) -- the figure that sets the step time.

Then, per step: the share of the step's span in which no, one and two launches of the kernel are on the
card; the duration of the launches that shared the card with no other launch of the kernel for their whole length and
of those that did; and the rates r1 (launches per ms of one alone: 1 / --alone-us, a lone duration taken from another
trace, or else 1 / the median of this trace's lone launches) and r2 (of two together: what N = T1 r1 + T2 r2 leaves for
the time T2 with two on the card).  Then, per stream of the trace that carries the kernel: what else ran on it, the gaps between its consecutive
launches, and for every launch but the first of a step how long before its start the last kernel of another stream
that started during the launch in front of it had ended (the first tile of its own chunk, when the measuring passes
run alone on their stream: positive = finished before the pass in front of its own ended)."""
import csv
import statistics
import sys


def occupancy(run):
    """Time with 0 / 1 / 2+ of the intervals active between the first start and the last end, in us."""
    edges = sorted([(s, 1) for s, _e in run] + [(e, -1) for _s, e in run])
    t = [0.0, 0.0, 0.0]
    active, prev = 0, edges[0][0]
    for at, d in edges:
        t[min(active, 2)] += (at - prev) / 1e3
        active += d
        prev = at
    return t


def main():
    args = sys.argv[1:]
    alone_us = None
    if "--alone-us" in args:
        k = args.index("--alone-us")
        alone_us = float(args[k + 1])
        del args[k:k + 2]
    path = args[0]
    want = args[1] if len(args) > 1 else "k_tile2<true, true, true>"
    rows, every = [], []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            k = (int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
            every.append((k[0], k[1], r.get("Stream_Id", "?"), r["Kernel_Name"]))
            if want in r["Kernel_Name"]:
                rows.append(k)
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

    # ---- how much of a step the launches share the card, and what sharing costs ----
    lone, shared = [], []
    for run in runs:
        for i, (s, e) in enumerate(run):
            other = any(s2 < e and e2 > s for j, (s2, e2) in enumerate(run) if j != i)
            (shared if other else lone).append((e - s) / 1e3)
    print(f"  launches alone on the card for their whole length: {len(lone)}"
          + (f", median {statistics.median(lone):.1f} us" if lone else ""))
    print(f"  launches that shared it with another: {len(shared)}"
          + (f", median {statistics.median(shared):.1f} us" if shared else ""))
    if lone and alone_us is None:
        alone_us = statistics.median(lone)
    for k, run in enumerate(runs):
        if len(run) < 4:
            continue
        t0, t1, t2 = occupancy(run)
        span = t0 + t1 + t2
        line = (f"  step {k}: {len(run)} launches over {span / 1e3:.3f} ms; none on the card {100 * t0 / span:.1f} %, "
                f"one {100 * t1 / span:.1f} %, two {100 * t2 / span:.1f} %")
        if alone_us and t2 > 0:
            r1 = 1e3 / alone_us
            r2 = (len(run) - t1 / 1e3 * r1) / (t2 / 1e3)
            line += f"; r1 {r1:.3f} / ms, r2 {r2:.3f} / ms ({100 * (r2 / r1 - 1):+.1f} %)"
        print(line)

    # ---- stream by stream ----
    every.sort()
    for sid in sorted({st for s, e, st, name in every if want in name}):
        mine = [(s, e, name) for s, e, st, name in every if st == sid]
        others = sorted({name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0].split("<")[0]
                         for _s, _e, name in mine if want not in name})
        walks = [(s, e) for s, e, name in mine if want in name]
        g = [(b[0] - a[1]) / 1e3 for a, b in zip(walks, walks[1:]) if b[0] - a[1] < 1_000_000]
        print(f"stream {sid}: {len(walks)} launches of the kernel; other kernels on it: {others if others else 'none'}")
        if g:
            print(f"  start(i+1) - end(i) on this stream: median {statistics.median(g):+.2f} us, min {min(g):+.2f}, "
                  f"max {max(g):+.2f}")
        ahead = []
        for a, b in zip(walks, walks[1:]):
            if b[0] - a[1] > 1_000_000:
                continue
            ends = [e for s, e, st, name in every if st != sid and a[0] <= s < b[0]]
            if ends:
                ahead.append((a[1] - max(ends)) / 1e3)
        if ahead:
            late = sum(1 for x in ahead if x < 0)
            print(f"  end of the launch in front - end of the last kernel other streams started during it: median "
                  f"{statistics.median(ahead):+.1f} us, min {min(ahead):+.1f} ({late} of {len(ahead)} ended later)")


if __name__ == "__main__":
    main()
