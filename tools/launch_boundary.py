#!/usr/bin/env python3
"""tools/launch_boundary.py KERNEL_TRACE.csv [LAST_N] -- what the boundary between back-to-back count scans costs, from a
rocprofv3 --kernel-trace of a plain bench.py run: per step the duration of sk_scan_grid and of sk_scan_wide, and the time
between the end of one sk_scan_grid and the start of the next (negative: the next one started while this one drained).
Only the last LAST_N (default 30) full-size launches are read: the timed steps, not the preheat's ramp."""
import csv
import statistics
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
last_n = int(sys.argv[2]) if len(sys.argv) > 2 else 30
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
grid = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if "sk_scan_grid" in r["Kernel_Name"]]
wide = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if "sk_scan_wide" in r["Kernel_Name"]]
grid, wide = grid[-last_n:], wide[-last_n:]
dur = [(e - s) / 1e3 for s, e in grid]
wdur = [(e - s) / 1e3 for s, e in wide]
gap = [(grid[i + 1][0] - grid[i][1]) / 1e3 for i in range(len(grid) - 1)]
period = [(grid[i + 1][0] - grid[i][0]) / 1e3 for i in range(len(grid) - 1)]
ends = [(grid[i + 1][1] - grid[i][1]) / 1e3 for i in range(len(grid) - 1)]


def line(name, v):
    print(f"{name:46s} median {statistics.median(v):9.2f} us   min {min(v):9.2f}   max {max(v):9.2f}   (n = {len(v)})")


line("sk_scan_grid duration", dur)
line("sk_scan_wide duration", wdur)
line("end of grid N -> start of grid N+1", gap)
line("start of grid N -> start of grid N+1", period)
line("end of grid N -> end of grid N+1 (step time)", ends)
print(f"launches that started before the previous one ended: {sum(1 for g in gap if g < 0)} of {len(gap)}")
