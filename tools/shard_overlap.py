"""Overlap of the step launches in a rocprofv3 kernel trace (step shards).

Takes the last `n` core_group_kernel dispatches of run_kernel_trace.csv (the timed window of
bench.py) and prints, from their start and end timestamps: the dispatches per stream / queue,
the mean kernel time, the span of the window per step (`period`: the launches of one step
count as one), the share of the window in which 0, 1, 2, ... step kernels were running, and
the first dispatches of the window as rows (start and end relative to the window's start).

    python tools/shard_overlap.py run_kernel_trace.csv <shards> [steps=500] [rows=12]
"""
import csv
import sys
from collections import Counter

path, S = sys.argv[1], int(sys.argv[2])
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 500
rows = int(sys.argv[4]) if len(sys.argv) > 4 else 12
ks = [r for r in csv.DictReader(open(path)) if "core_group_kernel" in r["Kernel_Name"]]
ks.sort(key=lambda r: int(r["Start_Timestamp"]))
ks = ks[-steps * S:]
t0 = int(ks[0]["Start_Timestamp"])
iv = [(int(r["Start_Timestamp"]) - t0, int(r["End_Timestamp"]) - t0) for r in ks]
span = max(e for _, e in iv)
dur = [e - s for s, e in iv]
qkey = "Queue_Id" if "Queue_Id" in ks[0] else "Stream_Id"
print(f"dispatches {len(ks)} ({S} per step), per {qkey}: {dict(Counter(r[qkey] for r in ks))}")
print(f"grids (workgroups): {dict(Counter(int(r['Grid_Size_X']) // max(1, int(r['Workgroup_Size_X'])) for r in ks))}"
      if "Grid_Size_X" in ks[0] else "")
print(f"kernel time mean {sum(dur) / len(dur) / 1e3:.2f} us, min {min(dur) / 1e3:.2f}, max {max(dur) / 1e3:.2f}")
print(f"window {span / 1e3:.1f} us = {span / 1e3 / (len(ks) / S):.2f} us per step; "
      f"summed kernel time {sum(dur) / 1e3:.1f} us = {sum(dur) / span:.3f} of the window")
ev = sorted([(s, 1) for s, _ in iv] + [(e, -1) for _, e in iv])
busy, level, last = Counter(), 0, 0
for t, d in ev:
    busy[level] += t - last
    level, last = level + d, t
print("share of the window with k step kernels running: " +
      ", ".join(f"k={k}: {busy[k] / span:.3f}" for k in sorted(busy)))
print(f"{'#':>3} {qkey:>9} {'start_us':>10} {'end_us':>10} {'dur_us':>8}")
for i, (r, (s, e)) in enumerate(zip(ks[:rows], iv)):
    print(f"{i:3d} {r[qkey]:>9} {s / 1e3:10.2f} {e / 1e3:10.2f} {(e - s) / 1e3:8.2f}")
