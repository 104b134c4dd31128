"""Timeline of one fused step in a rocprofv3 kernel trace (`--kernel-trace
--output-format csv` writes <name>_kernel_trace.csv): every dispatch of the
last step but one, from the first dispatch after the step before it to the
next step's first fill (so side-stream kernels that end after size_fix_kernel
are in it), with its queue, start (us from the step's first dispatch),
duration and the idle gap since the latest end of any earlier dispatch.
Usage: trace_timeline.py <kernel_trace.csv>"""
import csv
import re
import sys

rows = []
with open(sys.argv[1], newline="") as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Queue_Id", "")))
rows.sort()
marks = [i for i, r in enumerate(rows) if "size_fix_kernel" in r[2]]
if len(marks) < 3:
    sys.exit("fewer than three size_fix_kernel dispatches in the trace")
lo, hi = marks[-3] + 1, marks[-2] + 1
while lo < len(rows) and "fillBuffer" not in rows[lo][2]:   # the earlier step's side-stream tail
    lo += 1
while hi < len(rows) and "fillBuffer" not in rows[hi][2]:
    hi += 1
step = rows[lo:hi]
t0 = step[0][0]
latest = t0
print(f"{'kernel':34s} {'queue':>5s} {'start_us':>10s} {'dur_us':>10s} {'gap_us':>9s}")
for s, e, name, q in step:
    short = re.sub(r"\(anonymous namespace\)::", "", name)
    short = re.sub(r"\(.*", "", short).replace("void ", "").replace("ose::", "")
    print(f"{short[:34]:34s} {q:>5s} {(s - t0) / 1e3:10.1f} {(e - s) / 1e3:10.1f} {(s - latest) / 1e3:9.1f}")
    latest = max(latest, e)
print(f"step span {(latest - t0) / 1e3:.1f} us")
