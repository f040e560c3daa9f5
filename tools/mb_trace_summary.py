"""Share of every kernel and the gaps between consecutive dispatches of the profiled block of
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mb_throughput.py --profile-block`:
python tools/mb_trace_summary.py DIR"""
import collections
import csv
import glob
import sys

path = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
rows = list(csv.DictReader(open(path)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
# the timed block = the last half of the dispatches (warm-up block first, then the profiled block)
tail = rows[len(rows) // 2:]
span = int(tail[-1]["End_Timestamp"]) - int(tail[0]["Start_Timestamp"])
busy = sum(dur(r) for r in tail)
gaps = sorted(int(tail[i + 1]["Start_Timestamp"]) - int(tail[i]["End_Timestamp"]) for i in range(len(tail) - 1))
big = [g for g in gaps if g > 100_000]
print(f"# fused MOPO block (second half of the trace): {len(tail)} dispatches, wall {span / 1e6:.1f} ms, sum of kernel durations {busy / 1e6:.1f} ms "
      f"({100.0 * busy / span:.1f} % busy)")
print(f"# gap between consecutive dispatches: median {gaps[len(gaps) // 2] / 1e3:.2f} us, mean {sum(gaps) / len(gaps) / 1e3:.2f} us, "
      f"p99 {gaps[int(len(gaps) * 0.99)] / 1e3:.2f} us; {len(big)} gaps above 100 us sum to {sum(big) / 1e6:.1f} ms")
d = collections.defaultdict(list)
for r in tail:
    d[r["Kernel_Name"].split("(")[0][:90]].append(dur(r))
print("%-92s %9s %10s %10s %7s" % ("kernel", "launches", "avg us", "total ms", "share"))
for k, v in sorted(d.items(), key=lambda kv: -sum(kv[1])):
    print("%-92s %9d %10.1f %10.2f %6.1f%%" % (k, len(v), sum(v) / len(v) / 1e3, sum(v) / 1e6, 100.0 * sum(v) / busy))
