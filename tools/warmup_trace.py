"""The warm-up stretch of every pass, from a rocprofv3 kernel trace of bench.py (tools/ktrace.sh writes one):

    python3 tools/warmup_trace.py DIR            (DIR: the directory given to rocprofv3 -d)

Per pass (a pass ends with its longest kernel, the last level's pruned launch): every k_null_ie<M,L> launch with the
level it belongs to (the n-th launch of a pass is level n), k_fill_rec_segs, and the time from the end of the last
k_stats_ie2 to the start of the last level's pruned kernel -- the stretch in which nothing else is left to run."""
import csv
import glob
import sys

if len(sys.argv) != 2:
    sys.exit(__doc__)
d = sys.argv[1]
f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[-1]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
longest = max(rows, key=dur)["Kernel_Name"]
ends = [i for i, r in enumerate(rows) if r["Kernel_Name"] == longest]
print(f"{f}: {len(rows)} kernels, {len(ends)} passes; the last level's pruned kernel is {longest.split('(')[0][:60]}")
lo = 0
for n, hi in enumerate(ends):
    step = rows[lo:hi + 1]
    lo = hi + 1
    warm = [r for r in step if "k_null_ie<" in r["Kernel_Name"]]
    fill = [r for r in step if "k_fill_rec_segs" in r["Kernel_Name"]]
    stats = [r for r in step if "k_stats_ie2" in r["Kernel_Name"]]
    big = step[-1]
    line = f"pass {n}: pruned kernel {dur(big) / 1e6:.3f} ms; k_null_ie sum {sum(map(dur, warm)) / 1e6:.3f} ms:"
    for lvl, r in enumerate(warm, 1):
        line += f" [{lvl}] {r['Kernel_Name'].split('(')[0].split('k_null_ie')[-1]} {dur(r) / 1e3:.0f} us"
    line += "; k_fill_rec_segs " + " ".join(f"{dur(r) / 1e3:.0f} us" for r in fill)
    if stats:
        line += f"; last k_stats_ie2 end -> pruned kernel start {(int(big['Start_Timestamp']) - int(stats[-1]['End_Timestamp'])) / 1e3:.0f} us"
    print(line)
