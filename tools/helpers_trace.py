"""The per-join helper kernels of the last pass, from a rocprofv3 kernel trace of bench.py (tools/ktrace.sh writes one):

    python3 tools/helpers_trace.py DIR            (DIR: the directory given to rocprofv3 -d)

A pass ends with its longest kernel (the last level's pruned launch).  Of the last pass: every k_range_union, k_expand,
inspector (k_stats*) and k_fill_rec_segs launch and every fill kernel (hipMemsetAsync) on the queue of k_range_union, with
queue, start and end in us from the pass's first kernel, and the gap to the end of its predecessor on the same queue (a
negative gap would mean the two overlapped); then the per-pass sums of every pass, the stretch (end of the last inspector
to the start of the pruned kernel) and the chain (end of the last-but-one level's last inspector to the start of the last
level's first)."""
import csv
import glob
import sys

if len(sys.argv) != 2:
    sys.exit(__doc__)
d = sys.argv[1]
f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[-1]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
t0 = lambda r: int(r["Start_Timestamp"])
t1 = lambda r: int(r["End_Timestamp"])
dur = lambda r: t1(r) - t0(r)
name = lambda r: r["Kernel_Name"].split("(")[0]
queue = lambda r: r.get("Queue_Id", "?")
longest = max(rows, key=dur)["Kernel_Name"]
ends = [i for i, r in enumerate(rows) if r["Kernel_Name"] == longest]
print(f"{f}: {len(rows)} kernels, {len(ends)} passes; the last level's pruned kernel is {name(rows[ends[-1]])[:60]}")
HELP = ("k_range_union", "k_expand", "k_fill_rec_segs")
is_insp = lambda r: "k_stats" in r["Kernel_Name"]
lo = 0
for n, hi in enumerate(ends):
    step = rows[lo:hi + 1]
    lo = hi + 1
    sums = {h: [0, 0] for h in HELP}
    for r in step:
        for h in HELP:
            if h in r["Kernel_Name"]:
                sums[h][0] += dur(r)
                sums[h][1] += 1
    insp = [r for r in step if is_insp(r)]
    big = step[-1]
    line = f"pass {n}: pruned kernel {dur(big) / 1e3:.0f} us, pass {(t1(big) - t0(step[0])) / 1e3:.0f} us;"
    line += "".join(f" {h} {v[0] / 1e3:.0f} us x{v[1]};" for h, v in sums.items())
    if insp:
        line += f" stretch {(t0(big) - t1(insp[-1])) / 1e3:.0f} us;"
        # levels: an expansion starts a join's inspection; the chain is the gap between the inspectors of the last two
        exp = [r for r in step if "k_expand" in r["Kernel_Name"]]
        if len(exp) >= 2:
            prev = [r for r in insp if t1(r) <= t0(exp[-1])]
            last = [r for r in insp if t0(r) >= t1(exp[-1])]
            if prev and last:
                line += f" chain {(t0(last[0]) - t1(prev[-1])) / 1e3:.0f} us"
    print(line)
    if n != len(ends) - 1:
        continue
    ru = [r for r in step if "k_range_union" in r["Kernel_Name"]]
    qs = {queue(r) for r in ru} | {queue(r) for r in step if "k_expand" in r["Kernel_Name"]}
    base = t0(step[0])
    last_end = {}
    print(f"{'kernel':46s} {'queue':>6s} {'start':>9s} {'end':>9s} {'us':>8s} {'gap to predecessor on queue':>28s}")
    for r in step:
        q = queue(r)
        fill = "fill" in r["Kernel_Name"].lower() and q in qs
        want = fill or is_insp(r) or any(h in r["Kernel_Name"] for h in HELP) or r is big
        if want:
            gap = f"{(t0(r) - last_end[q]) / 1e3:.1f}" if q in last_end else "-"
            print(f"{name(r)[:46]:46s} {q:>6s} {(t0(r) - base) / 1e3:9.1f} {(t1(r) - base) / 1e3:9.1f} {dur(r) / 1e3:8.1f} {gap:>28s}")
        last_end[q] = max(last_end.get(q, 0), t1(r))
