"""Per (kernel, grid size) averages and per-queue gaps of a rocprofv3 kernel trace:
the launches of one kernel at different grids (the row chains' sizes, N = 96 / 192 / paired) are kept
apart, which the --stats table does not do; the first third of the trace (plan finalize, warm-up) is
dropped.  Per queue: busy against wall time and the gap before each kernel.
usage: python tools/trace_by_grid.py <kernel_trace.csv>"""
import collections, csv, re, sys
rows = list(csv.DictReader(open(sys.argv[1])))
cols = rows[0].keys()
print("columns:", ",".join(cols))
def pick(*names):
    for n in names:
        if n in cols:
            return n
    return None
cg = pick("Grid_Size_X", "Grid_Size"); cw = pick("Workgroup_Size_X", "Workgroup_Size"); cq = pick("Queue_Id"); cs = pick("Stream_Id")
def short(n):
    n = re.sub(r"^void ", "", n)
    n = n.replace("sd::", "").replace("(anonymous namespace)::", "")
    return n.split("(")[0][:80]
ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), int(r[cg]) // max(int(r[cw]), 1) if cg and cw else 0,
             (r.get(cq, ""), r.get(cs, ""))) for r in rows)
# drop the first third (warmup, plan finalize)
ks = ks[len(ks) // 3:]
per = collections.defaultdict(list)
for s, e, n, g, q in ks:
    per[(n, g)].append(e - s)
tot = sum(sum(v) for v in per.values())
print(f"{'kernel':82s} {'wgs':>6s} {'count':>7s} {'avg us':>8s} {'min us':>8s} {'share':>6s}")
for (n, g), v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
    print(f"{n:82s} {g:6d} {len(v):7d} {sum(v)/len(v)/1e3:8.2f} {min(v)/1e3:8.2f} {100*sum(v)/tot:5.1f}%")
# per queue / stream: gap between consecutive kernels of one queue (dependent kernels of one chain)
byq = collections.defaultdict(list)
for k in ks:
    byq[k[4]].append(k)
for q, v in sorted(byq.items()):
    if len(v) < 100:
        continue
    gaps = sorted(v[i][0] - v[i - 1][1] for i in range(1, len(v)))
    gaps_s = [g for g in gaps if g < 50000]
    busy = sum(e - s for s, e, *_ in v)
    wall = v[-1][1] - v[0][0]
    print(f"queue/stream {q}: {len(v)} kernels, busy {busy/1e6:.1f} ms of {wall/1e6:.1f} ms wall, gap median {gaps[len(gaps)//2]/1e3:.2f} us, "
          f"mean(<50us) {sum(gaps_s)/max(len(gaps_s),1)/1e3:.2f} us, p10 {gaps[len(gaps)//10]/1e3:.2f}, p90 {gaps[9*len(gaps)//10]/1e3:.2f}")
    gb = collections.defaultdict(list)
    for i in range(1, len(v)):
        gb[v[i][2]].append(v[i][0] - v[i - 1][1])
    for n, g in sorted(gb.items(), key=lambda kv: -len(kv[1]))[:8]:
        g.sort()
        print(f"    gap before {n[:70]:70s} n={len(g):6d} median {g[len(g)//2]/1e3:6.2f} us")
