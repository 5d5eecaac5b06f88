"""profiles/redo_tail_overlap.py <kernel_trace.csv> -- from one rocprofv3 kernel trace of bench.py: the kernels of a
step's tail by (name, grid) -- the redo scan and the redo select are their kernels' small-grid launches -- and, per
step, whether select_wave_kernel<16,2> ran beside <8,4>: the two durations against the span from the first start
to the last end."""
import collections
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
short = lambda n: n.replace("void ", "").replace("expann::", "").split("(")[0]
groups = collections.defaultdict(list)
for r in rows:
    name = short(r["Kernel_Name"])
    if not any(s in name for s in ("select_", "scan_gemm_i8w", "scan_gemm_f16x", "redo_compact", "gather_logs", "sum_u32")):
        continue
    grid = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
    groups[(name, grid)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
print("%-64s %9s %6s %9s" % ("kernel", "grid", "calls", "avg us"))
for (name, grid), d in sorted(groups.items(), key=lambda kv: -sum(kv[1])):
    d = d[len(d) // 5:]  # (the first fifth: warm-up steps)
    print("%-64s %9d %6d %9.1f" % (name[:64], grid, len(d), sum(d) / len(d)))

w8 = [r for r in rows if "select_wave_kernel<8, 4" in r["Kernel_Name"]]
w16 = [r for r in rows if "select_wave_kernel<16, 2" in r["Kernel_Name"]]
pairs = []
for a in w8:
    s8, e8 = int(a["Start_Timestamp"]), int(a["End_Timestamp"])
    nxt = [b for b in w16 if int(b["End_Timestamp"]) > s8]
    if not nxt:
        continue
    b = nxt[0]
    s16, e16 = int(b["Start_Timestamp"]), int(b["End_Timestamp"])
    if s16 - e8 > 1_000_000:
        continue  # (not the same step)
    pairs.append(((e8 - s8) / 1e3, (e16 - s16) / 1e3, (max(e8, e16) - min(s8, s16)) / 1e3, (s16 - s8) / 1e3))
pairs = pairs[len(pairs) // 5:]
if pairs:
    n = len(pairs)
    m = [sum(p[i] for p in pairs) / n for i in range(4)]
    print("select stages over %d steps: <8,4> %.1f us, <16,2> %.1f us, sum %.1f us, span first start -> last end %.1f us, "
          "<16,2> starts %.1f us after <8,4>" % (n, m[0], m[1], m[0] + m[1], m[2], m[3]))
else:
    print("select stages: no step ran both <8,4> and <16,2>")
