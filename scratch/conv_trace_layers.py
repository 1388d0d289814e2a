"""kernel_trace.csv of `rocprofv3 --kernel-trace` on bench.py (one engine lane) -> conv time per step, and per conv launch POSITION
in the step (the layers run in a fixed order, so a position is one layer): mean us over the last `steps` steps, grid, workgroup
size, kernel.  python3 scratch/conv_trace_layers.py trace.csv <conv launches per step> [steps]"""
import collections
import csv
import sys

trace, per_step = sys.argv[1], int(sys.argv[2])
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
conv = [r for r in rows if any(k in r["Kernel_Name"] for k in ("conv_dma", "conv_igemm", "conv_stem_pool", "conv_panel", "conv_row3", "conv_ring"))][-steps * per_step:]
dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
pos = collections.defaultdict(list)
for i, r in enumerate(conv):
    pos[i % per_step].append(r)
print(f"conv launches per step {per_step}, steps {steps}: conv {sum(map(dur, conv)) / steps / 1e3:.3f} ms per step")
print(f"{'pos':>3} {'mean us':>9} {'grid':>8} {'wg':>4}  kernel")
for p in range(per_step):
    rs = pos[p]
    r = rs[-1]
    name = r["Kernel_Name"].split("(")[0].replace("void pemp::", "").replace("pemp::", "")
    g = r.get("Grid_Size", r.get("Grid_Size_X", "")); wg = r.get("Workgroup_Size", r.get("Workgroup_Size_X", ""))
    print(f"{p:>3} {sum(map(dur, rs)) / len(rs):9.1f} {g:>8} {wg:>4}  {name}")
