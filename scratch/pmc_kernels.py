"""counter_collection.csv files of `rocprofv3 --pmc ...` runs -> per kernel (template arguments kept, so one line per tile variant):
dispatches and the mean of every counter, plus SQ_INSTS_VALU / SQ_INSTS_MFMA where both were collected.
python3 scratch/pmc_kernels.py <rocprofv3 output dir> [<kernel-name substring>]"""
import collections
import csv
import glob
import sys

d = sys.argv[1]
sub = sys.argv[2] if len(sys.argv) > 2 else "conv_dma2"
acc = collections.OrderedDict()
for f in sorted(glob.glob(d + "/**/*counter_collection.csv", recursive=True)):
    for r in csv.DictReader(open(f)):
        k = r["Kernel_Name"].split("(")[0].replace("void pemp::", "").replace("pemp::", "")
        if sub not in k:
            continue
        c = acc.setdefault(k, collections.OrderedDict()).setdefault(r["Counter_Name"], [])
        c.append(float(r["Counter_Value"]))
for k, cs in acc.items():
    mean = {n: sum(v) / len(v) for n, v in cs.items()}
    line = " ".join(f"{n}={v:.4g}" for n, v in mean.items())
    if "SQ_INSTS_VALU" in mean and mean.get("SQ_INSTS_MFMA"):
        line += f" VALU/MFMA={mean['SQ_INSTS_VALU'] / mean['SQ_INSTS_MFMA']:.2f}"
    print(f"{k}\n    n={len(next(iter(cs.values())))} {line}")
