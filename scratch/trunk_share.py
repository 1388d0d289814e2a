"""kernel_stats.csv of ``rocprofv3 --kernel-trace --stats --output-format csv -- python scratch/<model>_train_bench.py ...`` -> the
share of the process's kernel time that the frozen trunk's convs take: the conv_dma2 kernels with the statistics epilogue (template
argument EPI = 1: every non-stem trunk conv of a head trainer, plus RPMMs' one head conv in front of a BatchNorm), split by family
(the last template argument: S3), next to all other convs, the BatchNorm kernels and the rest.

usage: python scratch/trunk_share.py <kernel_stats.csv> [...]"""
import csv
import json
import re
import sys


def classify(name):
    m = re.search(r"conv_dma2_kernel<([^>]*)>", name)
    if m:
        a = [t.strip() for t in m.group(1).split(",")]
        a += ["false"] * (11 - len(a))
        if a[5] == "1":
            return "trunk_stats_conv_split3" if a[10] in ("true", "1") else "trunk_stats_conv_f32_chain"
        return "other_conv"
    if re.search(r"conv_|wgrad", name):
        return "other_conv"
    if re.search(r"bn_|batchnorm|colsum", name):
        return "batchnorm"
    return "rest"


def main():
    for path in sys.argv[1:]:
        tot = {}
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
                k = classify(row.get("Name") or row.get("KernelName") or "")
                tot[k] = tot.get(k, 0.0) + ns
        s = sum(tot.values()) or 1.0
        print(json.dumps({"file": path, "kernel_ms": round(s / 1e6, 2),
                          "share": {k: round(v / s, 4) for k, v in sorted(tot.items())}}))


if __name__ == "__main__":
    main()
