"""bench.py's `single_episode` figure with its checks spelled out (GPU).  The four sub-runs of that figure -- split-K allowed / exact
variants, one lane / four lanes in flight -- each evaluate the same 120 one-episode steps; this prints, per sub-run, the episodes
whose statistics row is non-finite or has a non-positive pixel count (column 1), and compares every row with the one-lane row of
the same variant family (the lanes run the same kernels on the same inputs: rows must be bit-identical).

    python3 scratch/single_episode_check.py [--repeat R]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from pemp_amd.entry.pemp_stage1 import Evaluator  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=2, help="four-lane runs per variant family")
    ap.add_argument("-n", type=int, default=120)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    net, _ = bench.build_model(dev, "stage1", 1)
    pool = bench.episode_pool(dev, 1, 1, 0, n_groups=5, dataset="PASCAL")
    eps = [((p["sup_img"], p["sup_mask"], p["qry_img"]), p["qry_mask"][None]) for p in pool]
    bad_total = 0

    def run(lanes, splitk):
        ev = Evaluator(net, device=dev, lanes=lanes, splitk=splitk)
        ev.test_steps_device([eps[i % len(eps)] for i in range(2 * len(eps) * lanes)])
        torch.cuda.synchronize()
        rows = ev.test_steps_device([eps[i % len(eps)] for i in range(args.n)])
        torch.cuda.synchronize()
        return rows.cpu().numpy()

    for splitk in (True, False):
        one = run(1, splitk)
        runs = [("1 lane", one)] + [(f"4 lanes #{r}", run(4, splitk)) for r in range(args.repeat)]
        for tag, st in runs:
            nonfin = np.where(~np.isfinite(st).all(1))[0]
            nonpos = np.where(~(st[:, 1] > 0))[0]
            diff = np.where((st != one).any(1) & np.isfinite(st).all(1))[0] if st is not one else np.array([], int)
            bad = len(nonfin) + len(nonpos) + len(diff)
            bad_total += bad
            print(f"splitk={int(splitk)} {tag}: non-finite rows {nonfin.tolist()[:12]} (cols {sorted(set(np.where(~np.isfinite(st[nonfin]))[1].tolist()))}), "
                  f"col1 <= 0 rows {nonpos.tolist()[:12]}, rows != 1-lane {diff.tolist()[:12]}" + ("" if bad else "  ok"), flush=True)
            for i in list(nonfin[:3]) + list(nonpos[:3]) + list(diff[:3]):
                print(f"    episode {i} (lane {i % 4}): {st[i].tolist()}\n    1-lane:               {one[i].tolist()}", flush=True)
    print("ALL OK" if bad_total == 0 else f"BAD ROWS: {bad_total}")


if __name__ == "__main__":
    main()
