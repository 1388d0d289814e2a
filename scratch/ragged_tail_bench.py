"""The ragged tails against the per-size loop they replace in the evaluators: 25 images at 51 x 51, 25 label sizes (side
benchmark; bench.py measures the headline and is not involved).

usage: python scratch/ragged_tail_bench.py [--images 25] [--classes 5] [--rounds 5] [--block-s 0.4]

One JSON line per comparison, the sides alternated in one process (``bank_bench.alternate``: warm sides, ``rounds`` rounds of
about ``block-s`` seconds per side between two device synchronisations, median ms and spread).  Both sides are
``ops.tail_rows`` on the same operands, with ``ops.RAGGED_TAIL`` off (the loop: per distinct size a blocking index upload, a
gather of the predictions, a concatenation of the labels, one fixed-size launch pair, a scatter of the rows) and on (one
descriptor upload, one concatenation, one launch pair):
  mixed    25 DISTINCT PASCAL-shaped label sizes (longer side 500): what a step on real data holds at the most
  equal    25 times 401 x 401: the synthetic rounds' case; a third side, ``ops.eval_tail`` / ``ops.nway_tail`` on the stacked
           target, shows what the ragged launch costs against the fixed-size one
each for the stage-1 eval tail and for the N-way tail over ``classes`` classes, with the labels on the device (as the parent's
evaluators held them) and, for ``mixed``, on the host (the evaluators now leave them there: the ragged side uploads each into its
place in the packed target, the loop uploads each and concatenates per size).
``ms_per_call`` is wall time per call, host work included.  ``tail_kernels_us`` is device time between HIP events recorded
around the library's tail launches alone, summed per call: it leaves out the loop's gathers, concatenations and scatters."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from bank_bench import alternate  # noqa: E402

LOW = 51


def pascal_shaped(n):
    """``n`` distinct sizes with the longer side 500, landscape and portrait, around ``synth.QUERY_SIZES``."""
    wide = [(333 + 7 * i, 500) for i in range((n + 1) // 2)]
    tall = [(500, 333 + 7 * i) for i in range(n // 2)]
    return [s for pair in zip(wide, tall) for s in pair] + wide[len(tall):]


class TimedTails:
    """Stands in for the library handle: HIP events around every tail launch, on the current stream."""

    def __init__(self, lib):
        self.lib, self.pairs = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if "_tail_" not in name or not name.endswith("_f32"):
            return fn

        def timed(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            self.pairs.append((e0, e1))
            return rc
        return timed


def tail_kernels_us(fn, calls=20):
    """Median over ``calls`` calls of the summed event time of the call's tail launches, in microseconds."""
    from pemp_amd import _lib
    real, load = _lib.load(), _lib.load
    proxy = TimedTails(real)
    _lib.load = lambda: proxy
    try:
        out = []
        for _ in range(calls):
            proxy.pairs = []
            fn()
            torch.cuda.synchronize()
            out.append(1e3 * sum(a.elapsed_time(b) for a, b in proxy.pairs))
        launches = len(proxy.pairs)
    finally:
        _lib.load = load
    return round(statistics.median(out), 1), launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=25)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block-s", type=float, default=0.4)
    args = ap.parse_args()
    from pemp_amd import ops
    dev = torch.device("cuda:0")
    n, K = args.images, args.classes
    g = torch.Generator().manual_seed(1)
    preds = {"eval": torch.randn(n, 2, LOW, LOW, generator=g).to(dev), "nway": torch.randn(n, K, 2, LOW, LOW, generator=g).to(dev)}
    want = [i % K for i in range(n)]
    want_dev = torch.tensor(want, dtype=torch.int32, device=dev)

    def with_switch(on, fn):
        def run():
            ops.RAGGED_TAIL = on
            return fn()
        return run

    for config, sizes in (("mixed", pascal_shaped(n)), ("equal", [(401, 401)] * n)):
        host = [torch.randint(0, 2, (1, ho, wo), generator=g) for ho, wo in sizes]
        for lab in host:
            lab[:, : lab.shape[1] // 8] = 255
        device = [lab.to(dev) for lab in host]
        stacked = torch.cat(device) if config == "equal" else None
        for tail in ("eval", "nway"):
            pred, w = preds[tail], (want if tail == "nway" else None)
            for where, labels in (("device", device), ("host", host)):
                if where == "host" and config == "equal":
                    continue
                ws = {}
                call = lambda: ops.tail_rows(pred, labels, want=w, ws_cache=ws)
                sides = {"loop": with_switch(False, call), "ragged": with_switch(True, call)}
                if stacked is not None:
                    if tail == "eval":
                        sides["fixed"] = lambda: ops.eval_tail(pred, stacked, ws_cache=ws)[1]
                    else:
                        sides["fixed"] = lambda: ops.nway_tail(pred, target=stacked, want=want_dev, ws_cache=ws)[2]
                rows = {name: fn().cpu() for name, fn in sides.items()}
                same = all(torch.equal(r, rows["loop"]) for r in rows.values())
                ms, reps = alternate(sides, args.rounds, args.block_s)
                row = {"what": "ragged_tail", "config": config, "tail": tail, "labels_on": where, "images": n,
                       "distinct_sizes": len(set(sizes)), "classes": K if tail == "nway" else 1, "low": [LOW, LOW],
                       "Mpixels": round(sum(ho * wo for ho, wo in sizes) / 1e6, 2), "rows_identical": same}
                for name, fn in sides.items():
                    v = ms[name]
                    us, launches = tail_kernels_us(fn)
                    row[name] = {"ms_per_call_median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                                 "calls_per_round": reps[name], "tail_kernels_us": us, "tail_launch_pairs": launches}
                for other in [s for s in sides if s != "ragged"]:
                    row[f"{other}_over_ragged_median"] = round(statistics.median(ms[other]) / statistics.median(ms["ragged"]), 2)
                    row[f"{other}_over_ragged_range"] = [round(min(ms[other]) / max(ms["ragged"]), 2),
                                                         round(max(ms[other]) / min(ms["ragged"]), 2)]
                print(json.dumps(row), flush=True)
    ops.RAGGED_TAIL = True


if __name__ == "__main__":
    main()
