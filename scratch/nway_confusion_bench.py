"""The N-way confusion tails against what the label tails offer for the same table: ``ops.nway_tail`` / ``ops.nway_tail_ragged``
followed by one ``torch.bincount`` per image (side benchmark; bench.py measures the headline and is not involved).

usage: python scratch/nway_confusion_bench.py [--images 25] [--classes 5] [--rounds 5] [--block-s 0.4] [--bias 1.5]

One JSON line per configuration, the sides alternated in one process (``bank_bench.alternate``: warm sides, ``rounds`` rounds of
about ``block-s`` seconds per side between two device synchronisations, median ms and spread):
  equal    25 times 401 x 401, the fixed-size calls
  mixed    25 DISTINCT PASCAL-shaped label sizes (longer side 500), the ragged calls
The sides, all on device tensors and all giving the same int64 [N,K+1,K+1] tables (checked before the timing):
  confusion          ``ops.nway_confusion(_ragged)``, no label map stored
  confusion_labels   the same call with ``want_labels``
  tail_bincount      ``ops.nway_tail(_ragged)`` for the labels, then per image ``torch.bincount(target * (K + 1) + labels)`` with
                     the ignored pixels sent to a spare bin -- the second pass over full-resolution data that the confusion call
                     saves
The logits are random with the background plane raised by ``bias``, the targets mostly 0: most pixels fall into bin (0,0), the
case the kernel counts in registers.  ``ms_per_call`` is wall time per call, host work included; ``kernels_us`` is device time
between HIP events around the library's launches alone (the confusion launch with its
memset, or the label tail without the bincounts)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from bank_bench import alternate  # noqa: E402
from ragged_tail_bench import LOW, pascal_shaped  # noqa: E402


class Timed:
    """Stands in for the library handle: HIP events around every N-way launch entry, on the current stream."""

    def __init__(self, lib):
        self.lib, self.pairs = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("pemp_nway_") or not name.endswith("_f32"):
            return fn

        def timed(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            self.pairs.append((e0, e1))
            return rc
        return timed


def kernels_us(fn, calls=20):
    """Median over ``calls`` calls of the summed event time of the call's library launches, in microseconds."""
    from pemp_amd import _lib
    real, load = _lib.load(), _lib.load
    proxy = Timed(real)
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
    ap.add_argument("--bias", type=float, default=1.5)
    args = ap.parse_args()
    from pemp_amd import ops
    dev = torch.device("cuda:0")
    n, K = args.images, args.classes
    bins = (K + 1) ** 2
    g = torch.Generator().manual_seed(1)
    pred = torch.randn(n, K, 2, LOW, LOW, generator=g)
    pred[:, :, 0] += args.bias
    pred = pred.to(dev)

    def bincounts(labels, targets):
        out = []
        for lab, t in zip(labels, targets):
            idx = torch.where(t == 255, bins, t * (K + 1) + lab.long())
            out.append(torch.bincount(idx.flatten(), minlength=bins + 1)[:bins].view(K + 1, K + 1))
        return torch.stack(out)

    for config, sizes in (("equal", [(401, 401)] * n), ("mixed", pascal_shaped(n))):
        targets = []
        for ho, wo in sizes:
            t = torch.randint(1, K + 1, (ho, wo), generator=g)
            t[torch.rand((ho, wo), generator=g) < 0.8] = 0
            t[: ho // 8] = 255
            targets.append(t.to(dev))
        ws = {}
        if config == "equal":
            stacked = torch.stack(targets)
            sides = {"confusion": lambda: ops.nway_confusion(pred, stacked, ws_cache=ws)[0],
                     "confusion_labels": lambda: ops.nway_confusion(pred, stacked, want_labels=True, ws_cache=ws)[0],
                     "tail_bincount": lambda: bincounts(ops.nway_tail(pred, sizes[0], ws_cache=ws)[0], stacked)}
        else:
            sides = {"confusion": lambda: ops.nway_confusion_ragged(pred, targets, ws_cache=ws)[0],
                     "confusion_labels": lambda: ops.nway_confusion_ragged(pred, targets, want_labels=True, ws_cache=ws, views=False)[0],
                     "tail_bincount": lambda: bincounts(ops.nway_tail_ragged(pred, sizes, ws_cache=ws)[0], targets)}
        tables = {name: fn().cpu() for name, fn in sides.items()}
        same = all(torch.equal(t, tables["tail_bincount"]) for t in tables.values())
        total = tables["confusion"].sum().item()
        ms, reps = alternate(sides, args.rounds, args.block_s)
        row = {"what": "nway_confusion", "config": config, "images": n, "distinct_sizes": len(set(sizes)), "classes": K,
               "low": [LOW, LOW], "Mpixels": round(sum(ho * wo for ho, wo in sizes) / 1e6, 2), "tables_identical": same,
               "share_in_bin_00": round(tables["confusion"][:, 0, 0].sum().item() / total, 3)}
        for name, fn in sides.items():
            v = ms[name]
            us, launches = kernels_us(fn)
            row[name] = {"ms_per_call_median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                         "calls_per_round": reps[name], "kernels_us": us, "library_calls": launches}
        for other in ("confusion_labels", "tail_bincount"):
            row[f"{other}_over_confusion_median"] = round(statistics.median(ms[other]) / statistics.median(ms["confusion"]), 2)
            row[f"{other}_over_confusion_range"] = [round(min(ms[other]) / max(ms["confusion"]), 2),
                                                    round(max(ms[other]) / min(ms["confusion"]), 2)]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
