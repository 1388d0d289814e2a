"""``--trunk-precision {f32_chain,split3,both}`` of the three head-training side benchmarks (canet / pfenet / rpmms
_train_bench.py).  ``both``: one trainer per precision in ONE process, warmed up, then ``--rounds`` rounds that alternate the two
(``--steps`` steps each, host clock around steps that end in a synchronise); every round's rates are printed -- their spread is
the run-to-run spread -- and the summary gives the median rate of each and the split3 / f32_chain ratio per round."""
import json
import statistics
import time

import torch

CHOICES = ("f32_chain", "split3", "both")


def add_argument(ap):
    ap.add_argument("--trunk-precision", choices=CHOICES, default="f32_chain",
                    help="frozen-trunk convs: the fp32 chain (default), the split3 family, or both alternated in one process")


def alternate(model, steps, n_steps, warmup, rounds, bs):
    """``steps``: {precision: callable that runs one train step and returns its loss}."""
    for fn in steps.values():
        for _ in range(warmup):                                    # picks every conv / wgrad variant, fills the workspaces
            fn()
    rates = {k: [] for k in steps}
    for r in range(rounds):
        for name, fn in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                loss = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rates[name].append(bs * n_steps / dt)
            print(json.dumps({"model": model, "round": r, "trunk_precision": name, "ms_per_step": round(1e3 * dt / n_steps, 3),
                              "episodes_per_s": round(rates[name][-1], 2), "loss": round(float(loss), 5)}), flush=True)
    out = {"model": model, "bs": bs, "steps": n_steps, "rounds": rounds}
    for name, v in rates.items():
        out[name] = {"median_episodes_per_s": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    if "split3" in rates and "f32_chain" in rates:
        ratio = [a / b for a, b in zip(rates["split3"], rates["f32_chain"])]
        out["split3_over_f32_chain"] = {"median": round(statistics.median(ratio), 4), "min": round(min(ratio), 4), "max": round(max(ratio), 4)}
    print(json.dumps({"trunk_precision_ab": out}), flush=True)
    return out
