"""RPMMs inference throughput at 401 x 401 (side benchmark; bench.py measures the stage-1 headline).

usage: python scratch/rpmms_bench.py [--per-step 25,1] [--steps 20] [--warmup 5] [--repeats 5]

Per episodes-per-step one JSON line: ms of the captured ``lowres`` step (hipGraph replay, Wgen weights, pinned initial mu) of
RPMMs and, in the same process and alternating with it, of CANet with a zero history -- RPMMs runs CANet's trunk once and
CANet's tail three times, the ratio says what that costs -- as the median over ``--repeats`` timed blocks of ``--steps`` steps.
Then the three new entry points on the step's own operands, timed with events around ``--steps`` back-to-back calls (median
over the repeats): the EM entry (its eleven launches), the prob map and the proto sum (tap GEMV + sum), their share of the
step, and the EM's achieved bytes/s (per iteration both sides read the support features twice: E step and M step)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _model(kind, dev):
    from pemp_amd import synth
    if kind == "rpmms":
        from pemp_amd.networks import rpmms as m
        net = m.RPMMs(None)
    else:
        from pemp_amd.networks import canet as m
        net = m.CaNet(None)
    net.load_state_dict(synth.wgen_state_dict_for(net, m.WGEN_SEED))
    net = net.to(dev).eval()
    if kind == "rpmms":
        net.resample_pmm_init(torch.Generator().manual_seed(7))
        net.set_pmm_init({k: net.pmm_mu0[j0:j0 + k].t() for j0, k in ((0, 1), (1, 3), (4, 6))})      # one init for every step
    return net


def _timed_block(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def _event_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-step", default="25,1")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from pemp_amd import ops, synth
    dev = torch.device("cuda:0")
    nets = {k: _model(k, dev) for k in ("rpmms", "canet")}
    for per in [int(s) for s in args.per_step.split(",")]:
        b = synth.make_batch(list(range(1000, 1000 + per)), shot=1, height=401, width=401, out_hw=(401, 401))
        inputs = [torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img")]
        ms = {k: [] for k in nets}
        with torch.no_grad():
            for k, net in nets.items():
                for _ in range(args.warmup):
                    net.lowres_graphed(*inputs)
            for _ in range(args.repeats):                                    # the two models alternating
                for k, net in nets.items():
                    ms[k].append(_timed_block(lambda: net.lowres_graphed(*inputs), args.steps))
            step = {k: statistics.median(v) for k, v in ms.items()}
            # the new entry points on the step's own operands
            eng = nets["rpmms"]._engine_for(dev)["rpmms"]
            a = eng.arena
            f5, mu, x56 = eng.last_layer5, eng.last_mu, eng.last_layer56_in
            h, w = f5.shape[1:3]
            mask = a.get("rp_mask", (per, h, w, 1)).view(per, h, w)
            work = a.get("rp_em_work", (ops.rpmms_em_work_floats(per, h, w, 256),))
            base, taps = a.get("rp_base", (per, h, w, 256)), a.get("rp_T", (per, ops.RPMMS_COLS, 9, 256))
            mu2 = torch.empty_like(mu)
            calls = {"em": lambda: ops.rpmms_em(f5[:per], mask, nets["rpmms"].pmm_mu0, out=mu2, work=work),
                     "prob_map": lambda: ops.rpmms_prob_map(f5[per:], mu, x56),
                     "proto_sum": lambda: ops.rpmms_proto_sum(eng.wz, mu, base, eng.b55, x56[..., :256], dil=eng.dil55, taps=taps)}
            kern = {}
            for name, fn in calls.items():
                for _ in range(args.warmup):
                    fn()
                kern[name] = statistics.median(_event_ms(fn, args.steps) for _ in range(args.repeats))
        em_bytes = 10 * 2 * 2 * per * h * w * 256 * 4
        new = sum(kern.values())
        print(json.dumps({"episodes_per_step": per, "rpmms_ms_per_step": round(step["rpmms"], 3),
                          "rpmms_episodes_per_s": round(1e3 * per / step["rpmms"], 2), "canet_ms_per_step": round(step["canet"], 3),
                          "canet_episodes_per_s": round(1e3 * per / step["canet"], 2),
                          "rpmms_over_canet": round(step["rpmms"] / step["canet"], 3),
                          "ms_per_call": {k: round(v, 4) for k, v in kern.items()},
                          "share_of_step": {k: round(v / step["rpmms"], 4) for k, v in kern.items()},
                          "new_kernels_share_of_step": round(new / step["rpmms"], 4),
                          "em_feature_bytes": em_bytes, "em_tb_per_s": round(em_bytes / (kern["em"] * 1e-3) / 1e12, 3),
                          "spread_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()}}), flush=True)


if __name__ == "__main__":
    main()
