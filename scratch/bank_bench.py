"""Prototype banks against whole episodes: stage 1, ResNet-50, 401 x 401, 25 queries per step (side benchmark; bench.py
measures the headline and is not involved).

usage: python scratch/bank_bench.py [--shots 1,5] [--queries 25] [--rounds 5] [--block-s 0.8]
       python scratch/bank_bench.py --kernels [--iters 50]          (to be run under rocprofv3 --kernel-trace --stats)

Default mode, one JSON line per comparison:
  episode_vs_bank   the captured episode step (``lowres_graphed``: S supports + 1 query per episode through the trunk) against the
                    captured bank step (``segment_graphed`` with an index: the queries alone; the K = 5 classes enrolled before)
  all_vs_indexed    one all-classes step (every query against the 5 classes: one trunk pass, one cosine launch) against five
                    indexed steps (one per class: five trunk passes)
Timing is steady state: both sides warmed up (graphs captured, kernel variants picked), then ``rounds`` rounds in which the two
sides alternate, each running for about ``block-s`` seconds per round between two device synchronisations; per side the median
ms per step over the rounds and their spread (min .. max) are reported.

``--kernels``: the cosine launches alone on a [25, 51, 51, 512] feature map -- ``iters`` all-classes bank launches (K = 5) and
``iters`` x 5 launches of the episode kernel -- for a kernel trace (pemp::j8::cosine_bank_mfma_kernel / cosine_mfma_kernel)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

K = 5


def alternate(sides, rounds, block_s):
    """``sides``: {name: callable running ONE step}.  -> {name: [ms per step of every round]}."""
    reps = {}
    for name, fn in sides.items():                 # size the blocks on warm sides
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps[name] = max(3, int(block_s / max((time.perf_counter() - t0) / 3, 1e-6)))
    ms = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps[name]):
                fn()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / reps[name])
    return ms, reps


def report(what, ms, reps, base, other, extra):
    row = {"what": what, **extra}
    for name in (base, other):
        v = ms[name]
        row[name] = {"ms_per_step_median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                     "steps_per_round": reps[name], "seconds_timed": round(sum(v) * reps[name] / 1e3, 2)}
    row["speedup_median"] = round(statistics.median(ms[base]) / statistics.median(ms[other]), 3)
    row["speedup_range"] = [round(min(ms[base]) / max(ms[other]), 3), round(max(ms[base]) / min(ms[other]), 3)]
    print(json.dumps(row), flush=True)


def kernels(iters):
    from pemp_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    q = torch.randn(25, 51, 51, 512, generator=g).to(dev)
    bank = torch.randn(K, 6, 512, generator=g).to(dev)
    per_class = [bank[k:k + 1].expand(25, 6, 512).contiguous() for k in range(K)]
    pred_b = torch.empty(25, K, 2, 51, 51, device=dev)
    resp_b = torch.empty(25, K, 51, 51, dtype=torch.uint8, device=dev)
    pred_e = torch.empty(25, 2, 51, 51, device=dev)
    resp_e = torch.empty(25, 51, 51, dtype=torch.uint8, device=dev)
    for _ in range(iters):
        ops.cosine_bank_max(q, bank, 20.0, want_resp=True, pred=pred_b, resp=resp_b)
    for _ in range(iters):
        for k in range(K):
            ops.cosine_proto_max(q, per_class[k], 20.0, want_resp=True, pred=pred_e, resp=resp_e)
    torch.cuda.synchronize()
    print(json.dumps({"what": "kernels", "iters": iters, "bank_launches": iters, "episode_kernel_launches": iters * K}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", default="1,5")
    ap.add_argument("--queries", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block-s", type=float, default=0.8)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if args.kernels:
        return kernels(args.iters)
    from pemp_amd import synth
    from pemp_amd.networks import pemp_stage1 as m
    dev = torch.device("cuda:0")
    net = m.PEMPStage1(None)
    net.load_state_dict(synth.wgen_state_dict_for(net))
    net = net.to(dev).eval()
    n = args.queries
    for shot in [int(s) for s in args.shots.split(",")]:
        b = synth.make_batch(list(range(1000, 1000 + n)), shot=shot, height=401, width=401, out_hw=(401, 401))
        sup, msk, qry = (torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img"))
        queries = qry[:, 0].contiguous()
        index = [i % K for i in range(n)]
        with torch.no_grad():
            bank = net.enroll(sup[:K], msk[:K])
            sides = {"episode": lambda: net.lowres_graphed(sup, msk, qry), "bank": lambda: net.segment_graphed(bank, queries, index=index)}
            ms, reps = alternate(sides, args.rounds, args.block_s)
        report("episode_vs_bank", ms, reps, "episode", "bank",
               {"shot": shot, "queries_per_step": n, "classes": K, "trunk_images_per_step": {"episode": n * (shot + 1), "bank": n}})
        if shot == 1:
            with torch.no_grad():
                per_class = [[k] * n for k in range(K)]

                def five():
                    for idx in per_class:
                        net.segment_graphed(bank, queries, index=idx)
                sides = {"five_indexed": five, "all_classes": lambda: net.segment_graphed(bank, queries)}
                ms, reps = alternate(sides, args.rounds, args.block_s)
            report("all_vs_indexed", ms, reps, "five_indexed", "all_classes", {"queries_per_step": n, "classes": K})


if __name__ == "__main__":
    main()
