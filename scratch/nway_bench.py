"""The N-way tail against what it replaces: 401 x 401, 25 queries, K in {1, 5, 20} classes (side benchmark; bench.py measures the
headline and is not involved).

usage: python scratch/nway_bench.py [--classes 1,5,20] [--queries 25] [--rounds 5] [--block-s 0.4] [--inner 10]

One JSON line per comparison, the sides alternated in one process (``bank_bench.alternate``: warm sides, ``rounds`` rounds of
about ``block-s`` seconds per side between two device synchronisations, median ms and spread):
  nway_vs_composition   ``ops.nway_tail`` on pred [25,K,2,51,51] against ``ops.upsample_bilinear_ac`` over the 25 * K * 2 planes plus
                        the rule in torch on the full-resolution logits
  nway_vs_eval_tail     K = 1 only: ``ops.nway_tail`` against ``ops.eval_tail`` on the same operand (labels only, no target)
  nway_bytes            the kernel's own traffic -- labels, + margin, + target and statistics -- over its time, in GB/s
  labels_vs_segment     stage 1, ResNet-50, K = 5: a ``segment_labels`` step (eager and graphed) against a ``segment`` step
The kernel sides are ``inner`` launches replayed from a captured graph, so that a launch of some tens of microseconds is not
timed through the host's launch path; the figures are per launch."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from bank_bench import alternate, report  # noqa: E402

HO = WO = 401
LOW = 51


def replayed(fn, inner):
    """``inner`` calls of ``fn`` captured into one graph -> a callable that replays it."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(inner):
            fn()
    return graph.replay


def torch_rule(up):
    """The rule on full-resolution logits [N,K,2,Ho,Wo] as a caller would write it in torch (ties aside: max's order)."""
    m = up[:, :, 1] - up[:, :, 0]
    best, k = m.max(dim=1)
    return torch.where(best > 0, k + 1, torch.zeros_like(k)).to(torch.uint8)


def per_launch(ms, inner):
    return {k: [x / inner for x in v] for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", default="1,5,20")
    ap.add_argument("--queries", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block-s", type=float, default=0.4)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    from pemp_amd import ops, synth
    dev = torch.device("cuda:0")
    n, inner = args.queries, args.inner
    g = torch.Generator().manual_seed(1)
    target = torch.randint(0, 2, (n, HO, WO), generator=g).to(dev)
    npix = n * HO * WO
    with torch.no_grad():
        for K in [int(k) for k in args.classes.split(",")]:
            pred = torch.randn(n, K, 2, LOW, LOW, generator=g).to(dev)
            want = torch.arange(n, dtype=torch.int32, device=dev) % K
            ws = {}
            extra = {"queries": n, "classes": K, "out_hw": [HO, WO], "launches_per_replay": inner}
            sides = {"composition": replayed(lambda: torch_rule(ops.upsample_bilinear_ac(pred.view(n * K, 2, LOW, LOW), (HO, WO))
                                                                .view(n, K, 2, HO, WO)), inner),
                     "nway_tail": replayed(lambda: ops.nway_tail(pred, (HO, WO), ws_cache=ws), inner)}
            ms, reps = alternate(sides, args.rounds, args.block_s)
            report("nway_vs_composition", per_launch(ms, inner), reps, "composition", "nway_tail",
                   {**extra, "full_res_logits_MB": round(npix * K * 2 * 4 / 1e6, 1)})
            if K == 1:
                one = pred[:, 0].contiguous()
                sides = {"eval_tail": replayed(lambda: ops.eval_tail(one, None, out_hw=(HO, WO), ws_cache=ws), inner),
                         "nway_tail": replayed(lambda: ops.nway_tail(pred, (HO, WO), ws_cache=ws), inner)}
                ms, reps = alternate(sides, args.rounds, args.block_s)
                report("nway_vs_eval_tail", per_launch(ms, inner), reps, "eval_tail", "nway_tail", extra)
            sides = {"labels": replayed(lambda: ops.nway_tail(pred, (HO, WO), ws_cache=ws), inner),
                     "labels_margin": replayed(lambda: ops.nway_tail(pred, (HO, WO), want_margin=True, ws_cache=ws), inner),
                     "labels_margin_target": replayed(lambda: ops.nway_tail(pred, target=target, want=want, want_margin=True, ws_cache=ws),
                                                      inner)}
            ms, reps = alternate(sides, args.rounds, args.block_s)
            nbytes = {"labels": npix, "labels_margin": npix * 5, "labels_margin_target": npix * 13}
            row = {"what": "nway_bytes", **extra}
            for name, v in per_launch(ms, inner).items():
                med = statistics.median(v)
                row[name] = {"us_per_launch_median": round(1e3 * med, 2), "min": round(1e3 * min(v), 2), "max": round(1e3 * max(v), 2),
                             "MB": round(nbytes[name] / 1e6, 1), "GB_per_s": round(nbytes[name] / (med * 1e-3) / 1e9, 1)}
            print(json.dumps(row), flush=True)
        # the model step: stage 1, ResNet-50, K = 5 enrolled classes
        from pemp_amd.networks import pemp_stage1 as m
        K = 5
        net = m.PEMPStage1(None)
        net.load_state_dict(synth.wgen_state_dict_for(net))
        net = net.to(dev).eval()
        b = synth.make_batch(list(range(1000, 1000 + n)), shot=1, height=HO, width=WO, out_hw=(HO, WO))
        sup, msk, qry = (torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img"))
        queries = qry[:, 0].contiguous()
        bank = net.enroll(sup[:K], msk[:K])
        sides = {"segment": lambda: net.segment(bank, queries),
                 "segment_labels": lambda: net.segment_labels(bank, queries),
                 "segment_labels_graphed": lambda: net.segment_labels(bank, queries, graphed=True)}
        ms, reps = alternate(sides, args.rounds, args.block_s)
        extra = {"queries_per_step": n, "classes": K}
        report("labels_vs_segment", ms, reps, "segment", "segment_labels", extra)
        report("labels_vs_segment", ms, reps, "segment", "segment_labels_graphed", extra)


if __name__ == "__main__":
    main()
