"""RPMMs support banks against whole episodes: ResNet-50, 401 x 401, 25 queries per step (side benchmark; bench.py measures the
headline and is not involved).

usage: python scratch/rpmms_bank_bench.py [--queries 25] [--rounds 5] [--block-s 0.8]
       python scratch/rpmms_bank_bench.py --kernels [--iters 20]      (to be run under rocprofv3 --kernel-trace --stats)

Default mode, one JSON line per figure (the timing protocol is scratch/bank_bench.py's: both sides warmed up, then rounds in which the
two sides alternate in one process, the median ms per step and its spread per side):
  bank_store        bytes per class of the enrolled bank (mu + taps)
  episode_vs_bank   the captured episode step (``lowres_graphed``: one support + one query per episode through the trunk, the EM) against
                    the captured bank step (``segment_graphed`` with an index: the queries alone; the K = 5 classes enrolled before)
  all_vs_indexed    one all-classes step (every query against the 5 classes: one trunk pass, one base conv, an N * K wide layer56
                    and three N * K wide tails) against five indexed steps (one per class: five trunk passes)

``--kernels``: layer56's input alone on [25, 51, 51, 256] layer5-like maps -- ``iters`` indexed bank launches (bank_l56_kernel),
``iters`` all-classes launches at K = 5 and ``iters`` launches of the episode kernels on the same operands as the indexed ones
(tap_gemv_kernel + proto_sum_kernel, prob_map_kernel) -- for a kernel trace."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bank_bench import alternate, report  # noqa: E402  (scratch/bank_bench.py)

K = 5


def kernels(iters):
    from pemp_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    n, h, w, c, ld = 25, 51, 51, 256, 288
    qry = (torch.rand(n, h, w, c, generator=g) - 0.3).clamp_min(0.0).to(dev)
    base = torch.randn(n, h, w, c, generator=g).to(dev)
    mu = torch.randn(K, 2, 10, c, generator=g)
    mu = (mu / mu.norm(dim=3, keepdim=True)).to(dev)
    wz = (torch.randn(9, c, c, generator=g) * (1.0 / (c * 9) ** 0.5)).to(dev)
    bias = (torch.randn(c, generator=g) * 0.1).to(dev)
    index = [i % K for i in range(n)]
    idx_dev = torch.tensor(index, dtype=torch.int32, device=dev)
    mu_e = mu[idx_dev.long()].contiguous()                          # what an episode step has: one mu per query
    taps = ops.rpmms_proto_taps(wz, mu)
    out_b, out_e = torch.zeros(3, n, h, w, ld, device=dev), torch.zeros(3, n, h, w, ld, device=dev)
    out_a = torch.zeros(3, n * K, h, w, ld, device=dev)
    scratch = torch.empty(n, 10, 9, c, device=dev)
    for _ in range(iters):
        ops._rpmms_bank_l56(qry, base, bias, mu, taps, out_b, idx_dev)
    for _ in range(iters):
        ops._rpmms_bank_l56(qry, base, bias, mu, taps, out_a, None)
    for _ in range(iters):
        ops.rpmms_proto_sum(wz, mu_e, base, bias, out_e[..., :c], taps=scratch)
        ops.rpmms_prob_map(qry, mu_e, out_e)
    torch.cuda.synchronize()
    pairs = out_a.view(3, n, K, h, w, ld)[:, torch.arange(n), idx_dev.long()]
    print(json.dumps({"what": "kernels", "iters": iters, "queries": n, "classes": K, "hw": h * w, "c": c,
                      "equal": bool(torch.equal(out_b, out_e)), "all_classes_equal": bool(torch.equal(pairs, out_e))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block-s", type=float, default=0.8)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if args.kernels:
        return kernels(args.iters)
    from pemp_amd import synth
    from pemp_amd.networks import rpmms as m
    dev = torch.device("cuda:0")
    n = args.queries
    net = m.RPMMs(None)
    net.load_state_dict(synth.wgen_state_dict_for(net, m.WGEN_SEED))
    net = net.to(dev).eval()
    net.resample_pmm_init(torch.Generator().manual_seed(7))
    net.set_pmm_init({k: net.pmm_mu0[j0:j0 + k].t() for j0, k in ((0, 1), (1, 3), (4, 6))})      # one init for every step
    b = synth.make_batch(list(range(1000, 1000 + n)), shot=1, height=401, width=401, out_hw=(401, 401))
    sup, msk, qry = (torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img"))
    queries = qry[:, 0].contiguous()
    index = [i % K for i in range(n)]
    with torch.no_grad():
        bank = net.enroll(sup[:K], msk[:K])
        print(json.dumps({"what": "bank_store", "classes": K, "bytes_per_class": bank.nbytes()}), flush=True)
        sides = {"episode": lambda: net.lowres_graphed(sup, msk, qry), "bank": lambda: net.segment_graphed(bank, queries, index=index)}
        ms, reps = alternate(sides, args.rounds, args.block_s)
        report("episode_vs_bank", ms, reps, "episode", "bank",
               {"queries_per_step": n, "classes": K, "trunk_images_per_step": {"episode": 2 * n, "bank": n}})
        per_class = [[k] * n for k in range(K)]

        def five():
            for idx in per_class:
                net.segment_graphed(bank, queries, index=idx)
        sides = {"five_indexed": five, "all_classes": lambda: net.segment_graphed(bank, queries)}
        ms, reps = alternate(sides, args.rounds, args.block_s)
    report("all_vs_indexed", ms, reps, "five_indexed", "all_classes", {"queries_per_step": n, "classes": K})


if __name__ == "__main__":
    main()
