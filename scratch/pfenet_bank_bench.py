"""PFENet support banks against whole episodes: ResNet-50, 401 x 401, 25 queries per step (side benchmark; bench.py measures the
headline and is not involved).

usage: python scratch/pfenet_bank_bench.py [--shots 1,5] [--queries 25] [--rounds 5] [--block-s 0.8]
       python scratch/pfenet_bank_bench.py --kernels [--iters 20]      (to be run under rocprofv3 --kernel-trace --stats)

Default mode, one JSON line per figure (the timing protocol is scratch/bank_bench.py's: both sides warmed up, then rounds in which the
two sides alternate in one process, the median ms per step and its spread per side):
  bank_store        bytes per class of the enrolled bank against the dense S * HW * C * 4 of its layer-4 maps, with the share of the
                    map the synthetic masks' foreground covers (stored rows / HW)
  trunk_share       eager, device-timed: the part of the episode step up to and including layer 4 against the whole step
  episode_vs_bank   the captured episode step (``lowres_graphed``: S supports + 1 query per episode through the trunk) against the
                    captured bank step (``segment_graphed`` with an index: the queries alone; the K = 5 classes enrolled before)
  all_vs_indexed    one all-classes step (every query against the 5 classes: one trunk pass, an N * K wide FEM tail) against five
                    indexed steps (one per class: five trunk passes)

``--kernels``: the prior alone on [25, 51, 51, 2048] layer-4-like maps -- ``iters`` indexed bank launches (prior_bank_kernel) and
``iters`` launches of the episode kernels on the same operands (prior_tile_kernel + prior_tilemax_kernel) -- for a kernel trace."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bank_bench import alternate, report  # noqa: E402  (scratch/bank_bench.py)

K = 5


def kernels(iters, share=0.15):
    from pemp_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    n, h, w, c = 25, 51, 51, 2048
    q = (torch.rand(n, h, w, c, generator=g) - 0.3).clamp_min(0.0).to(dev)
    s = (torch.rand(n, h, w, c, generator=g) - 0.3).clamp_min(0.0).to(dev)
    m = ((torch.rand(n, h, w, generator=g) < share).float() * torch.rand(n, h, w, generator=g).clamp_min(0.5)).to(dev)
    rows, norms, count = ops.prior_bank_pack(s, m, n, 1, cap=ops._round64(int(share * 2 * h * w)))   # one class per query
    assert int(count.max()) <= rows.shape[2], "the store is too small for these masks"
    index = torch.arange(n, dtype=torch.int32, device=dev)
    ws = {}
    out_b, out_e = torch.empty(n, h, w, device=dev), torch.empty(n, h, w, device=dev)
    for _ in range(iters):
        ops._prior_bank(q, rows, norms, count, index, out=out_b, ws_cache=ws)
    for _ in range(iters):
        ops.prior_mask(q, s, m, 1, out=out_e, ws_cache=ws)
    torch.cuda.synchronize()
    print(json.dumps({"what": "kernels", "iters": iters, "queries": n, "hw": h * w, "c": c, "rows_stored_mean": float(count.float().mean()),
                      "equal": bool(torch.equal(out_b, out_e))}))


def device_ms(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", default="1,5")
    ap.add_argument("--queries", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block-s", type=float, default=0.8)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if args.kernels:
        return kernels(args.iters)
    from pemp_amd import synth
    from pemp_amd.networks import pfenet as m
    dev = torch.device("cuda:0")
    n = args.queries
    for shot in [int(s) for s in args.shots.split(",")]:
        net = m.PFENet(shot, None)
        net.load_state_dict(synth.wgen_state_dict_for(net, m.WGEN_SEED))
        net = net.to(dev).eval()
        b = synth.make_batch(list(range(1000, 1000 + n)), shot=shot, height=401, width=401, out_hw=(401, 401))
        sup, msk, qry = (torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img"))
        queries = qry[:, 0].contiguous()
        index = [i % K for i in range(n)]
        with torch.no_grad():
            bank = net.enroll(sup[:K], msk[:K])
            dense = shot * bank.HW * bank.C * 4
            print(json.dumps({"what": "bank_store", "shot": shot, "classes": K, "cap": bank.cap, "bytes_per_class": bank.nbytes(),
                              "dense_bytes_per_class": dense, "ratio": round(bank.nbytes() / dense, 4),
                              "rows_stored_over_hw_mean": round(float(bank.count_host.float().mean()) / bank.HW, 4),
                              "rows_stored_over_hw_max": round(int(bank.count_host.max()) / bank.HW, 4)}), flush=True)
            eng = net._engine_for(dev)["pfenet"]
            whole = device_ms(lambda: net.lowres(sup, msk, qry))
            trunk = device_ms(lambda: eng._layer4((sup.flatten(0, 1), qry.flatten(0, 1)), msk, n * shot))
            print(json.dumps({"what": "trunk_share", "shot": shot, "queries_per_step": n, "episode_step_ms": round(whole, 3),
                              "through_layer4_ms": round(trunk, 3), "share": round(trunk / whole, 4)}), flush=True)
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
        del net, bank, sides
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
