"""PFENet head-training throughput at 4 x 401 x 401, 1-shot or 5-shot (side benchmark, bench.py measures the stage-1 headline).

usage: python scratch/pfenet_train_bench.py [--bs 4] [--shot 1] [--size 401] [--steps 20] [--warmup 5] [--rounds 5]
       [--trunk-precision f32_chain|split3|both] [--only-step]

``--trunk-precision both``: the two trunk precisions alternated in one process (scratch/trunk_precision_ab.py), nothing else;
``--only-step``: the ``train_step`` lines only (for a profiler run).

JSON lines:
  * ``train_step``: ms per ``PFENetTrainer.train_step`` and training episodes/s (host clock around steps that end in a
    synchronise, Wgen weights, Dropout2d on), twice -- the spread of the same command on the same code;
  * ``phases``: the step split by device events into the S + 1 trunk passes (with the prior), head forward, losses + their
    gradients, head backward, optimizer, and the trunk's share of the step;
  * ``kernels``: each new kernel of csrc/pfenet_bwd.hip alone on the step's shapes (events over ``--steps`` calls), as many calls
    as the step makes, and its share of the step."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import trunk_precision_ab  # noqa: E402


def timed(fn, reps, warm=3):
    """ms per call by device events."""
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=4)
    ap.add_argument("--shot", type=int, default=1)
    ap.add_argument("--size", type=int, default=401)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only-step", action="store_true")
    trunk_precision_ab.add_argument(ap)
    args = ap.parse_args()
    from pemp_amd import synth, train_ops as T
    from pemp_amd.networks import pfenet as m
    from pemp_amd.pfenet_engine import PYRAMID_BINS, REDUCE
    from pemp_amd.train_pfenet import PFENetTrainer
    dev = torch.device("cuda:0")
    H, B, S = args.size, args.bs, args.shot
    def trainer(precision):
        net = m.ModelClass(S, None)
        net.load_state_dict(synth.wgen_state_dict_for(net, m.WGEN_SEED))
        return PFENetTrainer(net, lr=1e-4, device=dev, trunk_precision=precision)

    both = args.trunk_precision == "both"
    tr = trainer("f32_chain" if both else args.trunk_precision)
    eng = tr.eng
    b = synth.make_batch(list(range(2000, 2000 + B)), shot=S, height=H, width=H, out_hw=(H, H))
    sup, msk, qry = (torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img"))
    gt = torch.from_numpy(b["qry_mask"]).reshape(-1, H, H).to(dev)

    def step():
        return tr.train_step(sup, msk, qry, qry_msk=gt)

    if both:
        tr3 = trainer("split3")
        trunk_precision_ab.alternate(f"pfenet_{S}shot", {"f32_chain": lambda: step()[0],
                                                         "split3": lambda: tr3.train_step(sup, msk, qry, qry_msk=gt)[0]},
                                     args.steps, args.warmup, args.rounds, B)
        return
    for _ in range(args.warmup):                                   # picks every conv / wgrad variant, fills the workspaces
        loss, aux = step()
    for rep in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss, aux = step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"train_step": rep, "bs": B, "shot": S, "size": H, "ms_per_step": round(1e3 * dt / args.steps, 3),
                          "episodes_per_s": round(B * args.steps / dt, 2), "loss": round(float(loss), 5), "aux": round(float(aux), 5)}),
              flush=True)
    step_ms = 1e3 * dt / args.steps
    if args.only_step:
        return

    # -- phases by device events ------------------------------------------------------------------------------------------
    order = ("t0", "trunk", "fwd", "loss", "bwd", "opt")
    ev = {k: [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)] for k in order}
    for i in range(args.steps):
        ev["t0"][i].record()
        eng.flat.attach_grads()
        eng.flat.grad.zero_()
        feats = eng.trunk_forward(sup, msk, qry)
        ev["trunk"][i].record()
        pred, inner = eng.head_forward(*feats, S)
        ev["fwd"][i].record()
        marked = eng.backward

        def backward(dpred, dinner, i=i, marked=marked):
            ev["loss"][i].record()
            return marked(dpred, dinner)
        eng.backward = backward
        tr.losses_backward(pred, inner, gt)
        del eng.backward                                           # back to the class's method
        ev["bwd"][i].record()
        tr.optimizer_step()
        ev["opt"][i].record()
    torch.cuda.synchronize()
    ph = {f"{a}->{c}": sum(x.elapsed_time(y) for x, y in zip(ev[a], ev[c])) / args.steps for a, c in zip(order, order[1:])}
    total = sum(ph.values())
    print(json.dumps({"phases_ms": {"trunk_passes": round(ph["t0->trunk"], 3), "head_forward": round(ph["trunk->fwd"], 3),
                                    "losses_and_gradients": round(ph["fwd->loss"], 3), "head_backward": round(ph["loss->bwd"], 3),
                                    "optimizer": round(ph["bwd->opt"], 3)},
                      "trunk_share_of_step": round(ph["t0->trunk"] / total, 4)}), flush=True)

    # -- the new kernels alone, as many calls as one step makes -----------------------------------------------------------------
    h = w = (H - 1) // 8 + 1
    f = eng.flat
    gs = [torch.randn((B, bn, bn, REDUCE), device=dev) for bn in PYRAMID_BINS]
    svec, dvec = torch.rand((B, REDUCE), device=dev), torch.randn((B, REDUCE), device=dev)
    wms = [f.krsc(mod.weight)[:, REDUCE:2 * REDUCE] for mod in eng.merge]
    dwms = [f.krsc_grad(mod.weight)[:, REDUCE:2 * REDUCE] for mod in eng.merge]
    mfeat = torch.rand((B * S, h, w), device=dev)
    dds, ddq = torch.empty((B * S, h, w, REDUCE), device=dev), torch.empty((B, h, w, REDUCE), device=dev)
    dres1 = torch.randn((B, h, w, REDUCE * len(PYRAMID_BINS)), device=dev)
    drec = [torch.randn((B, bn, bn, 2 * REDUCE), device=dev) for bn in PYRAMID_BINS]

    def resizes():                                                 # four map -> bin adjoints, three bin -> map ones with ``add``
        for k, bn in enumerate(PYRAMID_BINS):
            T.resize_bilinear_ac_bwd(dres1[..., k * REDUCE:(k + 1) * REDUCE], size=bn)
            if k >= 1:
                prev = dres1[..., (k - 1) * REDUCE:k * REDUCE]
                T.resize_bilinear_ac_bwd(drec[k][..., REDUCE:], add=prev, out=prev)

    kern = {
        "a_weighted_gap_bwd": lambda: T.weighted_gap_bwd(dvec, mfeat, S, dds),
        "b_adaptive_avgpool_bwd_multi": lambda: T.adaptive_avgpool_bwd_multi(gs, ddq),
        "c_resize_bilinear_ac_bwd_x7": resizes,
        "d_pfenet_merge_support_bwd": lambda: T.pfenet_merge_support_bwd(gs, wms, svec, dwms, ws_cache=eng.ws),
    }
    ms = {k: round(timed(fn, args.steps), 4) for k, fn in kern.items()}
    print(json.dumps({"kernels_ms": ms, "share_of_step": {k: round(v / step_ms, 5) for k, v in ms.items()},
                      "sum_share": round(sum(ms.values()) / step_ms, 5)}), flush=True)


if __name__ == "__main__":
    main()
