"""CANet head-training throughput at 4 x 401 x 401, 1-shot (the reference's ``bs = 4``; side benchmark, bench.py measures the
stage-1 headline).

usage: python scratch/canet_train_bench.py [--bs 4] [--shot 1] [--size 401] [--steps 20] [--warmup 5] [--rounds 5]
       [--trunk-precision f32_chain|split3|both] [--only-step]

``--trunk-precision both``: the two trunk precisions alternated in one process (scratch/trunk_precision_ab.py), nothing else;
``--only-step``: the ``train_step`` lines only (for a profiler run).

JSON lines:
  * ``train_step``: ms per ``CANetTrainer.train_step`` and training episodes/s (host clock around steps that end in a
    synchronise, Wgen weights, Dropout2d 0.5, a soft history), twice -- the spread of the same command on the same code;
  * ``phases``: the step split by device events into trunk forward, head forward, loss + its gradient, head backward, optimizer;
  * ``kernels``: each new kernel of csrc/canet_bwd.hip alone on the step's shapes (events over ``--steps`` calls) and its share
    of the step;
  * ``layer55_ab``: layer55's backward as shipped (query-half weight / input gradient + ``canet_zterm_bwd``) against the
    materialised form (cat(q, z broadcast) with 512 channels through the existing wgrad / dgrad kernels, dz as a pixel sum),
    alternated ``--rounds`` times in one process; every round's times are printed (the run-to-run spread)."""
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
    from pemp_amd import ops, synth, train_ops as T
    from pemp_amd.networks import canet as m
    from pemp_amd.ops import ConvParams
    from pemp_amd.train_canet import MID, CANetTrainer
    from pemp_amd.train_engine import _SliceWgrad
    dev = torch.device("cuda:0")
    def trainer(precision):
        net = m.CaNet(None)
        net.load_state_dict(synth.wgen_state_dict_for(net, m.WGEN_SEED))
        return CANetTrainer(net, lr=1e-4, device=dev, trunk_precision=precision), net

    both = args.trunk_precision == "both"
    tr, net = trainer("f32_chain" if both else args.trunk_precision)
    eng, H, B, S = tr.eng, args.size, args.bs, args.shot
    b = synth.make_batch(list(range(2000, 2000 + B)), shot=S, height=H, width=H, out_hw=(H, H))
    sup, msk, qry = (torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img"))
    gt = torch.from_numpy(b["qry_mask"]).reshape(-1, H, H).to(dev)
    h, w = net.feature_hw(H, H)
    hist = torch.softmax(torch.randn((B, 2, h, w), device=dev) * 2, dim=1)[:, None]

    def step():
        return tr.train_step(sup, msk, qry, qry_msk=gt, history_mask=hist)

    if both:
        tr3, _ = trainer("split3")
        trunk_precision_ab.alternate("canet", {"f32_chain": lambda: step()[0],
                                               "split3": lambda: tr3.train_step(sup, msk, qry, qry_msk=gt, history_mask=hist)[0]},
                                     args.steps, args.warmup, args.rounds, B)
        return
    for _ in range(args.warmup):                                   # picks every conv / wgrad variant, fills the workspaces
        loss, _ = step()
    for rep in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss, _ = step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"train_step": rep, "bs": B, "shot": S, "size": H, "feature_hw": h, "ms_per_step": round(1e3 * dt / args.steps, 3),
                          "episodes_per_s": round(B * args.steps / dt, 2), "loss": round(float(loss), 5)}), flush=True)
    step_ms = 1e3 * dt / args.steps
    if args.only_step:
        return

    # -- phases by device events ------------------------------------------------------------------------------------------
    ev = {k: [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)] for k in ("t0", "trunk", "fwd", "loss", "bwd", "opt")}
    trunk_fwd = eng._trunk_forward
    it = [0]

    def trunk_marked(images):
        out = trunk_fwd(images)
        ev["trunk"][it[0]].record()
        return out
    eng._trunk_forward = trunk_marked
    for i in range(args.steps):
        it[0] = i
        ev["t0"][i].record()
        eng.flat.attach_grads()
        eng.flat.grad.zero_()
        pred = eng.forward(sup, msk, qry, history=hist[:, 0].contiguous())
        ev["fwd"][i].record()
        _, stats, _ = ops.eval_tail(pred, gt, ws_cache=eng.ws)
        dpred = T.upsample_ce_bwd(pred, gt, stats)
        ev["loss"][i].record()
        eng.backward(dpred)
        ev["bwd"][i].record()
        tr.optimizer_step()
        ev["opt"][i].record()
    torch.cuda.synchronize()
    eng._trunk_forward = trunk_fwd
    order = ("t0", "trunk", "fwd", "loss", "bwd", "opt")
    ph = {f"{a}->{c}": round(sum(x.elapsed_time(y) for x, y in zip(ev[a], ev[c])) / args.steps, 3) for a, c in zip(order, order[1:])}
    print(json.dumps({"phases_ms": {"trunk_forward": ph["t0->trunk"], "head_forward": ph["trunk->fwd"], "loss_and_gradient": ph["fwd->loss"],
                                    "head_backward": ph["loss->bwd"], "optimizer": ph["bwd->opt"]}}), flush=True)

    # -- the new kernels alone ------------------------------------------------------------------------------------------------
    f = eng.flat
    c55 = eng.l55
    w55 = f.krsc(c55.conv.weight).view(MID, 9, 2 * MID)
    dw55 = f.krsc_grad(c55.conv.weight).view(MID, 9, 2 * MID)
    g55, z = torch.randn((B, h, w, MID), device=dev), torch.rand((B, MID), device=dev)
    fq = torch.randn((B, h, w, MID), device=dev)
    df = torch.empty((B * S, h, w, MID), device=dev)
    smask = msk.reshape(B * S, 2, H, H).float().contiguous()
    pred = torch.randn((B, 2, h, w), device=dev)
    _, stats, _ = ops.eval_tail(pred, gt, ws_cache=eng.ws)
    dpred = T.upsample_ce_bwd(pred, gt, stats)
    x6, dx6 = torch.randn((B, h, w, MID), device=dev), torch.empty((B, h, w, MID), device=dev)
    l7 = eng.l7.conv
    w7 = f.krsc(l7.weight)
    kern = {
        "a_zterm_bwd": lambda: T.canet_zterm_bwd(g55, w55[:, :, MID:], z, dw55[:, :, MID:], c55.dil, ws_cache=eng.ws),
        "b_support_vector_bwd": lambda: T.canet_support_vector_bwd(z, smask, S, df),
        "c_cls_bwd": lambda: T.canet_cls_bwd(dpred, x6, w7, dx6, f.krsc_grad(l7.weight), l7.bias.grad, ws_cache=eng.ws),
        "d_upsample_ce_bwd": lambda: T.upsample_ce_bwd(pred, gt, stats),
    }
    ms = {k: round(timed(fn, args.steps), 4) for k, fn in kern.items()}
    print(json.dumps({"kernels_ms": ms, "share_of_step": {k: round(v / step_ms, 5) for k, v in ms.items()},
                      "sum_share": round(sum(ms.values()) / step_ms, 5)}), flush=True)

    # -- layer55's backward: split form against the materialised 512-channel form ---------------------------------------------
    f.refresh_dgrad_mirror()
    torch.cuda.synchronize()
    wd = f.dgrad_krsc(c55.conv.weight)                                         # [512, 9 * 256]
    dq = torch.empty((B, h, w, MID), device=dev)
    pdq = ConvParams(wd[:MID], None, None, MID, MID, 3, 3, 1, c55.dil * 2 - c55.pad, c55.dil, wd.shape[1], False, False)
    wg_q = _SliceWgrad(MID, MID, [(dw55[:, :, :MID], slice(None))], 3, c55.pad, c55.dil)

    def split_form():
        wg_q._wgrad_now(fq, g55, eng.ws)
        ops.conv2d(g55, pdq, out=dq, splitk=True)
        T.canet_zterm_bwd(g55, w55[:, :, MID:], z, dw55[:, :, MID:], c55.dil, ws_cache=eng.ws)

    dcat = torch.empty((B, h, w, 2 * MID), device=dev)
    pdc = ConvParams(wd, None, None, MID, 2 * MID, 3, 3, 1, c55.dil * 2 - c55.pad, c55.dil, wd.shape[1], False, False)

    def materialised():
        cat = torch.cat((fq, z[:, None, None, :].expand(-1, h, w, -1)), dim=3)
        c55._wgrad_now(cat, g55, eng.ws)
        ops.conv2d(g55, pdc, out=dcat, splitk=True)
        return ops.global_avgpool(dcat[..., MID:]) * float(h * w)              # dz

    rounds = []
    for _ in range(args.rounds):
        rounds.append({"split_ms": round(timed(split_form, args.steps), 4), "materialised_ms": round(timed(materialised, args.steps), 4)})
    print(json.dumps({"layer55_ab": rounds, "split_min_max": [min(r["split_ms"] for r in rounds), max(r["split_ms"] for r in rounds)],
                      "materialised_min_max": [min(r["materialised_ms"] for r in rounds), max(r["materialised_ms"] for r in rounds)]}),
          flush=True)


if __name__ == "__main__":
    main()
