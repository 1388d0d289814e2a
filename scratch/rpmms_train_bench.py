"""RPMMs head-training throughput at 4 x 401 x 401, 1-shot, beside CANet's from the same process (side benchmark, bench.py
measures the stage-1 headline).

usage: python scratch/rpmms_train_bench.py [--bs 4] [--size 401] [--steps 20] [--warmup 5] [--only-rpmms]
       [--rounds 5] [--trunk-precision f32_chain|split3|both]

``--trunk-precision`` is the RPMMs trainer's (the CANet comparison stays on its default); ``both``: the two trunk precisions of the
RPMMs trainer alternated in one process (scratch/trunk_precision_ab.py), nothing else.

JSON lines:
  * ``train_step``: ms per ``RPMMsTrainer.train_step`` / ``CANetTrainer.train_step`` and training episodes/s (host clock around
    steps that end in a synchronise, Wgen weights, Dropout2d 0.5, Philox masks, a fresh initial mu per RPMMs step), the two
    models alternated twice -- the spread of the same command on the same code -- and the ratio CANet / RPMMs per round;
  * ``kernels``: each new op of csrc/rpmms_bwd.hip alone on the step's shapes (device events over ``--steps`` calls) and its share
    of the RPMMs step;
  * ``accumulate``: the elementwise work of the three accumulate points of the backward (clone, two adds and the copy back of
    the tail's span of the flat gradient buffer) alone, by device events.  The joins that go with them also end the overlap of
    the side stream's weight gradients with the next pass's chain; that part shows only in a kernel trace.

``--only-rpmms`` runs the RPMMs steps alone (for a ``rocprofv3 --kernel-trace --stats`` run of its own)."""
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
    ap.add_argument("--size", type=int, default=401)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only-rpmms", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    trunk_precision_ab.add_argument(ap)
    args = ap.parse_args()
    from pemp_amd import synth, train_ops as T
    from pemp_amd.networks import canet, rpmms
    from pemp_amd.train_canet import MID, CANetTrainer
    from pemp_amd.train_rpmms import RPMMsTrainer
    dev = torch.device("cuda:0")
    H, B = args.size, args.bs
    b = synth.make_batch(list(range(2000, 2000 + B)), shot=1, height=H, width=H, out_hw=(H, H))
    sup, msk, qry = (torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img"))
    gt = torch.from_numpy(b["qry_mask"]).reshape(-1, H, H).to(dev)

    def trainer(precision):
        net = rpmms.RPMMs(None)
        net.load_state_dict(synth.wgen_state_dict_for(net, rpmms.WGEN_SEED))
        return RPMMsTrainer(net.freeze_trunk(), lr=1e-4, device=dev, trunk_precision=precision), net

    both = args.trunk_precision == "both"
    rtr, rnet = trainer("f32_chain" if both else args.trunk_precision)
    h, w = rnet.feature_hw(H, H)
    if both:
        rtr3, _ = trainer("split3")
        trunk_precision_ab.alternate("rpmms", {"f32_chain": lambda: rtr.train_step(sup, msk, qry, qry_msk=gt)[0],
                                               "split3": lambda: rtr3.train_step(sup, msk, qry, qry_msk=gt)[0]},
                                     args.steps, args.warmup, args.rounds, B)
        return
    steps = {"rpmms": lambda: rtr.train_step(sup, msk, qry, qry_msk=gt)[0]}
    if not args.only_rpmms:
        cnet = canet.CaNet(None)
        cnet.load_state_dict(synth.wgen_state_dict_for(cnet, canet.WGEN_SEED))
        ctr = CANetTrainer(cnet, lr=1e-4, device=dev)
        hist = torch.softmax(torch.randn((B, 2, h, w), device=dev) * 2, dim=1)[:, None]
        steps["canet"] = lambda: ctr.train_step(sup, msk, qry, qry_msk=gt, history_mask=hist)[0]
    for fn in steps.values():
        for _ in range(args.warmup):                               # picks every conv / wgrad variant, fills the workspaces
            fn()
    ms = {}
    for rep in range(2):
        for name, fn in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ms[name] = 1e3 * dt / args.steps
            print(json.dumps({"train_step": rep, "model": name, "bs": B, "size": H, "feature_hw": h, "ms_per_step": round(ms[name], 3),
                              "episodes_per_s": round(B * args.steps / dt, 2), "loss": round(float(loss), 5)}), flush=True)
        if "canet" in ms:
            print(json.dumps({"round": rep, "canet_over_rpmms_episodes_per_s": round(ms["rpmms"] / ms["canet"], 3)}), flush=True)
    if args.only_rpmms:
        return
    step_ms = ms["rpmms"]

    # -- the new ops alone ----------------------------------------------------------------------------------------------------
    eng = rtr.eng
    f, c55 = eng.flat, eng.l55
    w55 = f.krsc(c55.conv.weight).view(MID, 9, 2 * MID)
    dw55 = f.krsc_grad(c55.conv.weight).view(MID, 9, 2 * MID)
    wz = w55[:, :, MID:].permute(1, 0, 2).contiguous()
    mu = torch.randn((B, 2, 10, MID), device=dev)
    mu = (mu / mu.norm(dim=3, keepdim=True)).contiguous()
    base, bias = torch.randn((B, h, w, MID), device=dev), c55.conv.bias.data
    mult = (torch.rand((B, 10, MID), device=dev) < 0.5).float() * 2.0
    x56 = torch.zeros((3, B, h, w, 320), device=dev)
    _, taps = T.rpmms_proto_sum_train(wz, mu, base, bias, mult, x56[..., :MID], dil=c55.dil)
    dout, dbias = torch.randn((3, B, h, w, MID), device=dev), torch.empty(MID, device=dev)
    dh, dpred = torch.randn((B, h, w, 64), device=dev), torch.zeros((B, 2, h, w), device=dev)
    prob = torch.softmax(torch.randn((B, 2, h, w), device=dev), dim=1).contiguous()
    kern = {
        "a_proto_sum_train": lambda: T.rpmms_proto_sum_train(wz, mu, base, bias, mult, x56[..., :MID], dil=c55.dil, taps=taps),
        "b_proto_sum_bwd_dbase_G": lambda: T.rpmms_proto_sum_bwd(dout, base, bias, taps, mult, dil=c55.dil, ws_cache=eng.ws),
        "c_proto_sum_bwd_with_dWz_dbias": lambda: T.rpmms_proto_sum_bwd(dout, base, bias, taps, mult, dil=c55.dil, mu=mu, dw_z=dw55[:, :, MID:],
                                                                        dbias=dbias, ws_cache=eng.ws),
        "d_history_bwd": lambda: T.rpmms_history_bwd(dh[..., :2], prob, dpred),
    }
    kms = {k: round(timed(fn, args.steps), 4) for k, fn in kern.items()}
    per_step = kms["a_proto_sum_train"] + kms["c_proto_sum_bwd_with_dWz_dbias"] + 2 * kms["d_history_bwd"]
    print(json.dumps({"kernels_ms": kms, "dWz_and_dbias_ms": round(kms["c_proto_sum_bwd_with_dWz_dbias"] - kms["b_proto_sum_bwd_dbase_G"], 4),
                      "new_ops_per_step_ms": round(per_step, 4), "share_of_step": round(per_step / step_ms, 5)}), flush=True)

    # -- the accumulate points' elementwise work -------------------------------------------------------------------------------
    tail = f.grad[eng.tail_lo:]

    def accumulate():
        acc = tail.clone()
        acc.add_(tail)
        acc.add_(tail)
        tail.copy_(acc)
    ams = timed(accumulate, args.steps)
    print(json.dumps({"accumulate": {"tail_floats": tail.numel(), "ms_per_step": round(ams, 4), "share_of_step": round(ams / step_ms, 5)}}), flush=True)


if __name__ == "__main__":
    main()
