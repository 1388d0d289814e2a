"""PFENet inference throughput at 401 x 401 (side benchmark; bench.py measures the stage-1 headline).

usage: python scratch/pfenet_bench.py [--shots 1,5] [--per-step 25,1] [--steps 10] [--warmup 3]

Prints one JSON line per (shot, episodes per step): episodes/s of the captured lowres step (trunk, prior, FEM, classifier;
Wgen weights), the FLOPs per episode computed from the layer shapes below, and the prior kernel's compute bound (its
GEMM FLOPs at the fp32 MFMA peak).  The prior kernel's measured time comes from a separate run of this script under
``rocprofv3 --kernel-trace --stats`` (prior_tile_kernel in the stats CSV)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

FP32_MFMA_PEAK = 157.3e12          # MI355X, v_mfma_f32_32x32x2_f32, spec


def conv_out(i, k, s, p, d=1):
    return (i + 2 * p - d * (k - 1) - 1) // s + 1


def flops_per_episode(shot, H=401):
    """2 * MACs of every conv / GEMM of one episode's eval forward (the reference's layer shapes, pfenet.py:157-274)."""
    imgs = shot + 1
    f = 0.0

    def conv(n, h, w, cin, cout, k):
        return 2.0 * n * h * w * cin * cout * k * k
    h = conv_out(H, 3, 2, 1)
    f += conv(imgs, h, h, 3, 64, 3) + conv(imgs, h, h, 64, 64, 3) + conv(imgs, h, h, 64, 128, 3)
    h = conv_out(h, 3, 2, 1)
    cin = 128
    for planes, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 1), (512, 3, 1)):
        for b in range(blocks):
            ho = conv_out(h, 3, stride if b == 0 else 1, 1)
            f += conv(imgs, h, h, cin, planes, 1) + conv(imgs, ho, ho, planes, planes, 3) + conv(imgs, ho, ho, planes, planes * 4, 1)
            if b == 0:
                f += conv(imgs, ho, ho, cin, planes * 4, 1)
            h, cin = ho, planes * 4
    hw = h * h
    prior = 2.0 * shot * hw * hw * 2048
    f += prior
    f += conv(imgs, h, h, 1536, 256, 1)                                   # down_query / down_supp
    for i, b in enumerate((60, 30, 15, 8)):
        f += conv(1, b, b, 513, 256, 1) + 2 * conv(1, b, b, 256, 256, 3)
        if i:
            f += conv(1, b, b, 512, 256, 1)
    f += conv(1, h, h, 1024, 256, 1) + 2 * conv(1, h, h, 256, 256, 3) + conv(1, h, h, 256, 256, 3) + conv(1, h, h, 256, 2, 1)
    return f, prior, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", default="1,5")
    ap.add_argument("--per-step", default="25,1")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from pemp_amd import synth
    from pemp_amd.networks import pfenet as m
    dev = torch.device("cuda:0")
    for shot in [int(s) for s in args.shots.split(",")]:
        net = m.PFENet(shot, None)
        net.load_state_dict(synth.wgen_state_dict_for(net, m.WGEN_SEED))
        net = net.to(dev).eval()
        fl, prior_fl, h = flops_per_episode(shot)
        for per in [int(s) for s in args.per_step.split(",")]:
            b = synth.make_batch(list(range(1000, 1000 + per)), shot=shot, height=401, width=401, out_hw=(401, 401))
            inputs = [torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img")]
            with torch.no_grad():
                for _ in range(args.warmup):
                    net.lowres_graphed(*inputs)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    net.lowres_graphed(*inputs)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            eps = per * args.steps / dt
            print(json.dumps({"shot": shot, "episodes_per_step": per, "episodes_per_s": round(eps, 2),
                              "ms_per_step": round(1e3 * dt / args.steps, 3), "gflop_per_episode": round(fl / 1e9, 2),
                              "tflops": round(fl * eps / 1e12, 2), "feature_hw": h,
                              "prior_gflop_per_shot": round(prior_fl / shot / 1e9, 2),
                              "prior_bound_us_per_shot_fp32_mfma": round(prior_fl / shot / FP32_MFMA_PEAK * 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
