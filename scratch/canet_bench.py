"""CANet inference throughput at 401 x 401 (side benchmark; bench.py measures the stage-1 headline).

usage: python scratch/canet_bench.py [--shots 1,5] [--per-step 25,1] [--episodes 200] [--rounds 3]

Per (shot, episodes per step) one JSON line: episodes/s of ``entry.canet.Evaluator.eval_round`` (captured slot-form steps,
fused tail, history table; Wgen weights) over a synthetic round with repeating keys whose episodes are generated once and
kept on the host, after one warm-up round; the number of steps the group-closing rule made of the round; FLOPs per episode
from the layer shapes below.  Then, twice, the captured 25-episode lowres step timed alone."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def conv_out(i, k, s, p, d=1):
    return (i + 2 * p - d * (k - 1) - 1) // s + 1


def flops_per_episode(shot, H=401):
    """2 * MACs of every conv of one episode's eval forward (the reference's layer shapes, canet.py:50-121)."""
    imgs = shot + 1
    conv = lambda n, h, cin, cout, k: 2.0 * n * h * h * cin * cout * k * k
    h = conv_out(H, 7, 2, 3)
    f = conv(imgs, h, 3, 64, 7)
    h = -(-(h - 1) // 2) + 1                                # ceil-mode 3x3/2 max pool, padding 1
    cin = 64
    for planes, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 1)):
        for b in range(blocks):
            ho = conv_out(h, 1, stride if b == 0 else 1, 0)
            f += conv(imgs, ho, cin, planes, 1) + conv(imgs, ho, planes, planes, 3) + conv(imgs, ho, planes, planes * 4, 1)
            if b == 0:
                f += conv(imgs, ho, cin, planes * 4, 1)
            h, cin = ho, planes * 4
    head = {"layer5": conv(imgs, h, 1536, 256, 3), "layer55": conv(1, h, 256, 256, 3),
            "residual": 6 * conv(1, h, 256, 256, 3), "aspp": conv(1, h, 256, 256, 1) + 3 * conv(1, h, 256, 256, 3) + conv(1, h, 1024, 256, 1)}
    return f + sum(head.values()), head, h


class _Cached:
    """A round of SyntheticHistoryEpisodes generated once (the host-side synthesis is not what is measured)."""

    def __init__(self, data):
        data.sample_tasks()
        self.height, self.width = data.height, data.width
        self.keys = [data.history_key(i) for i in range(len(data))]
        self.tasks = [data.task(i) for i in range(len(data))]

    def __len__(self):
        return len(self.tasks)

    def history_key(self, i):
        return self.keys[i]

    def task(self, i):
        return self.tasks[i]


def _model(shot, dev):
    from pemp_amd import synth
    from pemp_amd.networks import canet as m
    net = m.CaNet(None)
    net.load_state_dict(synth.wgen_state_dict_for(net, m.WGEN_SEED))
    return net.to(dev).eval()


def step_alone(net, dev, shot, per, steps, warmup):
    """ms per captured lowres step of ``per`` episodes."""
    from pemp_amd import synth
    b = synth.make_batch(list(range(1000, 1000 + per)), shot=shot, height=401, width=401, out_hw=(401, 401))
    inputs = [torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img")]
    with torch.no_grad():
        for _ in range(warmup):
            out = net.lowres_graphed(*inputs)[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = net.lowres_graphed(*inputs)[0]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    print(json.dumps({"captured_step_alone": True, "shot": shot, "episodes_per_step": per,
                      "ms_per_step": round(1e3 * dt / steps, 3), "episodes_per_s": round(per * steps / dt, 2),
                      "logit_sum": float(out.double().sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", default="1,5")
    ap.add_argument("--per-step", default="25,1")
    ap.add_argument("--episodes", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from pemp_amd.entry import canet as entry
    dev = torch.device("cuda:0")
    for shot in [int(s) for s in args.shots.split(",")]:
        net = _model(shot, dev)
        fl, head, h = flops_per_episode(shot)
        data = _Cached(entry.SyntheticHistoryEpisodes(args.episodes, 5678, shot, split=0, pool=max(args.episodes // 16, 1)))
        for per in [int(s) for s in args.per_step.split(",")]:
            ev = entry.Evaluator(net, device=dev)
            nsteps = len(entry.close_groups(data.keys, per))
            ev.eval_round(data, batch=per)                                   # warm-up: graphs for every group size
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.rounds):
                ev.eval_round(data, batch=per)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            eps = len(data) * args.rounds / dt
            print(json.dumps({"shot": shot, "episodes_per_step": per, "episodes_per_s": round(eps, 2), "round_episodes": len(data),
                              "distinct_keys": len(set(data.keys)), "steps_per_round": nsteps,
                              "gflop_per_episode": round(fl / 1e9, 2), "tflops": round(fl * eps / 1e12, 2), "feature_hw": h,
                              "head_gflop": {k: round(v / 1e9, 2) for k, v in head.items()}}), flush=True)
    net = _model(1, dev)
    for rep in range(2):
        step_alone(net, dev, 1, 25, 20, 5)


if __name__ == "__main__":
    main()
