#!/usr/bin/env python3
"""Headline benchmark: episodes/sec of the PEMP hot path on N MI355X.

    python bench.py --gpus N --steps K --warmup W                      eval, BASELINE.json configs[1] (headline)
    python bench.py --mode train [--model stage2]                      training step, configs[2] (stage 2: + the prior pass)
    python bench.py --model stage2 --shot 5 --batch 8                  stage-1 prior + stage 2, 5-shot, configs[3]
    python bench.py --dataset COCO                                     COCO-20i-shaped episodes, configs[4]
    python bench.py --model baseline --batch 12                        Baseline VGG-16, configs[0]
    python bench.py ... --dump-outputs DIR                             + what the last timed step computed, DIR/<name>.npy
    python bench.py ... --full                                         + every figure beside the headline (list below)

A "step" is one pass of the hot path over ``--batch`` synthetic episodes already resident in HBM: for eval the device
work of Evaluator.test_step (encoder, meta-prototype module, cosine map, upsample + argmax + CE + IoU counts; reference
entry/pemp_stage1.py:48-53), for train the whole Trainer.train_step (entry/pemp_stage1.py:57-65).  Ranks are independent
in eval (episodes shard; no data-path collective) and data-parallel in training (gradient all-reduce over RCCL); scaling
is weak.  ``--gpus N`` without a launcher around it (no WORLD_SIZE in the environment) starts the N ranks itself.

Rank 0 prints ONE JSON line: the headline (metric, value, unit, ms_per_step, ...), its `config`, and
  comm            what the ranks exchanged inside the timed region and how evenly they ran: backend, world, RCCL version,
                  bytes all-reduced, the gradient buckets with their element ranges (train), exposed communication time,
                  every rank's own ms_per_step; eval: the round's metric table is all-reduced INSIDE the timed region and
                  checked against the sum of the rank shards (``miou`` for N > 1, ``round_miou`` for N = 1, from the
                  reduced table)
A plain run does nothing else: it sets up, warms up, times the K steps, writes --dump-outputs and prints the line.
``--full`` adds the objects below, each measured after the timed region in the same process (``--no-roofline``,
``--no-single``, ``--no-e2e``, ``--no-sides`` and ``--cpu-episodes 0`` leave single ones out of a full line):
  roofline        the dominant kernel class (the fp32-MFMA implicit-GEMM convs) against the 157.3 TFLOP/s dense fp32
                  matrix peak: algorithmic flops of every conv launch of a step / their durations, taken live with HIP
                  events on the stream each kernel is launched on (an instrumented pass over the C ABI, eager, same
                  workload); ``by_class`` splits the step over conv / weight-gradient / BatchNorm / head / optimizer
  single_episode  (eval, N = 1) the reference's own protocol, one episode per test_step (data_kits/datasets.py:23)
  end_to_end      (N = 1) episodes/s including input staging (uint8 host samples -> device preprocessing -> the step)
  cpu_baseline    the CPU oracle (oracle/ref_cpu.py, bit-equal to the reference here) timed on the host cores in child
                  processes: 1 thread and all cores of the box's share, bounded samples of the same workload; ``miou``
                  (stage 1, N = 1): the mIoU of the episodes it evaluated, on the device and on the CPU
  protocol_5x1000 (headline line) the reference's evaluation protocol: 5 rounds x 1000 episodes, one episode per test_step
  cedt            (headline line) the eval step and the train step with loss=cedt (CELossDT on the device), next to loss=ce
  train, stage2_5shot, coco, baseline_vgg16
                  (headline line) the other BASELINE.json configurations, each with a roofline fraction of its own
  bf16_variant    (with --bf16-side; SIDE FIGURE, never `value` / `roofline`) the eval step with bf16 operands in the
                  encoder: episodes/s, and the mIoU / arg-max pixels it moves on one round over the resident episodes
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md, "Peak FP32 (matrix)"
PEAK_HBM_GBS = 8000.0            # MI355X_MICROARCH.md, "HBM3E peak BW" (spec; 6.29 TB/s measured for a float4 copy)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--batch", type=int, default=int(os.environ.get("PEMP_BENCH_BATCH", "25")),
                    help="episodes per step (the reference evaluates 1 per step); 25 -> 50 x 2601 feature rows, "
                         "which fill the 256-row conv tiles and the 256 CUs almost exactly")
    ap.add_argument("--shot", type=int, default=1)
    ap.add_argument("--model", choices=("stage1", "stage2", "baseline", "panet"), default="stage1",
                    help="stage1 = headline; stage2 = stage-1 prior + stage-2 (use with --shot 5 for configs[3]); "
                         "baseline = Baseline VGG-16 (configs[0]); panet = PANet VGG-16 (the Baseline step + the alignment branch)")
    ap.add_argument("--mode", choices=("eval", "train"), default="eval",
                    help="eval (headline metric, BASELINE.json configs[1]) or train (configs[2])")
    ap.add_argument("--dataset", choices=("PASCAL", "COCO"), default="PASCAL",
                    help="COCO: BASELINE.json configs[4] -- COCO-20i label set and picture formats (ground truth up to 640x640)")
    ap.add_argument("--loss", choices=("ce", "cedt"), default="ce",
                    help="cedt: CELossDT (core/losses.py:17-43; what the reference's scripts train with) -- boundary + exact "
                         "distance transform + weighted CE on the device, inside the timed region")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure every other figure of the line: roofline, CPU baseline, "
                         "single-episode and staging-inclusive figures, the other configurations (see the module docstring)")
    ap.add_argument("--cpu-episodes", type=int, default=12, help="--full: bounded CPU-baseline sample (0 = skip)")
    ap.add_argument("--train-graph", action="store_true", help="--mode train: replay forward/backward from a hipGraph")
    ap.add_argument("--no-roofline", action="store_true", help="--full: skip the roofline pass")
    ap.add_argument("--no-e2e", action="store_true", help="--full: skip the staging-inclusive end_to_end figure")
    ap.add_argument("--no-single", action="store_true", help="--full: skip the one-episode-per-step figure")
    ap.add_argument("--no-sides", action="store_true", help="--full, headline line: skip the `protocol_5x1000` / `cedt` / `train` / "
                                                            "`stage2_5shot` / `coco` / `baseline_vgg16` objects")
    ap.add_argument("--bf16-side", action="store_true", help="--full, headline line: also measure the bf16-operand side figure")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="write what the last timed step computed (rank 0's share) as DIR/<name>.npy: eval -> qry_pred (arg-max "
                         "class per pixel) and stats (ce_sum, n_valid, tp/fp/fn bg, tp/fp/fn fg per episode); train -> loss "
                         "and weights (the flat parameter buffer after the step)")
    ap.add_argument("--cpu-leg", default="", help=argparse.SUPPRESS)        # internal: "<threads>" -> run one CPU-baseline leg
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


# ---------------------------------------------------------------------------------------------
# N > 1 without an external launcher: `python bench.py --gpus N` starts its own ranks
# ---------------------------------------------------------------------------------------------
def beat():
    """Heartbeat of a rank started by ``launch_ranks``: touches the rank's file (PEMP_BENCH_HEARTBEAT) at every phase
    boundary outside the timed region.  The launcher's silence watchdog reads the modification times."""
    path = os.environ.get("PEMP_BENCH_HEARTBEAT")
    if path:
        with open(path, "a"):
            os.utime(path, None)


def host_cores():
    try:
        return len(os.sched_getaffinity(0))
    except AttributeError:
        return os.cpu_count() or 1


def host_threads_per_rank(local_world):
    """Host threads one of ``local_world`` ranks on this host may use: cores / ranks, at most 16 -- what one rank's episode
    synthesis and enqueue loop can use (PEMP_BENCH_THREADS overrides)."""
    return max(1, int(os.environ.get("PEMP_BENCH_THREADS", min(16, host_cores() // max(1, local_world)))))


# ---------------------------------------------------------------------------------------------
# what the ranks exchanged, and how evenly they ran (the `comm` object of every line)
# ---------------------------------------------------------------------------------------------
def rccl_version():
    try:
        v = torch.cuda.nccl.version()
        return ".".join(str(x) for x in v) if isinstance(v, (tuple, list)) else str(v)
    except Exception:  # noqa: BLE001
        return None


def gather_rank_ms(local_dt, steps, world, dev):
    """Every rank's OWN elapsed time of the timed region (the headline uses the MAX), as ms per step, rank order."""
    if world == 1:
        return [local_dt / steps * 1e3]
    mine = torch.tensor([local_dt], dtype=torch.float64, device=dev)
    out = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(out, mine)
    return [float(t.item()) / steps * 1e3 for t in out]


def comm_object(world, rank_ms, **fields):
    backend = dist.get_backend() if world > 1 and dist.is_initialized() else None
    out = {"backend": backend, "world": world, "rccl_version": rccl_version() if backend == "nccl" else None,
           "host_threads_per_rank": torch.get_num_threads()}
    out.update(fields)
    out["rank_ms_per_step"] = {"min": round(min(rank_ms), 4), "max": round(max(rank_ms), 4), "all": [round(v, 4) for v in rank_ms]}
    return out


class RoundReduce:
    """The evaluation round's aggregation INSIDE the timed region (reference core/base_trainer.py:70-100: the metric table
    of the round's episodes, mIoU per round): statistics rows -> [C+1, 3] table by class on the device, ONE all-reduce(SUM)
    of table + loss sum + episode count (``DeviceRoundTable``), bracketed by events.  ``verify`` (after the timed region)
    gathers every rank's own shard and checks that the reduced table is exactly their sum."""

    def __init__(self, nclass, dev, dataset="PASCAL"):
        from pemp_amd.entry.pemp_stage1 import DeviceRoundTable
        self.table, self.dev, self.dataset, self.nclass = DeviceRoundTable(nclass, dev), dev, dataset, nclass
        self.local, self.nbytes, self.events = None, 0, None

    def reduce(self, stats, classes):
        self.table.reset()
        self.table.add(stats, classes)
        self.local = self.table.pack.clone()
        if self.dev.type == "cuda":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.nbytes = self.table.allreduce()
            e1.record()
            self.events = (e0, e1)
        else:
            t0 = time.perf_counter()
            self.nbytes = self.table.allreduce()
            self.events = (time.perf_counter() - t0) * 1e3

    def allreduce_ms(self):
        if isinstance(self.events, tuple):
            self.events[1].synchronize()
            return self.events[0].elapsed_time(self.events[1])
        return self.events

    def verify(self, world):
        """-> (reduced table == sum of the rank shards [exact: integer-valued doubles], miou object) -- a collective: every
        rank calls it."""
        from pemp_amd import synth
        from pemp_amd.core.metrics import FewShotMetric
        shards = [self.local]
        if world > 1:
            shards = [torch.zeros_like(self.local) for _ in range(world)]
            dist.all_gather(shards, self.local)
        total = torch.stack(shards).sum(dim=0)
        same = bool(torch.equal(total[:-2], self.table.pack[:-2])) and float(total[-1]) == float(self.table.pack[-1])
        stat, loss_sum, count = self.table.fetch()
        m = FewShotMetric(self.nclass)
        m.stat = stat
        seen = [c for c in synth.val_labels(0, self.dataset) if stat[c].sum() > 0]
        miou = {"miou": round(float(m.mIoU(seen)[1]), 6) if seen else None,
                "biou": round(float(m.mIoU(seen, binary=True)[1]), 6) if seen else None,
                "episodes": int(count), "classes": len(seen), "mean_ce_loss": round(loss_sum / max(count, 1.0), 6),
                "episodes_per_rank": [int(t[-1].item()) for t in shards],
                "source": "the round's tp/fp/fn table, all-reduced inside the timed region (synthetic episodes: the value says "
                          "nothing about PASCAL accuracy)"}
        return same, miou


def sync_replicas(tr):
    """Rank 0's parameters and buffers on every rank (after the rank-local tuning pass moved BatchNorm running statistics)."""
    flat = tr.eng.flat
    dist.broadcast(flat.data, 0)
    model = getattr(tr, "model", None)
    if model is not None:
        for b in model.buffers():
            dist.broadcast(b.data, 0)
        for q in model.parameters():
            if not q.requires_grad:
                dist.broadcast(q.data, 0)


def launch_ranks(n):
    """Start ``n`` copies of this script, one per GPU (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment,
    as torchrun would), wait for them and return the exit code: 0 only if every rank exited 0.  Runs BEFORE this
    process makes any GPU call (it never makes one): the children are fresh processes, nothing is re-exec'ed.  A rank
    that dies takes the job down -- the survivors (blocked in a barrier) are terminated by PID.  Silence watchdog: every
    rank touches a heartbeat file at each phase boundary (``beat``); when NO rank has done so for PEMP_BENCH_SILENCE_S
    seconds (default 300 -- a rank stuck in a collective keeps the others waiting in theirs) all children are
    terminated and the job exits 124."""
    import socket
    import subprocess
    import tempfile
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    silence = float(os.environ.get("PEMP_BENCH_SILENCE_S", "300"))
    hbdir = tempfile.mkdtemp(prefix="pemp_bench_hb_")
    procs, beats = [], []
    threads = str(host_threads_per_rank(n))       # N ranks share the host: numpy / torch-CPU episode synthesis and the eager
    for r in range(n):                            # enqueue loop of every rank run with cores / N threads, not with all of them
        hb = os.path.join(hbdir, f"rank{r}")
        open(hb, "w").close()
        beats.append(hb)
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), PEMP_BENCH_CHILD="1", PEMP_BENCH_HEARTBEAT=hb,
                   OMP_NUM_THREADS=threads, MKL_NUM_THREADS=threads)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    alive = list(procs)
    try:
        while alive:
            time.sleep(0.2)
            for p in list(alive):
                code = p.poll()
                if code is None:
                    continue
                alive.remove(p)
                if code != 0 and rc == 0:
                    rc = code if code > 0 else 1
                    print(f"bench.py: rank {procs.index(p)} exited with {code}; stopping the other ranks", file=sys.stderr)
                    for q in alive:
                        q.terminate()
            if alive and rc == 0:
                quiet = time.time() - max(os.path.getmtime(b) for b in beats)
                if quiet > silence:
                    rc = 124
                    print(f"bench.py: no rank has made progress for {quiet:.0f} s (> {silence:.0f} s); stopping all "
                          f"{len(alive)} rank(s) still running", file=sys.stderr)
                    for q in alive:
                        q.terminate()
                    t_end = time.time() + 10
                    while time.time() < t_end and any(q.poll() is None for q in alive):
                        time.sleep(0.1)
                    break
    finally:
        for q in alive:
            if q.poll() is None:
                q.kill()
        for b in beats:
            try:
                os.unlink(b)
            except OSError:
                pass
        try:
            os.rmdir(hbdir)
        except OSError:
            pass
    return rc


def dry_rows(n, rank, nclass=20):
    """Statistics rows [n, 8] (integer tp/fp/fn counts, a loss sum, a pixel count) and classes of rank ``rank``'s episodes of a
    dry run: what pemp_eval_tail would have left on the device."""
    rng = np.random.RandomState(777 + rank)
    st = np.zeros((n, 8))
    st[:, 2:] = rng.randint(0, 50000, (n, 6))
    st[:, 1] = 401 * 401
    st[:, 0] = rng.rand(n) * st[:, 1]
    return torch.from_numpy(st), torch.from_numpy(rng.randint(1, 6, n).astype(np.int64))


def dry_run(args, world, rank):
    """PEMP_BENCH_DRYRUN=1 (tests, CPU): the control flow of an N-rank run -- rendezvous, barriers, K timed steps, the eval
    round's metric all-reduce inside the timed region, MAX over ranks, the `comm` object, process group gone before rank 0's
    extras, ONE line on rank 0 -- with a sleep in place of the GPU step.  PEMP_BENCH_FAIL_RANK=r makes rank r exit non-zero
    before the first barrier (the launcher must then fail the whole job)."""
    if os.environ.get("PEMP_BENCH_FAIL_RANK") == str(rank):
        raise SystemExit(3)
    beat()
    if os.environ.get("PEMP_BENCH_HANG_RANK") == str(rank):       # a rank that never reaches the collective the others wait in
        time.sleep(3600)
    dev = torch.device("cpu")
    if world > 1:
        dist.init_process_group(os.environ.get("PEMP_BENCH_BACKEND", "gloo"))
        dist.barrier()
    for _ in range(args.warmup):
        time.sleep(0.001)
    rr = RoundReduce(20, dev) if args.mode == "eval" else None
    rows, classes = dry_rows(args.steps * args.batch, rank)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.002 * (1 + rank))
    local_dt = time.perf_counter() - t0           # this rank's own steps, before the round's collective couples the ranks
    if rr is not None:
        rr.reduce(rows, classes)
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    extra = {}
    if world > 1:
        tmax = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    rank_ms = gather_rank_ms(local_dt, args.steps, world, dev)
    if rr is not None:
        same, miou = rr.verify(world)
        extra["miou"] = miou
        comm = comm_object(world, rank_ms, collectives_in_timed_region=1 if world > 1 else 0, allreduce_bytes_per_round=rr.nbytes,
                           allreduce_ms=round(rr.allreduce_ms(), 4), table_equals_sum_of_rank_shards=same)
    else:
        comm = comm_object(world, rank_ms)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        out = {"metric": "episodes/sec (dry run: no GPU work)", "value": round(args.steps * args.batch * world / dt, 2),
               "unit": "episodes/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": "f32", "data": "synthetic", "dry_run": True,
               "config": {"workload": "dry run", "mode": args.mode}, "comm": comm,
               "process_group_alive_at_print": bool(dist.is_initialized())}
        out.update(extra)
        print(json.dumps(out))


# ---------------------------------------------------------------------------------------------
# models and episodes
# ---------------------------------------------------------------------------------------------
def build_model(dev, kind="stage1", shot=1):
    """Random-init model of the reference's architecture with Wgen(1234) weights (no checkpoint exists on either box)."""
    from pemp_amd import synth
    if kind == "stage1":
        from pemp_amd.networks import pemp_stage1 as m
        net = m.ModelClass(None)
        sd = synth.wgen_state_dict_for(net)
    elif kind == "stage2":
        from pemp_amd.networks import pemp_stage2 as m2
        net = m2.ModelClass(shot, 1, None)
        sd = synth.wgen_state_dict_for(net, seed=4321)
    else:
        from pemp_amd.networks import baseline as mb, panet as mp
        net = mb.Baseline(None, backbone="vgg16") if kind == "baseline" else mp.PANet(None, backbone="vgg16")
        sd = synth.wgen_state_dict_for(net)
    net.load_state_dict(sd)
    return (net.to(dev).eval() if dev is not None else net), sd


def episode_pool(dev, shot, batch, rank, n_groups=5, dataset="PASCAL"):
    """n_groups batches of `batch` episodes; all episodes of a batch share one query size so that one
    fused tail launch serves the batch.  Seeds follow the evaluation sampler (test_seed = 5678)."""
    from pemp_amd import synth
    sizes = synth.query_sizes(dataset)
    pool = []
    for g in range(n_groups):
        hw = sizes[g % len(sizes)]
        seeds = [5678 + 1000 * rank + g * batch + b for b in range(batch)]
        b = synth.make_batch(seeds, shot=shot, out_hw=hw, dataset=dataset)
        pool.append(dict(
            sup_img=torch.from_numpy(b["sup_img"]).to(dev), sup_mask=torch.from_numpy(b["sup_mask"]).to(dev),
            qry_img=torch.from_numpy(b["qry_img"]).to(dev), qry_mask=torch.from_numpy(b["qry_mask"][:, 0]).to(dev),
            cls=torch.from_numpy(np.asarray(b["cls"], np.int64)).to(dev), seeds=seeds, hw=hw))
    return pool


# ---------------------------------------------------------------------------------------------
# live per-kernel timing over the C ABI
# ---------------------------------------------------------------------------------------------
CLASS_OF = {
    "pemp_conv2d_nhwc_f32": "conv", "pemp_conv2d_padv_nhwc_f32": "conv", "pemp_conv2d_padv_splitk_nhwc_f32": "conv",
    "pemp_conv2d_wgrad_nhwc_f32": "wgrad",
    "pemp_conv2d_stats_nhwc_f32": "conv", "pemp_bn_stats_partials_f32": "batchnorm", "pemp_conv2d_splitk_nhwc_f32": "conv",
    "pemp_conv2d_bnbwd_nhwc_f32": "conv", "pemp_bn_bwd_partials_f32": "batchnorm", "pemp_bn_apply_mask_f32": "batchnorm",
    "pemp_bn_fwd_partials_f32": "batchnorm", "pemp_bn_bwd_mask_f32": "batchnorm",
    "pemp_bn_stats_f32": "batchnorm", "pemp_bn_apply_f32": "batchnorm", "pemp_bn_bwd_f32": "batchnorm",
    "pemp_relu_bias_bwd_f32": "batchnorm",
    "pemp_mpm_protos_f32": "head", "pemp_masked_avg_pool_f32": "head", "pemp_cosine_proto_max_f32": "head",
    "pemp_eval_tail_f32": "head", "pemp_eval_tail_weighted_f32": "head", "pemp_head_bwd_f32": "head",
    "pemp_head_bwd_dlogits_f32": "head", "pemp_upsample_bilinear_ac_f32": "head", "pemp_argmax_masks_f32": "head",
    "pemp_sgd_clip_step_f32": "optimizer", "pemp_adam_clip_step_f32": "optimizer",
    # round 4: the DropBlock-fused forms, the grouped launch of small evaluation steps, the side figure's bf16 conv
    "pemp_conv2d_dropblock_nhwc_f32": "conv", "pemp_bn_apply_dropblock_f32": "batchnorm", "pemp_conv2d_group_nhwc_f32": "conv",
    "pemp_conv2d_bf16_nhwc": "conv",
}
_RESIDUAL_AT_6 = ("pemp_conv2d_nhwc_f32", "pemp_conv2d_padv_nhwc_f32", "pemp_conv2d_splitk_nhwc_f32", "pemp_conv2d_padv_splitk_nhwc_f32",
                  "pemp_conv2d_dropblock_nhwc_f32", "pemp_conv2d_bf16_nhwc")


class TimedLib:
    """Stand-in for the ctypes handle of libpemp_hip.so that brackets every kernel-launching entry point with a pair of
    HIP events recorded on the stream the launch is made on (the ABI's last argument)."""

    def __init__(self, lib):
        self._lib, self.rec = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.endswith("_bytes") or name in ("pemp_last_error", "pemp_abi_version", "pemp_episode_plan"):
            return fn

        def timed(*a):
            st = a[-1]
            st = st.value if hasattr(st, "value") else st
            stream = torch.cuda.ExternalStream(int(st)) if st else torch.cuda.current_stream()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = fn(*a)
            e1.record(stream)
            self.rec.append((name, e0, e1, a))
            return rc
        return timed


def _conv_work(name, a):
    """(flops, algorithmic bytes, (M, N, K, shortcut)) of one conv / weight-gradient launch from its descriptor."""
    if name == "pemp_conv2d_group_nhwc_f32":       # (n, descriptors, pointer arrays ...): the members' work added up
        fl = nb = 0.0
        m_all, n_max, k_max = 0, 0, 0
        for i in range(int(a[0])):
            d = a[1][i]
            m = d.N * d.Ho * d.Wo
            k = d.KH * d.KW * d.Cin
            fl += 2.0 * m * d.Cout * k
            nb += 4.0 * (d.N * d.H * d.W * d.Cin + m * d.Cout + d.Cout * k)
            m_all, n_max, k_max = m_all + m, max(n_max, d.Cout), max(k_max, k)
        return fl, nb, (m_all, n_max, k_max, False)
    d = a[0]._obj if hasattr(a[0], "_obj") else a[0].contents
    stem = bool(d.flags & 4)
    cin = 3 if stem else d.Cin
    m = d.N * d.Ho * d.Wo
    k = d.KH * d.KW * cin
    flops = 2.0 * m * d.Cout * k
    res = (name in _RESIDUAL_AT_6 and bool(a[6])) or (name == "pemp_conv2d_bnbwd_nhwc_f32" and bool(a[4]))
    outs = (2 if res else 1) + (1 if name == "pemp_conv2d_bnbwd_nhwc_f32" else 0)       # bnbwd also reads the BatchNorm's input z
    nbytes = 4.0 * (d.N * d.H * d.W * d.Cin + m * d.Cout * outs + d.Cout * d.KH * d.KW * d.Cin)
    return flops, nbytes, (m, d.Cout, k, res)


def instrumented(run, reps=3):
    """Run ``run()`` reps+1 times with every C-ABI launch bracketed by HIP events; returns the records of the last
    ``reps`` runs."""
    from pemp_amd import _lib
    real = _lib.load()
    proxy = TimedLib(real)
    _lib._lib = proxy
    try:
        for r in range(reps + 1):
            if r == 1:
                proxy.rec.clear()
            run(r)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
    finally:
        _lib._lib = real
    return proxy.rec


def summarize(rec, reps, step_ms=None):
    """Per-class time / work of a step from the instrumented records, and the roofline object of the conv class."""
    by, layers, entries = {}, {}, {}
    conv_ms = conv_fl = conv_by = 0.0
    conv_n = 0
    for name, e0, e1, a in rec:
        ms = e0.elapsed_time(e1)
        cls = CLASS_OF.get(name, "other")
        c = by.setdefault(cls, {"ms": 0.0, "launches": 0, "gflop": 0.0})
        c["ms"] += ms
        c["launches"] += 1
        en = entries.setdefault(name, [0.0, 0])
        en[0] += ms
        en[1] += 1
        if cls in ("conv", "wgrad"):
            fl, nb, shape = _conv_work(name, a)
            c["gflop"] += fl / 1e9
            conv_ms += ms
            conv_fl += fl
            conv_by += nb
            conv_n += 1
            t = layers.setdefault((cls,) + shape, [0.0, 0.0])
            t[0] += ms
            t[1] += fl
    out = {}
    for cls, c in sorted(by.items(), key=lambda kv: -kv[1]["ms"]):
        e = {"ms_per_step": round(c["ms"] / reps, 3), "launches_per_step": c["launches"] // reps}
        if c["gflop"]:
            e["gflop_per_step"] = round(c["gflop"] / reps, 1)
            e["tflops"] = round(c["gflop"] / c["ms"], 1)
            e["frac_of_fp32_mfma_peak"] = round(c["gflop"] / c["ms"] / PEAK_F32_MFMA_TFLOPS, 4)
        out[cls] = e
    top = sorted(layers.items(), key=lambda kv: -kv[1][0])[:int(os.environ.get("PEMP_BENCH_LAYERS", "6"))]
    by_layer = [{"kind": k[0], "M": k[1], "N": k[2], "K": k[3], "shortcut": k[4], "share": round(v[0] / max(conv_ms, 1e-9), 3),
                 "tflops": round(v[1] / (v[0] * 1e-3) / 1e12, 1)} for k, v in top]
    ach = conv_fl / (conv_ms * 1e-3) / 1e12 if conv_ms else 0.0
    roof = {"bound": "mfma",
            "kernel": "conv_dma2_kernel / conv_dma_kernel / conv_wgrad_kernel (every implicit-GEMM launch of a step: forward, input-gradient, weight-gradient)",
            "achieved": round(ach, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_F32_MFMA_TFLOPS, 4),
            "traffic": None, "algorithmic_bytes_per_launch": int(conv_by / max(conv_n, 1)),
            "launches_per_step": conv_n // reps, "avg_launch_us": round(conv_ms * 1e3 / max(conv_n, 1), 2),
            "gflop_per_step": round(conv_fl / reps / 1e9, 2), "conv_ms_per_step": round(conv_ms / reps, 4),
            "timing": "HIP events around every launch on its own stream, eager pass of the same workload inside bench.py",
            "by_layer": by_layer, "by_class": out,
            "by_entry": {k: {"ms_per_step": round(v[0] / reps, 3), "calls_per_step": v[1] // reps}
                         for k, v in sorted(entries.items(), key=lambda kv: -kv[1][0])[:10]}}
    if step_ms:
        roof["step_effective_tflops"] = round(conv_fl / reps / 1e9 / step_ms, 2)
    return roof


PROFILE_ROUNDS = ("r06", "r05", "r04", "r03")      # committed PMC summaries are looked up newest round first


def attach_pmc(roof, workload_key):
    """HBM bytes and MFMA-pipe utilisation come from rocprofv3 --pmc passes (they cannot be collected in-process).  A
    committed profile is quoted ONLY when it was taken on exactly this conv-engine source (build.conv_digest) and workload."""
    from pemp_amd import build
    digest = build.conv_digest()
    for stem, field, key in (("conv_traffic.json", "traffic", "hbm_bytes_per_launch"),
                             ("mfma_util.json", "mfma_util_pmc_pct", "conv_mfma_util_pct_time_weighted")):
        for rnd in PROFILE_ROUNDS:
            fname = f"{rnd}_{stem}"
            path = os.path.join(ROOT, "profiles", fname)
            if not os.path.exists(path):
                continue
            with open(path) as f:
                rec = json.load(f)
            if rec.get("conv_digest") == digest and rec.get("workload_key") == workload_key:
                roof[field] = rec.get(key)
                roof.setdefault("pmc_source", []).append(f"profiles/{fname} (rocprofv3 --pmc, replayed: same conv-engine source {digest})")
                break
    return roof


def attach_train_pmc(roof, args):
    """The training step's HBM traffic per implicit-GEMM launch (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of
    `bench.py --mode train`, scratch/pmc_train_traffic.py), quoted only next to the kernel sources it was measured on."""
    from pemp_amd import build
    if args.model != "stage1" or args.batch != 4 or args.shot != 1 or not isinstance(roof, dict) or "error" in roof:
        return roof
    digest = build.csrc_digest()
    for rnd in PROFILE_ROUNDS:
        path = os.path.join(ROOT, "profiles", f"{rnd}_train_traffic.json")
        if not os.path.exists(path):
            continue
        with open(path) as f:
            rec = json.load(f)
        if rec.get("csrc_digest") == digest and rec.get("gemm_hbm_bytes_per_launch"):
            roof["traffic"] = rec["gemm_hbm_bytes_per_launch"]
            roof["hbm_GB_per_step_total"] = rec.get("hbm_GB_per_step_total")
            roof.setdefault("pmc_source", []).append(f"profiles/{rnd}_train_traffic.json (rocprofv3 --pmc, same kernel sources {digest})")
            break
    return roof


def cosine_roofline(net, pool):
    """The pixel x prototype cosine kernel against the HBM roofline: 20 back-to-back launches on the step's operands
    between one pair of events (a 25 us kernel bracketed by its own events also measures the launch gap)."""
    from pemp_amd import ops
    last = []
    orig = ops.cosine_proto_max

    def spy(qry, protos, dist_scalar, **kw):
        last[:] = [(qry, protos, dist_scalar, kw)]
        return orig(qry, protos, dist_scalar, **kw)

    ops.cosine_proto_max = spy
    try:
        ep = pool[0]
        with torch.no_grad():
            net.lowres(ep["sup_img"], ep["sup_mask"], ep["qry_img"])
    finally:
        ops.cosine_proto_max = orig
    if not last:
        return None
    qry, protos, ds, kw = last[0]
    b, h, w, c = qry.shape
    nbytes = 4.0 * (b * h * w * c + protos.numel() + 2 * b * h * w)
    nflop = 2.0 * b * h * w * c * protos.shape[1]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        orig(qry, protos, ds, **kw)
        e0.record()
        for _ in range(20):
            orig(qry, protos, ds, **kw)
        e1.record()
    torch.cuda.synchronize()
    cms = e0.elapsed_time(e1) / 20
    gbs = nbytes / (cms * 1e-3) / 1e9
    return {"bound": "hbm", "kernel": "cosine_mfma_kernel (pixel x prototype cosine, MFMA outer product)",
            "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4),
            "avg_launch_us": round(cms * 1e3, 2), "useful_mfma_tflops": round(nflop / (cms * 1e-3) / 1e12, 3)}


# ---------------------------------------------------------------------------------------------
# CPU baseline: the oracle on the host cores, each thread setting in its own process
# ---------------------------------------------------------------------------------------------
def cpu_leg(args):
    """Child process (no GPU call): time the oracle with ``--cpu-leg`` threads and print one JSON object."""
    from oracle import ref_cpu
    from pemp_amd import synth
    threads = int(args.cpu_leg)
    torch.set_num_threads(threads)
    kind = args.model if args.model in ("stage2", "baseline") else "stage1"
    # BASELINE.json configs[0] ("baseline model, VGG-16, 4 test episodes on CPU", entry/baseline.py:46-62 around
    # networks/baseline.py:69-118): the timed episodes are exactly seeds 5678..5681, the
    # warm-up episode in front of them is seed 5677; the other models time 5679.. after warming on 5678
    first = 5677 if kind == "baseline" else 5678
    _, sd = build_model(None, "baseline" if kind == "baseline" else "stage1", 1)
    sd2 = build_model(None, "stage2", args.shot)[1] if kind == "stage2" else None
    t = lambda a: torch.from_numpy(a)
    budget = float(os.environ.get("PEMP_CPU_BUDGET_S", "25"))
    times = []
    if args.mode == "train":
        B = max(1, min(args.batch, int(os.environ.get("PEMP_CPU_TRAIN_BATCH", str(args.batch)))))
        n = 0
        while True:
            b = synth.make_batch([1234 + n * B + i for i in range(B)], shot=args.shot, out_hw=(401, 401))
            ins = (t(b["sup_img"]), t(b["sup_mask"]), t(b["qry_img"]), t(b["qry_mask"][:, 0]))
            t0 = time.time()
            if kind == "stage2":
                with torch.no_grad():
                    prior = ref_cpu.stage1_forward(sd, *ins[:3], (401, 401)).argmax(dim=1, keepdim=True)
                ref_cpu.train_step(sd2, *ins, model="stage2", qry_prior=prior)
            else:
                ref_cpu.train_step(sd, *ins, model="stage1")
            times.append(time.time() - t0)
            n += 1
            if sum(times) > budget or n >= 3:
                break
        per = B
        what = f"{len(times)} train step(s) of {B} episode(s) (oracle/ref_cpu.py train_step: train-mode forward, CE, autograd backward, clip, SGD)"
    else:
        rows = []
        with torch.no_grad():
            for i in range(args.cpu_episodes + 1):
                ep = synth.make_episode(first + i, shot=args.shot, index=i, dataset=args.dataset)
                sup, msk, qry = t(ep["sup_img"])[None], t(ep["sup_mask"])[None], t(ep["qry_img"])[None]
                gt = t(ep["qry_mask"])
                t0 = time.time()
                if kind == "stage2":
                    prior = ref_cpu.stage1_forward(sd, sup, msk, qry, tuple(sup.shape[-2:])).argmax(dim=1, keepdim=True)
                    fwd = lambda a, b, c, hw: ref_cpu.stage2_forward(sd2, a, b, c, prior, hw)
                elif kind == "baseline":
                    fwd = lambda a, b, c, hw: ref_cpu.baseline_forward(sd, a, b, c, hw, backbone="vgg16")
                else:
                    fwd = lambda a, b, c, hw: ref_cpu.stage1_forward(sd, a, b, c, hw)
                pred, loss, _ = ref_cpu.test_step(fwd, (sup, msk, qry), gt)
                dt = time.time() - t0
                if i > 0:                      # first episode warms the allocator / oneDNN primitives
                    times.append(dt)
                # outside the timed region: the episode's tp/fp/fn row (core/metrics.py:9-23) for the mIoU comparison
                m = ref_cpu.FewShotMetric(80)
                m.update(pred, gt.numpy(), [int(ep["cls"])])
                rows.append({"seed": first + i, "index": i, "shot": args.shot, "dataset": args.dataset, "cls": int(ep["cls"]),
                             "counts": [float(v) for v in np.r_[m.stat[0], m.stat[int(ep["cls"])]]], "loss": loss})
                if sum(times) > budget and kind != "baseline":          # configs[0] is exactly its four episodes
                    break
        per = 1
        what = (f"{len(times)} episodes (seeds {first + 1}..{first + len(times)}), oracle/ref_cpu.py test_step"
                + (" over baseline_forward, VGG-16 (BASELINE.json configs[0])" if kind == "baseline" else ""))
    tot = sum(times)
    res = {"value": round(len(times) * per / tot, 3), "threads": threads, "steps": len(times),
           "median_ms": round(float(np.median(times)) * 1e3, 1), "min_ms": round(min(times) * 1e3, 1), "max_ms": round(max(times) * 1e3, 1),
           "sample": f"{what}, torch {torch.__version__} CPU, {threads} thread(s), median {np.median(times) * 1e3:.0f} ms/step "
                     f"(min {min(times) * 1e3:.0f}, max {max(times) * 1e3:.0f})"}
    if args.mode != "train":
        res["episodes"] = rows
    print(json.dumps(res))


def host_description():
    """CPU model string, physical core count (distinct (package, core) pairs of /proc/cpuinfo), logical CPUs, and the CPUs this
    process may run on (the CPU baseline states where it was measured)."""
    model, cores, logical = None, set(), 0
    try:
        phys = core = None
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "processor":
                logical += 1
                phys = core = None
            elif k == "model name" and model is None:
                model = v
            elif k == "physical id":
                phys = v
            elif k == "core id":
                core = v
                cores.add((phys, core))
    except OSError:
        pass
    try:
        allowed = len(os.sched_getaffinity(0))
    except AttributeError:
        allowed = os.cpu_count() or 1
    return {"cpu_model": model, "physical_cores": len(cores) or None, "logical_cpus": logical or os.cpu_count(),
            "cpus_allowed": allowed, "share_per_gpu": host_threads_per_rank(1)}


def cpu_baseline(args):
    """Oracle legs in child processes, one per thread setting (switching set_num_threads inside one process inflates the
    timings): ALL PHYSICAL cores the process may use, this box's per-GPU share
    (<= 16 threads: what one rank of an 8-GPU job has), and one thread.  `value` / `cores` = the fastest leg and the threads it
    used; every leg is listed with its median / min / max step time; `host` names the CPU."""
    import subprocess
    host = host_description()
    allowed = host["cpus_allowed"]
    phys = min(host["physical_cores"] or allowed, allowed)
    share = max(1, min(allowed, int(os.environ.get("PEMP_CPU_THREADS", "16"))))
    settings = []
    for th in (phys, share, 1):
        if th not in settings:
            settings.append(th)
    legs = {}
    for threads in settings:
        env = dict(os.environ, OMP_NUM_THREADS=str(threads), MKL_NUM_THREADS=str(threads), HIP_VISIBLE_DEVICES="")
        if threads == 1:
            env.setdefault("PEMP_CPU_BUDGET_S", "20")
            env.setdefault("PEMP_CPU_TRAIN_BATCH", "1")
        else:
            env.setdefault("PEMP_CPU_BUDGET_S", "20")
        n_ep = args.cpu_episodes if threads > 1 or args.model == "baseline" else max(2, min(args.cpu_episodes, 10))
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-leg", str(threads), "--mode", args.mode, "--model", args.model,
               "--shot", str(args.shot), "--batch", str(args.batch), "--dataset", args.dataset, "--cpu-episodes", str(n_ep)]
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            legs[threads] = json.loads(line[-1]) if r.returncode == 0 and line else {"error": (r.stderr or r.stdout)[-300:]}
        except subprocess.TimeoutExpired:
            legs[threads] = {"error": "timeout"}
        beat()
    good = {t: l for t, l in legs.items() if "error" not in l and t > 1} or {t: l for t, l in legs.items() if "error" not in l}
    if not good:
        return {"error": str(legs), "host": host}
    best = max(good, key=lambda t: good[t]["value"])
    main = good[best]
    out = {"value": main["value"], "unit": "episodes/s", "cores": best, "kind": "port", "sample": main["sample"], "host": host,
           "legs": [{"threads": t, "value": l.get("value"), "median_ms": l.get("median_ms"), "min_ms": l.get("min_ms"),
                     "max_ms": l.get("max_ms"), "steps": l.get("steps"), "error": l.get("error")} for t, l in legs.items()]}
    with_rows = [l["episodes"] for l in legs.values() if "episodes" in l]
    if with_rows:
        out["episodes"] = max(with_rows, key=len)      # per-episode tp/fp/fn rows: consumed by miou_vs_cpu, not printed
    one = legs.get(1, {})
    out["one_thread"] = {"value": one.get("value"), "cores": 1, "sample": one.get("sample", one.get("error"))}
    return out


# ---------------------------------------------------------------------------------------------
# staging-inclusive figure (SURVEY.md §8d ii)
# ---------------------------------------------------------------------------------------------
def end_to_end(net, args, dev):
    """Episodes/s INCLUDING input staging: decoded uint8 samples in host memory -> one pinned blob per step -> async H2D
    -> Pillow-exact resize/normalise on the device (pemp_episode_preprocess) -> the same eval step, double-buffered on a
    side stream.  JPEG decode is not included (no dataset)."""
    from pemp_amd import ops
    from pemp_amd.data_kits import synth_u8
    from pemp_amd.data_kits.episode import EpisodeLoader, EpisodeTransform, test_samples
    B, S = args.batch, args.shot
    sizes = [(375, 500), (333, 500), (500, 375), (366, 500), (457, 500)]
    raw = []
    for g in range(3):
        hs, ws = sizes[g]
        imgs = [(synth_u8.image(10 * g + k, hs, ws), synth_u8.mask(10 * g + k, hs, ws)) for k in range(S + 1)]
        batch = []
        for _ in range(B):
            batch += test_samples(imgs[:S], imgs[S:], 401, 401)
        raw.append(batch)
    steps = max(6, min(args.steps, 20))
    ws_cache = {}

    def batches():
        for i in range(steps + 2):
            yield raw[i % len(raw)]

    def consume(out):
        img, planes, labels = out
        img = img.view(B, S + 1, 3, 401, 401)
        with torch.no_grad():
            pred, _ = net.lowres_graphed(img[:, :S].contiguous(), planes.view(B, S, 2, 401, 401), img[:, S:].contiguous())
            return ops.eval_tail(pred, torch.stack(labels), ws_cache=ws_cache)[1]

    loader = EpisodeLoader(batches(), EpisodeTransform(401, 401, device=dev))
    stats = [consume(next(loader)) for _ in range(2)]                      # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for out in loader:
        stats.append(consume(out))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = torch.stack(stats).cpu().numpy()
    assert np.isfinite(st).all() and (st[..., 1] > 0).all()
    per_ep = sum(s.img.size + (s.mask.size if s.mask is not None else 0) for s in raw[0]) / B
    return {"value": round(steps * B / dt, 2), "unit": "episodes/s", "ms_per_step": round(dt / steps * 1e3, 3),
            "h2d_bytes_per_episode": int(per_ep),
            "path": "host uint8 (decoded) -> pinned blob -> async H2D -> device resize/normalise -> eval step; "
                    "double-buffered on a side stream; JPEG decode excluded"}


def single_episode(net, dev, args, n=120):
    """The reference's own protocol: ONE episode per test_step (data_kits/datasets.py:23 test_bs = 1,
    entry/pemp_stage1.py:47-53), no host synchronisation per episode (statistics are fetched once per round).
    ``value``: with the opt-in split-K conv variants for the 5202-row layers (Evaluator(splitk=True): equal to the batched
    step to rounding); ``exact``: the default, bit-identical variants (a one-episode step equals the batched step bit for
    bit).  ``in_flight`` > 1: episodes issued round-robin over that many engine replicas on their own streams."""
    from pemp_amd.entry.pemp_stage1 import Evaluator
    pool = episode_pool(dev, args.shot, 1, 0, n_groups=5, dataset=args.dataset)
    eps = [((p["sup_img"], p["sup_mask"], p["qry_img"]), p["qry_mask"][None]) for p in pool]
    lanes_n = int(os.environ.get("PEMP_EVAL_LANES", "4"))

    def run(lanes, splitk):
        ev = Evaluator(net, device=dev, lanes=lanes, splitk=splitk)
        ev.test_steps_device([eps[i % len(eps)] for i in range(2 * len(eps) * lanes)])     # warm-up: graphs captured
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = ev.test_steps_device([eps[i % len(eps)] for i in range(n)])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st = rows.cpu().numpy()
        assert np.isfinite(st).all() and (st[:, 1] > 0).all()
        return round(n / dt, 2), round(dt / n * 1e3, 4)

    out = {}
    out["value"], out["ms_per_episode"] = run(1, True)
    out[f"value_{lanes_n}_in_flight"], out[f"ms_per_episode_{lanes_n}_in_flight"] = run(lanes_n, True)
    ex1, exn = run(1, False), run(lanes_n, False)
    out["exact"] = {"value": ex1[0], "ms_per_episode": ex1[1], f"value_{lanes_n}_in_flight": exn[0],
                    "what": "the default conv variants (all bit-identical): one episode per step == the batched step bit for bit"}
    out["conv_variants"] = ("`value` / `value_N_in_flight`: split-K allowed for layers of <= 12000 output rows (Evaluator(splitk=True) / "
                            "PEMP_EVAL_SPLITK=1; opt-in); `exact`, `reference_body`, `reference_body_pinned`: the default exact variants")
    out["exact"]["conv_variants"] = "exact"
    # The reference's Evaluator.test_step body as written (entry/pemp_stage1.py:48-53): host tensors in, three .cuda()
    # copies, forward, loss.item() and argmax .cpu().numpy() out -- two host synchronisations per episode.
    ev = Evaluator(net, device=dev, splitk=False)
    host = [(tuple(x.cpu() for x in ins), msk.cpu()) for ins, msk in eps]
    for ins, msk in host:
        ev.test_step(ins, msk)
    torch.cuda.synchronize()
    m = max(20, n // 2)
    t0 = time.perf_counter()
    for i in range(m):
        pred, loss = ev.test_step(*host[i % len(host)])
    dt = time.perf_counter() - t0
    assert pred.ndim == 3 and np.isfinite(loss)
    out["reference_body"] = {"value": round(m / dt, 2), "ms_per_episode": round(dt / m * 1e3, 4), "conv_variants": "exact",
                             "what": "Evaluator.test_step as the reference writes it: host tensors -> 3 H2D copies -> forward -> "
                                     "loss float + argmax numpy on the host, every episode (pageable host memory, no overlap); "
                                     "exact conv variants since round 5 (rounds <= 4: split-K allowed -- not like for like)"}
    # the same body with the episode's host tensors in PINNED memory (what a DataLoader(pin_memory=True) hands over)
    pinned = [(tuple(x.pin_memory() for x in ins), msk) for ins, msk in host]
    for ins, msk in pinned:
        ev.test_step(ins, msk)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(m):
        pred, loss = ev.test_step(*pinned[i % len(pinned)])
    dt = time.perf_counter() - t0
    out["reference_body_pinned"] = {"value": round(m / dt, 2), "ms_per_episode": round(dt / m * 1e3, 4), "conv_variants": "exact",
                                    "what": "the same test_step body, inputs in pinned host memory"}
    out.update(unit="episodes/s", episodes_per_step=1,
               protocol="one episode per test_step (reference data.test_bs = 1), hipGraph replay, statistics fetched once per round")
    return out


class ResidentEpisodes:
    """``Evaluator.start_eval_loop``'s dataset protocol over episodes already resident in HBM: task ``i`` of round ``r`` is
    episode ``(r * test_n + i) mod P`` of a pool of P distinct E(seed) episodes (generating 5000 distinct 401 x 401 episodes on
    the host would take minutes; the device work per episode does not depend on which one it is).  Episodes of the five
    query formats alternate, as in the reference's loader."""

    def __init__(self, pool, test_n):
        per = [[((g["sup_img"][b:b + 1], g["sup_mask"][b:b + 1], g["qry_img"][b:b + 1]), g["qry_mask"][b:b + 1][None], c)
                for b, c in enumerate(g["cls"].tolist())] for g in pool]
        self.eps = [grp[j] for j in range(max(len(g) for g in per)) for grp in per if j < len(grp)]
        if test_n % len(self.eps) == 0 and len(self.eps) > 2:
            self.eps = self.eps[:-2]               # rounds then differ in which episodes they hold
        self.test_n, self.round = test_n, -1
        self.shot, self.height, self.width = pool[0]["sup_img"].shape[1], *pool[0]["sup_img"].shape[-2:]

    def reset_sampler(self):
        self.round = -1

    def sample_tasks(self):
        self.round += 1

    def __len__(self):
        return self.test_n

    def task(self, i):
        ins, msk, c = self.eps[(self.round * self.test_n + i) % len(self.eps)]
        return ins, msk, torch.tensor([c])


def protocol_5x1000(net, pool, dev, args, rounds=5, test_n=1000, lanes=4):
    """The reference's evaluation protocol (core/solver.py:47-50 te.epochs = 5, data_kits/datasets.py:23,27 test_bs = 1,
    test_n = 1000; core/base_trainer.py:59-102): 5 rounds x 1000 episodes, one episode per test_step, mIoU per round, through
    ``Evaluator.start_eval_loop`` -- the loop the ``test`` command runs -- with ``lanes`` steps in flight."""
    from pemp_amd.entry.pemp_stage1 import Evaluator
    nclass = 20 if args.dataset == "PASCAL" else 80
    data = ResidentEpisodes(pool, test_n)
    ev = Evaluator(net, device=dev, lanes=lanes, splitk=False)      # the exact (bit-identical) variants: since round 5's hybrid launch also the faster ones
    warm = ResidentEpisodes(pool, 8 * lanes)
    ev.start_eval_loop(warm, nclass, 0, te_epochs=1, batch=1, dataset_name=args.dataset)      # graphs of every lane / label size
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss, miou, biou = ev.start_eval_loop(data, nclass, 0, te_epochs=rounds, batch=1, dataset_name=args.dataset)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return {"rounds": rounds, "episodes_per_round": test_n, "test_bs": 1, "in_flight": lanes,
            "episodes_per_s": round(rounds * test_n / wall, 2), "wall_s": round(wall, 3),
            "timer_cps": round(ev.cps, 2),
            "miou_per_round": [round(float(np.nanmean(r)), 6) for r in ev.round_miou],
            "biou_per_round": [round(float(np.nanmean(r)), 6) for r in ev.round_biou],
            "miou": round(float(np.nanmean(miou)), 6), "biou": round(float(np.nanmean(biou)), 6), "mean_ce_loss": round(float(loss), 6),
            "distinct_episodes": len(data.eps),
            "conv_variants": "exact (rounds <= 4 of this project ran this figure with split-K allowed: not like for like with BENCH_r04)",
            "what": "Evaluator.start_eval_loop: 5 rounds x 1000 single-episode test_steps (the default, bit-identical conv variants), per-round "
                    "device-side metric table + one fetch; timer_cps = calls / time inside test_step (the reference's Timer), "
                    "episodes_per_s = wall clock of the whole loop; episodes cycle through a resident pool of synthetic E(seed) "
                    "episodes (the mIoU says nothing about PASCAL accuracy)"}


PEAK_BF16_MFMA_TFLOPS = 2500.0   # MI355X_MICROARCH.md, dense bf16 matrix peak (the figure below is priced against it, not the fp32 one)


def bf16_variant(run, dev, args, steps=10, warmup=3):
    """SIDE FIGURE, never `value`, never `roofline`: the same eval step with bf16 OPERANDS in the encoder (bf16 activations and
    weights between the fp32 stem and the fp32 prototype head, fp32 accumulation on v_mfma_f32_32x32x16_bf16;
    model.precision("bf16")) -- what the exact-fp32 arithmetic of the product path costs, and what giving it up would move: the
    mIoU of one round over every resident episode of the run's pool on both precisions, and the arg-max pixels that flip."""
    from pemp_amd.core.metrics import FewShotMetric
    from pemp_amd import ops, synth
    net, pool = run.net, run.pool
    r = EvalRunner(dev, 0, "stage1", args.shot, args.batch, args.dataset, steps, net=net, pool=pool, precision="bf16")
    dt, ml, _ = r.timed(steps, warmup, 1, dev)
    ms = dt / steps * 1e3
    nclass = 20 if args.dataset == "PASCAL" else 80
    res, ws = {}, {}
    for prec in ("f32", "bf16"):
        m, ams, loss = FewShotMetric(nclass), [], []
        for ep in pool:
            with net.precision(prec), torch.no_grad():
                pred, _ = net.lowres_graphed(ep["sup_img"], ep["sup_mask"], ep["qry_img"])
                am, st, _ = ops.eval_tail(pred, ep["qry_mask"], ws_cache=ws)
            st = st.cpu().numpy()
            m.update_counts(st[:, 2:], ep["cls"].tolist())
            loss += list(st[:, 0] / st[:, 1])
            ams.append(am.clone())
        seen = [c for c in synth.val_labels(0, args.dataset) if m.stat[c].sum() > 0]
        res[prec] = (float(m.mIoU(seen)[1]), float(m.mIoU(seen, binary=True)[1]), float(np.mean(loss)), ams)
    flips = sum(int((a != b).sum()) for a, b in zip(res["f32"][3], res["bf16"][3]))
    pixels = sum(a.numel() for a in res["f32"][3])
    gflop = 129.87 * args.batch if args.shot == 1 else None
    out = {"dtype": "bf16 operands / fp32 accumulate (encoder convs between the fp32 stem and the fp32 head)",
           "what": "side figure only: never `value`, never `roofline` -- what the exact-fp32 MFMA arithmetic of the product path costs",
           "episodes_per_step": args.batch, "steps": steps, "warmup": warmup, "ms_per_step": round(ms, 4),
           "episodes_per_s": round(args.batch / ms * 1e3, 2),
           "round_episodes": sum(len(ep["cls"]) for ep in pool),
           "miou_f32": round(res["f32"][0], 6), "miou_bf16": round(res["bf16"][0], 6), "delta_miou": round(abs(res["f32"][0] - res["bf16"][0]), 6),
           "biou_f32": round(res["f32"][1], 6), "biou_bf16": round(res["bf16"][1], 6), "delta_biou": round(abs(res["f32"][1] - res["bf16"][1]), 6),
           "mean_ce_loss_f32": round(res["f32"][2], 6), "mean_ce_loss_bf16": round(res["bf16"][2], 6),
           "argmax_flips": flips, "pixels": pixels, "argmax_flip_share": round(flips / max(pixels, 1), 6),
           "dataset": args.dataset}
    if gflop:
        out["effective_tflops"] = round(gflop / ms, 1)
        out["frac_of_bf16_mfma_peak"] = round(gflop / ms / PEAK_BF16_MFMA_TFLOPS, 4)
    return out


def side_cedt_eval(run, dev, args, steps=10, warmup=3):
    """The eval step with loss = cedt (CELossDT: boundary + exact distance transform + weighted CE on the device, all inside the
    timed region; reference entry/pemp_stage1.py:51, core/losses.py:17-43) next to the same step with loss = ce, measured the
    same way on the headline run's engine and episodes."""
    res = {}
    for kind in ("ce", "cedt"):
        r = EvalRunner(dev, 0, "stage1", args.shot, args.batch, args.dataset, steps, loss=kind, net=run.net, pool=run.pool)
        dt, ml, _ = r.timed(steps, warmup, 1, dev)
        res[kind] = (dt / steps * 1e3, ml)
    ms, ce_ms = res["cedt"][0], res["ce"][0]
    return {"workload": "pemp_stage1 eval test_step with loss=cedt, %d episodes/step" % args.batch, "steps": steps, "warmup": warmup,
            "ms_per_step": round(ms, 4), "ce_ms_per_step": round(ce_ms, 4), "delta_ms_vs_ce": round(ms - ce_ms, 4),
            "episodes_per_s": round(args.batch / ms * 1e3, 2), "mean_weighted_ce_loss": round(res["cedt"][1], 6),
            "mean_ce_loss": round(res["ce"][1], 6)}


def side_cedt_train(keep, dev, steps=10, warmup=3):
    """The train step with loss = cedt (reference entry/pemp_stage1.py:60, scripts/pemp_stage1.sh:11) on the `train` object's
    trainer and batches, next to its loss = ce figure."""
    from pemp_amd.core import losses
    tr, pool = keep["trainer"], keep["pool"]
    tr.loss_obj = losses.get({"loss": "cedt", "sigma": 5.0})
    dt, host_ms, ls, _, _ = timed_train_steps(tr, pool, steps, warmup, 1, dev)
    ms = dt / steps * 1e3
    B = pool[0][0].shape[0]
    return {"workload": "pemp_stage1 train_step with loss=cedt, %d episodes/step" % B, "steps": steps, "warmup": warmup,
            "ms_per_step": round(ms, 3), "ce_ms_per_step": round(keep["step_ms"], 3), "delta_ms_vs_ce": round(ms - keep["step_ms"], 3),
            "episodes_per_s": round(B / ms * 1e3, 2), "last_loss": round(float(ls[-1]), 5)}


# ---------------------------------------------------------------------------------------------
# training step (--mode train, and the ``train`` object of the default line)
# ---------------------------------------------------------------------------------------------
def stub_trainer(rank):
    """PEMP_BENCH_STUB=1 (tests; CPU, gloo): the REAL ``Stage1Trainer.train_step`` / ``reduce_gradients`` / ``GradBuckets``
    control flow -- bucket hooks fired during "backward", finished in the optimizer step, the ``collectives`` switch --
    over a 64 K-float flat buffer, with two lines of arithmetic in place of the HIP kernels."""
    from pemp_amd.train_engine import GradBuckets, Stage1Trainer

    class _NS:
        pass

    class Stub(Stage1Trainer):
        def __init__(self):
            n = 1 << 16
            f, e = _NS(), _NS()
            f.data, f.grad, f.side_stream = torch.zeros(n), torch.zeros(n), None
            e.flat, e.ws = f, {}
            e.buckets = GradBuckets(f.grad, [n // 4, n // 2, 3 * n // 4], min_bytes=n)        # four buckets of 64 KB
            self.eng, self.use_graph, self.optimizer, self.calls, self.device = e, False, None, 0, torch.device("cpu")     # (no hipGraphs on the CPU: --train-graph is plumbing only here)

        def forward_backward(self, *ins):
            f, b = self.eng.flat, self.eng.buckets
            n = f.grad.numel()
            f.grad.fill_(float(rank + 1))                   # rank r's gradient: r + 1 everywhere
            for lo in (3 * n // 4, n // 2, n // 4, 0):      # "backward" finishes the buffer from its end
                b.ready_from(lo)
            self.calls += 1
            return torch.tensor(float(self.calls)), None

        def apply_update(self, scale):
            self.eng.flat.data.add_(self.eng.flat.grad * scale, alpha=-0.1)

    return Stub()


def make_trainer(model, shot, dev, rank, use_graph=False, loss="ce"):
    if os.environ.get("PEMP_BENCH_STUB"):
        return stub_trainer(rank)
    from pemp_amd.train_engine import Stage1Trainer
    net, _ = build_model(None, "stage1", 1)
    if model == "stage2":          # frozen stage-1 prior + stage-2 step (entry/pemp_stage2.py:72-83)
        from pemp_amd.train_stage2 import Stage2Trainer
        net2, _ = build_model(None, "stage2", shot)
        return Stage2Trainer(net.to(dev).eval(), net2, device=dev, use_graph=use_graph, loss=loss)
    # eager by default: the weight-gradient kernels run on a side stream concurrently with the input-gradient chain
    return Stage1Trainer(net, device=dev, use_graph=use_graph, loss=loss)


def train_pool(dev, rank, shot, B, groups=3):
    from pemp_amd import synth
    pool = []
    for g in range(groups):
        b = synth.make_batch([1234 + 1000 * rank + g * B + i for i in range(B)], shot=shot, out_hw=(401, 401))
        pool.append(tuple(torch.from_numpy(b[k]).to(dev) for k in ("sup_img", "sup_mask", "qry_img")) +
                    (torch.from_numpy(b["qry_mask"][:, 0]).to(dev),))
    return pool


def device_sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def timed_train_steps(tr, pool, steps, warmup, world, dev):
    """W untimed + K timed ``train_step`` calls between barriers
    -> (seconds [MAX over ranks], host ms per step, losses, this rank's own seconds, exposed communication ms per step)."""
    if world > 1:
        # kernel variants are timed by rank 0 only and broadcast (pemp_amd.ops.tuned_by_rank0).  That pass is rank-local (no
        # gradient collective: the ranks do not run it at the same time) and has no optimizer step; what it does move --
        # BatchNorm running statistics -- is brought back in line by broadcasting rank 0's replica afterwards, so that the
        # timed run starts from identical replicas and is the data-parallel run of ONE model.
        from pemp_amd import ops

        def local_pass():
            tr.collectives = False
            try:
                tr.forward_backward(*pool[0])
                device_sync(dev)
            finally:
                tr.collectives = True
        ops.tuned_by_rank0(local_pass)
        sync_replicas(tr)
        beat()
    for i in range(warmup):
        tr.train_step(*pool[i % len(pool)])
        beat()

    def barrier():
        if world > 1:
            dist.barrier()
        device_sync(dev)

    barrier()
    tr.comm_log = []
    t0 = time.perf_counter()
    losses = []
    host = 0.0
    cpu0 = time.process_time()
    for i in range(steps):
        h0 = time.perf_counter()
        losses.append(tr.train_step(*pool[i % len(pool)]))
        host += time.perf_counter() - h0
    timed_train_steps.cpu_ms = (time.process_time() - cpu0) / steps * 1e3      # CPU time of ALL this process' threads while it enqueued
    device_sync(dev)
    local_dt = time.perf_counter() - t0
    barrier()
    dt = time.perf_counter() - t0
    beat()
    if world > 1:
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    exposed = tr.exposed_comm_ms()
    tr.comm_log = None
    ls = torch.stack(losses).cpu().numpy()
    assert np.isfinite(ls).all()
    return dt, host / steps * 1e3, ls, local_dt, exposed


def train_end_to_end(tr, dev, B=4, S=1, steps=10, warmup=3):
    """Training episodes/s INCLUDING input staging ("end-to-end"): decoded uint8 samples of
    PASCAL-like sizes in host memory -> the reference's augmentation DRAWS on the host (data_kits/pascal_voc.py:184-240: scale
    1..1.5, flip, colour-jitter order and factors, crop_obj window -- pemp_amd.data_kits.episode.train_samples) -> one pinned
    blob per step -> async H2D -> Pillow-exact resize / flip / jitter / crop / normalise on the device
    (pemp_episode_preprocess) -> the same train_step, the next batch staged on a side stream while the step runs.  JPEG decode
    is not included (no dataset).  Stage 1 only."""
    import random
    from pemp_amd.data_kits import synth_u8
    from pemp_amd.data_kits.episode import EpisodeLoader, EpisodeTransform, train_samples
    sizes = [(375, 500), (333, 500), (500, 375), (366, 500), (457, 500)]
    rng = random.Random(4321)
    imgs = [[(synth_u8.image(100 * g + k, *sizes[g]), synth_u8.mask(100 * g + k, *sizes[g])) for k in range(S + 1)] for g in range(len(sizes))]
    host = 0.0

    def batches():
        nonlocal host
        for i in range(warmup + steps):
            h0 = time.perf_counter()
            batch = []
            for e in range(B):
                im = imgs[(i * B + e) % len(imgs)]
                batch += train_samples(im[:S], im[S:], 401, 401, rng)
            host += time.perf_counter() - h0
            yield batch

    loader = EpisodeLoader(batches(), EpisodeTransform(401, 401, device=dev))
    losses, t0 = [], None
    for i, (img, planes, labels) in enumerate(loader):
        if i == warmup:
            torch.cuda.synchronize()
            t0, host = time.perf_counter(), 0.0
        img = img.view(B, S + 1, 3, 401, 401)
        losses.append(tr.train_step(img[:, :S].contiguous(), planes.view(B, S, 2, 401, 401), img[:, S:].contiguous(), torch.stack(labels)))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ls = torch.stack(losses).cpu().numpy()
    assert np.isfinite(ls).all() and len(losses) == warmup + steps
    per_ep = sum(a.size + b.size for a, b in imgs[0])
    return {"value": round(steps * B / dt, 2), "unit": "episodes/s", "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps,
            "host_augment_draw_ms_per_step": round(host / steps * 1e3, 3), "h2d_bytes_per_episode": int(per_ep),
            "path": "host uint8 (decoded) -> augmentation draws (scale, flip, jitter, crop_obj) -> pinned blob -> async H2D -> device "
                    "resize/flip/jitter/crop/normalise -> train_step; next batch staged on a side stream; JPEG decode excluded"}


def train_comm(tr, world, rank_ms, exposed):
    """The `comm` object of a training line: the gradient exchange of one step as the trainer issues it."""
    flat = tr.eng.flat
    buckets = [[int(lo), int(hi)] for lo, hi in tr.eng.buckets.buckets]
    return comm_object(
        world, rank_ms, collective="all_reduce(SUM) per gradient bucket, launched as the backward pass finishes the bucket "
                                   "(GradBuckets), mean + clip + SGD fused behind the last one",
        allreduce_bytes_per_step=int(flat.grad.numel() * flat.grad.element_size()) if world > 1 else 0,
        gradient_elements=int(flat.grad.numel()), buckets=buckets,
        bucket_bytes=[(hi - lo) * 4 for lo, hi in buckets], collectives_per_step=len(buckets) if world > 1 else 0,
        exposed_comm_ms=None if exposed is None else round(exposed, 4),
        exposed_comm_what="HIP events around reduce_gradients() on the step's stream: launch of the last bucket + wait for all")


def train_roofline(tr, pool, step_ms, reps=2):
    """Per-kernel durations of the training step: an instrumented eager pass on ONE stream (kernels of the two streams
    overlap in the timed step) and -- it may run on one rank alone -- with every gradient collective switched off
    (``collectives`` False: no bucket hook, no all-reduce in the optimizer step)."""
    flat = tr.eng.flat
    side, bside, ug, coll = flat.side_stream, tr.eng.buckets.side, tr.use_graph, tr.collectives
    flat.side_stream = tr.eng.buckets.side = None
    tr.use_graph, tr.collectives = False, False
    try:
        rec = instrumented(lambda r: tr.train_step(*pool[r % len(pool)]), reps=reps)
    finally:
        flat.side_stream, tr.eng.buckets.side, tr.use_graph, tr.collectives = side, bside, ug, coll
    r = summarize(rec, reps, step_ms)
    r["note"] = ("per-kernel durations from a single-stream, rank-local eager pass; the timed step overlaps the weight-gradient "
                 "kernels with the input-gradient chain on a side stream%s (step_effective_tflops = conv flops / timed step)"
                 % (" and replays a chain of hipGraph segments" if ug else ""))
    return r


def main_train(args, world, rank, dev):
    """Trainer.train_step (reference entry/pemp_stage1.py:57-65) on `--batch` episodes per rank (the reference's
    data.bs = 4), data-parallel: bucketed flat-gradient all-reduce over RCCL, overlapped with backward."""
    use_graph = args.train_graph
    s2 = args.model == "stage2"
    tr = make_trainer(args.model, args.shot, dev, rank, use_graph, loss=args.loss)
    B = args.batch
    pool = train_pool(dev, rank, args.shot, B)
    beat()
    dt, host_ms, ls, local_dt, exposed = timed_train_steps(tr, pool, args.steps, args.warmup, world, dev)
    rank_ms = gather_rank_ms(local_dt, args.steps, world, dev)
    comm = train_comm(tr, world, rank_ms, exposed)
    # every rank's own host time per step (Python enqueue of the step's launches; ``--train-graph``: of its hipGraph chain): a
    # rank whose figure approaches its rank_ms_per_step is enqueue-bound, not communication-bound -- the eager step enqueues
    # ~450 launches from ONE host thread per rank, eight of them share the node's cores
    host_all = gather_rank_ms(host_ms * 1e-3 * args.steps, args.steps, world, dev)
    cpu_all = gather_rank_ms(getattr(timed_train_steps, "cpu_ms", 0.0) * 1e-3 * args.steps, args.steps, world, dev)
    comm["host_enqueue_ms_per_step"] = {"max": round(max(host_all), 3), "all": [round(v, 3) for v in host_all],
                                        "of_step": round(max(h / max(r, 1e-9) for h, r in zip(host_all, rank_ms)), 3),
                                        "cpu_ms_all": [round(v, 3) for v in cpu_all],
                                        "note": "wall time inside train_step (includes waiting for room in the launch queue while the GPU "
                                                "is the bottleneck); cpu_ms_all = process CPU time over the same calls, all threads"}
    if world > 1:
        # the process group ends HERE: what rank 0 measures below is rank-local, and the other ranks leave instead of spinning
        # in a barrier kernel on their GPUs for its whole duration
        dist.barrier()
        dist.destroy_process_group()
    if rank != 0:
        return
    if args.dump_outputs:           # before the roofline pass below, which takes more steps
        dump_outputs(args.dump_outputs, {"loss": ls[-1], "weights": tr.eng.flat.data})
    step_ms = dt / args.steps * 1e3
    out = {
        "metric": "train episodes/sec (PEMP %s train_step, ResNet-50, %d-shot, 401x401)" % ("stage-2" if s2 else "stage-1", args.shot),
        "value": round(args.steps * B * world / dt, 2), "unit": "episodes/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(step_ms, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": ("pemp_stage2 train_step (frozen stage-1 prior pass, batch-stat BN, CM, Dropout2d 0.5, %s, SGD), "
                                if s2 else "pemp_stage1 train_step (batch-stat BN, DropBlock 0.1, %s, clip 1.1, SGD), ") % args.loss.upper() +
                               "ResNet-50, %d-shot, 401x401, %d episodes/rank/step, synthetic E(seed) episodes + Wgen weights" % (args.shot, B),
                   "episodes_per_step": B, "shot": args.shot, "loss": args.loss, "hipgraph": use_graph,
                   "host_enqueue_ms_per_step": round(host_ms, 2),
                   "first_loss": round(float(ls[0]), 5), "last_loss": round(float(ls[-1]), 5)},
        "comm": comm}
    if os.environ.get("PEMP_BENCH_STUB"):
        out["config"]["stub_weight"] = float(tr.eng.flat.data[0])      # before the rank-local roofline pass
        out["process_group_alive_at_roofline"] = bool(dist.is_initialized())
    if not args.full:               # a plain run ends with the headline
        print(json.dumps(out))
        return

    def guarded(key, fn):
        try:
            out[key] = fn()
        except Exception as exc:  # noqa: BLE001
            out[key] = {"error": f"{type(exc).__name__}: {exc}"}
        beat()

    if not args.no_roofline:
        # rank 0 alone, after the process group is gone; the pass is collective-free by construction as well
        # (train_roofline switches every collective of the step off)
        guarded("roofline", lambda: attach_train_pmc(train_roofline(tr, pool, step_ms), args))
    if world == 1 and not s2 and not os.environ.get("PEMP_BENCH_STUB"):
        guarded("end_to_end", lambda: train_end_to_end(tr, dev, B, args.shot, steps=max(6, min(args.steps, 20))))
    if world == 1 and args.cpu_episodes > 0 and not os.environ.get("PEMP_BENCH_STUB"):
        guarded("cpu_baseline", lambda: cpu_baseline(args))
    print(json.dumps(out))


def side_train(dev, model="stage1", shot=1, batch=4, steps=10, warmup=4, keep=None):
    """The training step (BASELINE.json configs[2]; the reference's data.bs = 4) measured inside the default run, so that it
    sits under the driver's clock too: same code as ``--mode train``, compact record."""
    tr = make_trainer(model, shot, dev, 0)
    pool = train_pool(dev, 0, shot, batch)
    dt, host_ms, ls, _, _ = timed_train_steps(tr, pool, steps, warmup, 1, dev)
    step_ms = dt / steps * 1e3
    r = train_roofline(tr, pool, step_ms, reps=1)
    eff = r.get("step_effective_tflops", 0.0)
    if keep is not None:
        keep.update(trainer=tr, pool=pool, step_ms=step_ms)
    r = attach_train_pmc(r, argparse.Namespace(model=model, batch=batch, shot=shot))
    try:
        e2e = train_end_to_end(tr, dev, batch, shot, steps=steps) if model == "stage1" else None
    except Exception as exc:  # noqa: BLE001
        e2e = {"error": f"{type(exc).__name__}: {exc}"}
    return {"end_to_end": e2e, "workload": "pemp_%s train_step, ResNet-50, %d-shot, 401x401, %d episodes/step (see --mode train)" % (model, shot, batch),
            "episodes_per_step": batch, "steps": steps, "warmup": warmup, "ms_per_step": round(step_ms, 3),
            "episodes_per_s": round(steps * batch / dt, 2), "host_enqueue_ms_per_step": round(host_ms, 2),
            "gflop_per_step": r["gflop_per_step"], "step_effective_tflops": eff,
            "frac": round(eff / PEAK_F32_MFMA_TFLOPS, 4), "kernel_frac": r["frac"],
            "kernel_ms_by_class": {k: v["ms_per_step"] for k, v in r["by_class"].items()},
            "roofline": {"bound": "mfma", "achieved": r["achieved"], "peak": r["peak"], "unit": r["unit"], "frac": r["frac"],
                         "traffic": r.get("traffic"), "algorithmic_bytes_per_launch": r["algorithmic_bytes_per_launch"],
                         "launches_per_step": r["launches_per_step"], "avg_launch_us": r["avg_launch_us"],
                         "pmc_source": r.get("pmc_source")},
            "last_loss": round(float(ls[-1]), 5),
            "note": "frac = conv + weight-gradient flops of a step / timed step / fp32 MFMA peak; kernel_frac = the same flops / "
                    "the summed durations of those kernels in a single-stream pass"}


# ---------------------------------------------------------------------------------------------
# --dump-outputs: what the timed path computed, so that two builds can be compared output for output
# ---------------------------------------------------------------------------------------------
DUMP_LIMIT_BYTES = 60 * 10 ** 6          # array data of one dump; the files stay under 64 MB with their headers


def dump_outputs(outdir, arrays):
    """Write ``arrays`` ({name: tensor or array}) as ``outdir/<name>.npy``: float64 stays float64, every other dtype becomes
    float32 (exact for class indices).  Smallest array first, each one gets at most an equal share of the DUMP_LIMIT_BYTES
    still left; an array larger than its share is replaced by a fixed sample of it: the flattened elements at sorted indices
    drawn without replacement by a generator seeded with 0, the same elements on every run with the same arguments.  A set
    that fits is written whole."""
    os.makedirs(outdir, exist_ok=True)
    out = {}
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        out[name] = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
    left, n = DUMP_LIMIT_BYTES, len(out)
    for name in sorted(out, key=lambda k: out[k].nbytes):
        a = out[name]
        keep = min(a.size, left // n // a.itemsize)
        if keep < a.size:
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, keep, replace=False))]
        np.save(os.path.join(outdir, name + ".npy"), a)
        left, n = left - a.nbytes, n - 1
    print(f"bench.py: wrote {', '.join(f'{k}.npy' for k in out)} to {outdir}", file=sys.stderr)


# ---------------------------------------------------------------------------------------------
# eval
# ---------------------------------------------------------------------------------------------
class EvalRunner:
    """The device work of Evaluator.test_step for ``batch`` resident episodes: hipGraph replay of the shape-static part +
    the fused tail; ``model`` stage2 = stage-1 prior pass + stage 2 (entry/pemp_stage2.py:53-61).  ``loss`` cedt: the
    CELossDT weight map of every ground truth (boundary, exact distance transform; core/losses.py:23-41) is computed on the
    device inside the step and weights the fused tail's cross-entropy."""

    def __init__(self, dev, rank, model="stage1", shot=1, batch=25, dataset="PASCAL", steps=40, graph=True, loss="ce", net=None,
                 pool=None, precision="f32"):
        from pemp_amd import ops
        from pemp_amd.core import losses
        self.graph = graph
        self.ops, self.model, self.shot, self.batch = ops, model, shot, batch
        self.vgg = model in ("baseline", "panet")
        self.net = net if net is not None else build_model(dev, model if self.vgg else "stage1", shot)[0]
        self.stage2 = build_model(dev, "stage2", shot)[0] if model == "stage2" else None
        self.pool = pool if pool is not None else episode_pool(dev, shot, batch, rank, dataset=dataset)
        self.loss = losses.get({"loss": loss, "sigma": 5.0})
        self.precision = precision          # "bf16": the side-figure variant of the encoder (never the headline)
        self.ws, self.ws_align, self.aux_log = {}, {}, []
        self.stats_log = torch.zeros((steps, batch, 8), dtype=torch.float64, device=dev)
        self.cls_log = torch.stack([self.pool[i % len(self.pool)]["cls"] for i in range(steps)])      # [steps, batch]
        self.round = RoundReduce(20 if dataset == "PASCAL" else 80, dev, dataset)
        # Consecutive steps alternate between two engine replicas on their own HIP streams (model.lane(k): same weights, own
        # activation arena, graphs and workspaces): the prototype head + tail of step i (HBM-bound, 0.3 ms) and the gap
        # between two graph replays run beside the first convolutions of step i + 1.  Every step still does all of its work
        # inside the timed region (the closing barrier synchronises the device).
        self.lanes = int(os.environ.get("PEMP_BENCH_LANES", "2")) if model == "stage1" else 1
        self.lane_streams = [torch.cuda.Stream(device=dev) for _ in range(self.lanes)] if self.lanes > 1 else []
        self.lane_ws = [{} for _ in range(self.lanes)]

    def _tail(self, pred, ep, ws):
        wmap = None
        if self.loss.kind == "cedt":
            wmap = self.ops.cedt_weight(ep["qry_mask"], self.loss.sigma, ws_cache=ws)
        return self.ops.eval_tail(pred, ep["qry_mask"], ws_cache=ws, weight=wmap)

    def step(self, i, log=True, graph=None):
        graph = self.graph if graph is None else graph
        if self.lanes > 1 and graph:
            k = i % self.lanes
            ep = self.pool[i % len(self.pool)]
            with torch.cuda.stream(self.lane_streams[k]), self.net.lane(k), self.net.precision(self.precision), torch.no_grad():
                pred, _ = self.net.lowres_graphed(ep["sup_img"], ep["sup_mask"], ep["qry_img"])
                am, stats, _ = self._tail(pred, ep, self.lane_ws[k])
                if log:
                    self.stats_log[i].copy_(stats)
            return am
        ops, net, stage2 = self.ops, self.net, self.stage2
        ep = self.pool[i % len(self.pool)]
        ins = (ep["sup_img"], ep["sup_mask"], ep["qry_img"])
        with net.precision(self.precision), torch.no_grad():
            pred, _ = net.lowres_graphed(*ins) if graph else net.lowres(*ins)
            if stage2 is not None:
                prior, _, _ = ops.eval_tail(pred, None, out_hw=ins[0].shape[-2:], ws_cache=self.ws)
                prior = prior.unsqueeze(1).float()
                pred, _ = stage2.lowres_graphed(*ins, prior) if graph else stage2.lowres(*ins, prior)
            if self.model == "panet":       # auxiliary prototype-alignment loss of every episode (entry/panet.py:51-57)
                from pemp_amd.networks.panet import align_forward
                self.aux_log.append(align_forward(net._last_feats, pred, ins[1], ins[0].shape[0], self.shot, 1, 20, self.ws_align)["loss"])
            am, stats, _ = self._tail(pred, ep, self.ws)
        if log:
            self.stats_log[i].copy_(stats)
        return am

    def timed(self, steps, warmup, world, dev):
        """-> (seconds [MAX over ranks], mean CE loss, this rank's own seconds).  The round's metric aggregation -- statistics
        rows -> class table -> ONE all-reduce over the ranks -- happens inside the timed region, once per K steps (the
        reference aggregates per round, core/base_trainer.py:84-100)."""
        def prime():                    # setup, not a step: every lane records its hipGraph (and rank 0 times kernel variants)
            for k in range(max(self.lanes, 1)):
                self.step(k, log=False)
            torch.cuda.synchronize()
        if world == 1:
            prime()
        if world > 1:                   # kernel variants are timed by rank 0 only and broadcast
            self.ops.tuned_by_rank0(prime)
            beat()
        # the aggregation's own kernels (a dozen small ATen launches) are loaded once here, not inside the timed region; the
        # collective itself first runs in the timed region (every rank would have to take part in a rehearsal).  BEFORE the
        # warm-up steps, not behind them: their first use is 30 ms of code loading on the host with the GPU idle, and a
        # GPU that has idled that long starts the timed region below its steady clocks (round 4's driver line lost 0.4 ms
        # per step that way: 25.84 ms against 25.34 ms of convolutions measured later in the same process)
        self.round.table.reset()
        self.round.table.add(self.stats_log[:steps].view(-1, 8), self.cls_log[:steps].reshape(-1))
        self.round.table.pack.clone()
        torch.cuda.synchronize()
        for i in range(warmup):
            self.step(i, log=False)
            beat()

        def barrier():
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()

        cur = torch.cuda.current_stream()
        e_start, e_steps = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        barrier()
        t0 = time.perf_counter()
        e_start.record()
        for st in self.lane_streams:
            st.wait_stream(cur)
        dbg_ev = []
        for i in range(steps):
            am = self.step(i)
            if os.environ.get("PEMP_BENCH_DEBUG") and self.lane_streams:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(self.lane_streams[i % self.lanes])
                dbg_ev.append(ev)
        for st in self.lane_streams:    # the lanes' last steps have logged their rows before the table is built
            cur.wait_stream(st)
        e_steps.record()                # this rank's own steps are done here; the collective below couples the ranks
        t_enq = time.perf_counter() - t0
        self.round.reduce(self.stats_log[:steps].view(-1, 8), self.cls_log[:steps].reshape(-1))
        t_red = time.perf_counter() - t0
        barrier()
        dt = time.perf_counter() - t0
        if os.environ.get("PEMP_BENCH_DEBUG"):
            print(f"[timed] host: steps enqueued after {t_enq * 1e3:.2f} ms, reduce enqueued after {t_red * 1e3:.2f} ms, "
                  f"device idle after {dt * 1e3:.2f} ms; device span of the steps {e_start.elapsed_time(e_steps):.2f} ms", file=sys.stderr)
            if dbg_ev:
                ends = [e_start.elapsed_time(ev) for ev in dbg_ev]
                print("[timed] step completion deltas (ms): " + " ".join(f"{b - a:.2f}" for a, b in zip([0.0] + ends[:-1], ends)), file=sys.stderr)
        local_dt = e_start.elapsed_time(e_steps) * 1e-3
        beat()
        self.last_outputs = {"qry_pred": am, "stats": self.stats_log[steps - 1]}        # what the last timed step returned
        if self.aux_log:
            self.last_outputs["align_loss"] = self.aux_log[-1]
        if world > 1:
            tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dt = float(tmax.item())
        # sanity on the logged statistics (the work really happened): finite losses, counts add up
        st = self.stats_log[:steps].cpu().numpy()
        assert np.isfinite(st).all() and (st[..., 1] > 0).all(), "eval tail produced invalid statistics"
        return dt, float((st[..., 0] / st[..., 1]).mean()), local_dt

    def comm(self, steps, world, local_dt, dev):
        """A collective (every rank calls it, right after ``timed``): -> (`comm` object, `miou` object of the reduced table)."""
        rank_ms = gather_rank_ms(local_dt, steps, world, dev)
        same, miou = self.round.verify(world)
        if not same:
            raise AssertionError("the all-reduced metric table is not the sum of the rank shards")
        return comm_object(world, rank_ms, collective="all_reduce(SUM) of the round's [C+1, 3] tp/fp/fn table + loss sum + episode "
                                                      "count, once per K steps, inside the timed region",
                           collectives_in_timed_region=1 if world > 1 else 0, allreduce_bytes_per_round=self.round.nbytes,
                           allreduce_ms=round(self.round.allreduce_ms(), 4), table_equals_sum_of_rank_shards=same), miou


def side_stage2(dev, shot=5, batch=8, steps=8, warmup=3):
    """BASELINE.json configs[3] inside the default run: stage-1 prior + stage 2, 5-shot, 8 episodes per step."""
    run = EvalRunner(dev, 0, "stage2", shot, batch, steps=steps)
    dt, mean_loss, _ = run.timed(steps, warmup, 1, dev)
    step_ms = dt / steps * 1e3
    rec = instrumented(lambda r: run.step(r, log=False, graph=False), reps=1)
    r = summarize(rec, 1, step_ms)
    return {"workload": "pemp_stage1 prior + pemp_stage2 eval test_step, ResNet-50, %d-shot, 401x401, %d episodes/step" % (shot, batch),
            "episodes_per_step": batch, "steps": steps, "warmup": warmup, "ms_per_step": round(step_ms, 3),
            "episodes_per_s": round(steps * batch / dt, 2), "gflop_per_step": r["gflop_per_step"],
            "step_effective_tflops": r.get("step_effective_tflops"),
            "frac": round(r.get("step_effective_tflops", 0.0) / PEAK_F32_MFMA_TFLOPS, 4), "kernel_frac": r["frac"],
            "mean_ce_loss": round(mean_loss, 6)}


def side_eval(dev, model, dataset, batch, steps=8, warmup=3, net=None, what=""):
    """Another BASELINE.json evaluation configuration inside the default run, under the driver's clock: the same timed loop as
    the headline (EvalRunner.timed) and a live roofline pass of its own."""
    run = EvalRunner(dev, 0, model, 1, batch, dataset, steps=steps, net=net)
    dt, mean_loss, _ = run.timed(steps, warmup, 1, dev)
    step_ms = dt / steps * 1e3
    rec = instrumented(lambda r: run.step(r, log=False, graph=False), reps=1)
    r = summarize(rec, 1, step_ms)
    return {"workload": what, "episodes_per_step": batch, "steps": steps, "warmup": warmup, "ms_per_step": round(step_ms, 3),
            "episodes_per_s": round(steps * batch / dt, 2), "gflop_per_step": r["gflop_per_step"],
            "step_effective_tflops": r.get("step_effective_tflops"),
            "frac": round(r.get("step_effective_tflops", 0.0) / PEAK_F32_MFMA_TFLOPS, 4), "kernel_frac": r["frac"],
            "avg_launch_us": r.get("avg_launch_us"), "launches_per_step": r.get("launches_per_step"),
            "mean_ce_loss": round(mean_loss, 6)}


def miou_vs_cpu(net, dev, cpu):
    """mIoU of the episodes the CPU baseline leg evaluated (the reference prints mIoU and speed together,
    core/base_trainer.py:84-100): the same E(seed) episodes through Evaluator.test_step_device, the tp/fp/fn rows through
    FewShotMetric on both sides."""
    from pemp_amd import synth
    from pemp_amd.core.metrics import FewShotMetric
    from pemp_amd.entry.pemp_stage1 import Evaluator
    eps = cpu.get("episodes") or []
    if not eps:
        return {"error": "the CPU leg returned no per-episode rows"}
    ev = Evaluator(net, device=dev)
    labels = synth.val_labels(0, eps[0].get("dataset", "PASCAL"))
    nclass = 20 if eps[0].get("dataset", "PASCAL") == "PASCAL" else 80
    m_gpu, m_cpu = FewShotMetric(nclass), FewShotMetric(nclass)
    dloss, same = 0.0, 0
    t = lambda a: torch.from_numpy(a)[None]
    for e in eps:
        ep = synth.make_episode(e["seed"], shot=e["shot"], index=e["index"], dataset=e.get("dataset", "PASCAL"))
        _, stats = ev.test_step_device((t(ep["sup_img"]), t(ep["sup_mask"]), t(ep["qry_img"])), t(ep["qry_mask"]))
        st = stats.cpu().numpy()
        m_gpu.update_counts(st[:, 2:], [e["cls"]])
        m_cpu.update_counts(np.asarray(e["counts"], np.float64)[None], [e["cls"]])
        dloss = max(dloss, abs(float(st[0, 0] / st[0, 1]) - e["loss"]))
        same += int(np.array_equal(st[0, 2:], np.asarray(e["counts"], np.float64)))
    seen = [c for c in labels if m_cpu.stat[c].sum() > 0]
    mg, mc = float(m_gpu.mIoU(seen)[1]), float(m_cpu.mIoU(seen)[1])
    bg, bc = float(m_gpu.mIoU(seen, binary=True)[1]), float(m_cpu.mIoU(seen, binary=True)[1])
    return {"miou": round(mg, 6), "miou_cpu": round(mc, 6), "delta_miou_vs_cpu": round(abs(mg - mc), 8),
            "biou": round(bg, 6), "delta_biou_vs_cpu": round(abs(bg - bc), 8), "episodes": len(eps), "classes": len(seen),
            "episodes_with_identical_pixel_counts": same, "max_abs_delta_ce_loss": round(dloss, 8),
            "note": "synthetic E(seed) episodes + Wgen weights: the value says nothing about PASCAL accuracy, the delta is the parity figure"}


def main():
    args = parse()
    if args.cpu_leg:
        return cpu_leg(args)
    if args.mode == "train" and "--batch" not in sys.argv:           # the reference trains with data.bs = 4
        args.batch = 4
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:              # no launcher around us: be the launcher
        raise SystemExit(launch_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    # the training engines seed their DropBlock / Dropout2d Philox stream from torch.initial_seed(): one fixed seed per rank,
    # so that the same arguments give the same inputs on every run (episodes and weights are seeded already)
    torch.manual_seed(rank)
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and rank == 0:
        print(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s); reporting n_gpus = {world}", file=sys.stderr)
    if world > 1:
        # N ranks share this host's cores (episode synthesis in numpy / torch-CPU, the eager enqueue loop): cores / N threads
        # each, set before any GPU call (torchrun's own default would be OMP_NUM_THREADS = 1)
        torch.set_num_threads(host_threads_per_rank(int(os.environ.get("LOCAL_WORLD_SIZE", world))))
    if os.environ.get("PEMP_BENCH_DRYRUN"):
        return dry_run(args, world, rank)
    beat()
    if os.environ.get("PEMP_BENCH_STUB"):          # tests: main_train's real control flow on CPU tensors over gloo
        if args.mode != "train":
            raise SystemExit("PEMP_BENCH_STUB drives --mode train only")
        if world > 1:
            dist.init_process_group("gloo")
            dist.barrier()
        return main_train(args, world, rank, torch.device("cpu"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    # PEMP_BENCH_BACKEND=gloo: rehearsal of the N > 1 control flow on a box with fewer GPUs than ranks (ranks share
    # devices round-robin; the numbers mean nothing then).  The driver's runs use the default: one GPU per rank, RCCL.
    backend = os.environ.get("PEMP_BENCH_BACKEND", "nccl")
    first_local = local == 0
    if backend != "nccl":
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    from pemp_amd import build
    if first_local:
        build.build()                 # normally a no-op: the prebuilt .so travels with the snapshot
    if world > 1:
        dist.barrier()
    beat()
    if args.mode == "train":
        return main_train(args, world, rank, dev)
    vgg = args.model in ("baseline", "panet")
    run = EvalRunner(dev, rank, args.model, args.shot, args.batch, args.dataset, args.steps, graph=not args.no_graph, loss=args.loss)
    net, pool = run.net, run.pool
    beat()
    dt, mean_loss, local_dt = run.timed(args.steps, args.warmup, world, dev)
    comm, round_miou = run.comm(args.steps, world, local_dt, dev)
    if world > 1:
        # the process group ends HERE: everything rank 0 measures below is rank-local, and the other ranks leave instead of
        # spinning in a barrier kernel on their GPUs while it does
        dist.barrier()
        dist.destroy_process_group()
    if rank != 0:
        return
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, run.last_outputs)

    eps_total = args.steps * args.batch * world
    name = "Baseline" if args.model == "baseline" else "PANet" if args.model == "panet" else \
        "PEMP stage-1" if run.stage2 is None else "PEMP stage-1 prior + stage-2"
    dsn = "PASCAL-5i" if args.dataset == "PASCAL" else "COCO-20i"
    step_ms = dt / args.steps * 1e3
    out = {
        "metric": "episodes/sec (%s eval step, %s-shaped %d-shot, %s)" % (name, dsn, args.shot, "VGG-16" if vgg else "ResNet-50"),
        "value": round(eps_total / dt, 2), "unit": "episodes/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(step_ms, 4), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "%s eval test_step, %s, %d-shot, 401x401, %d episode(s)/step, %s-shaped "
                               "synthetic E(seed) episodes + Wgen(1234) weights; episodes resident in HBM when the timed "
                               "region starts; the round's metric table is built and all-reduced inside the timed region and "
                               "fetched once after it (the reference's Timer region also holds the "
                               "three H2D copies and the argmax/loss D2H of every episode: that figure is `end_to_end` and "
                               "`single_episode.reference_body`)" % (
                                   args.model if vgg else "pemp_" + args.model, "VGG-16" if vgg else "ResNet-50",
                                   args.shot, args.batch, dsn),
                   "episodes_per_step": args.batch, "shot": args.shot, "loss": args.loss, "hipgraph": not args.no_graph,
                   "engine_lanes": run.lanes if not args.no_graph else 1,
                   "dataset": args.dataset, "mean_ce_loss": round(mean_loss, 6)},
        "comm": comm,
    }
    if world > 1:
        out["miou"] = round_miou      # N = 1: `round_miou` holds this table; --full adds `miou` against the CPU oracle
    else:
        out["round_miou"] = round_miou
    if not args.full:               # a plain run ends with the headline
        print(json.dumps(out))
        return

    # the auxiliary measurements must never cost the headline line: a failure is reported in place
    def guarded(key, fn):
        try:
            out[key] = fn()
        except Exception as exc:  # noqa: BLE001
            out[key] = {"error": f"{type(exc).__name__}: {exc}"}
        beat()

    if not args.no_roofline:
        def roof():
            rec = instrumented(lambda r: run.step(r, log=False, graph=False), reps=3)
            r = summarize(rec, 3, step_ms)
            r["cosine_kernel"] = cosine_roofline(net, pool)
            return attach_pmc(r, f"{args.model}-eval-b{args.batch}-s{args.shot}")
        guarded("roofline", roof)
    headline = world == 1 and args.model == "stage1" and not args.no_graph and args.loss == "ce"
    if headline and not args.no_single:
        guarded("single_episode", lambda: single_episode(net, dev, args))
    if headline and not args.no_e2e and args.dataset == "PASCAL":
        guarded("end_to_end", lambda: end_to_end(net, args, dev))
    if world == 1 and args.cpu_episodes > 0 and args.model != "panet":
        if args.model == "baseline":
            args.cpu_episodes = 4                # BASELINE.json configs[0]: exactly four test episodes
        guarded("cpu_baseline", lambda: cpu_baseline(args))
        if args.model == "stage1" and isinstance(out["cpu_baseline"], dict) and "episodes" in out["cpu_baseline"]:
            rows = {"episodes": out["cpu_baseline"].pop("episodes")}
            guarded("miou", lambda: miou_vs_cpu(net, dev, rows))
        elif isinstance(out.get("cpu_baseline"), dict):
            out["cpu_baseline"].pop("episodes", None)          # per-episode rows: only the stage-1 line compares them (`miou`)
    # the other BASELINE.json configurations, measured in this process so that they sit under the driver's clock too
    if headline and args.dataset == "COCO" and args.shot == 1 and args.bf16_side:
        guarded("bf16_variant", lambda: bf16_variant(run, dev, args))       # the COCO-shaped round's delta mIoU
    if headline and args.dataset == "PASCAL" and args.shot == 1 and not args.no_sides:
        guarded("protocol_5x1000", lambda: protocol_5x1000(net, pool, dev, args))
        if args.bf16_side:              # not in the default line any more (round 4's verdict: a narrower arithmetic earns nothing)
            guarded("bf16_variant", lambda: bf16_variant(run, dev, args))
        cedt = {}
        try:
            cedt["eval"] = side_cedt_eval(run, dev, args)
        except Exception as exc:  # noqa: BLE001
            cedt["eval"] = {"error": f"{type(exc).__name__}: {exc}"}
        del run
        keep = {}
        guarded("train", lambda: side_train(dev, keep=keep))
        try:
            cedt["train"] = side_cedt_train(keep, dev) if keep else {"error": "the `train` object failed"}
        except Exception as exc:  # noqa: BLE001
            cedt["train"] = {"error": f"{type(exc).__name__}: {exc}"}
        keep.clear()
        out["cedt"] = cedt
        guarded("stage2_5shot", lambda: side_stage2(dev))
        # BASELINE.json configs[4] and configs[0]: every configuration has a driver-timed figure with its own roofline fraction
        guarded("coco", lambda: side_eval(dev, "stage1", "COCO", 25, net=net,
                                          what="pemp_stage1 eval test_step, ResNet-50, 1-shot, COCO-20i-shaped episodes (80 classes, "
                                               "ground truth up to 640x640), 25 episodes/step"))
        guarded("baseline_vgg16", lambda: side_eval(dev, "baseline", "PASCAL", 12,
                                                    what="baseline eval test_step, VGG-16, 1-shot, 401x401, 12 episodes/step"))
        if isinstance(out.get("baseline_vgg16"), dict) and "error" not in out["baseline_vgg16"] and args.cpu_episodes > 0:
            # configs[0] names its own CPU figure: "VGG-16, 4 test episodes on CPU" -- the oracle's baseline_forward on seeds 5678..5681
            try:
                cb = cpu_baseline(argparse.Namespace(mode="eval", model="baseline", shot=1, batch=1, dataset="PASCAL", cpu_episodes=4))
                cb.pop("episodes", None)
                out["baseline_vgg16"]["cpu_baseline"] = cb
            except Exception as exc:  # noqa: BLE001
                out["baseline_vgg16"]["cpu_baseline"] = {"error": f"{type(exc).__name__}: {exc}"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
