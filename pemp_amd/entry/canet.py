"""CANet evaluation harness on MI355X (counterpart of the reference's entry/canet.py: config :29-40, ``Evaluator`` :45-103,
``test`` :178-196) with the iterative refinement loop kept on the device.

The reference keeps, per query image, the softmax of its last prediction (``history_mask_list[cls][index]``,
data_kits/pascal_voc.py:324,420-429) and feeds it to the next episode of the round that meets the same query
(entry/canet.py:72-80).  Here the softmaxes live in a device-resident table [slots,2,h,w]; the host keeps only the
``key -> slot`` integers.  Two rules make the result independent of batching and of the number of ranks:

* **group closing** (``close_groups``): a step's group of episodes is closed early when the next episode's key is already in
  the group, so inside a step no episode needs the result of another and every episode reads exactly what the
  one-episode-per-step protocol would have left for it;
* **rank assignment** (``assign_ranks``): episodes go to ranks by history key, all episodes of a key on one rank in round
  order, not as ``tasks[rank::world]``.

The table is cleared (all keys forgotten) at every ``sample_tasks()``.

``train_head`` trains the head behind the frozen trunk (``pemp_amd.train_canet``; the reference's ``freeze_backbone = True``
procedure, entry/canet.py:106-175) with the same kind of table: a training episode reads the row of its key -- dropped with
probability 0.3, as the reference's loader drops a stored history (data_kits/pascal_voc.py:316,426) -- and the step writes its
softmax back.  ``train`` (the reference's command name) still raises: a ``train()``-mode autograd forward is not ported."""
import time

import numpy as np
import torch
import torch.distributed as dist

from .. import ops, synth
from ..config import Experiment
from ..core.metrics import Accumulator, FewShotMetric
from ..networks.canet import WGEN_SEED, ModelClass, net_ingredient  # noqa: F401
from ..train_canet import CANetTrainer
from .pemp_stage1 import INGREDIENTS, DeviceRoundTable, SyntheticEpisodes, get_val_labels, num_classes  # noqa: F401
from .pemp_stage1 import Evaluator as _Evaluator

NAME = "PEMP"
ex = Experiment(name=NAME, ingredients=[net_ingredient] + INGREDIENTS[1:])      # CANet's own net ingredient; data, tr, te, g, d


@ex.config
def ex_config():
    tag = "canet"               # str, configuration tag
    shot = 1                    # int, support samples per episode
    query = 1                   # int, query samples per episode
    split = -1                  # int, split number [0, 1, 2, 3], required
    seed = 1234                 # int, random seed
    ckpt = "bestckpt.pth"       # str, checkpoint file
    exp_id = -1                 # experiment id to load checkpoint
    loss = "ce"                 # str, loss type [ce/cedt]
    sigma = 5.                  # float, sigma of the DT loss
    trunk_precision = "f32_chain"   # str, frozen-trunk convs of train_head [f32_chain/split3]; test / train ignore it


def close_groups(keys, batch):
    """Episode indices 0..len(keys)-1 in order, cut into steps: a group takes at most ``batch`` episodes and is closed early
    when the next episode's key is already in it.  -> list of lists."""
    groups, cur, seen = [], [], set()
    for i, k in enumerate(keys):
        if cur and (len(cur) >= batch or k in seen):
            groups.append(cur)
            cur, seen = [], set()
        cur.append(i)
        seen.add(k)
    if cur:
        groups.append(cur)
    return groups


def assign_ranks(keys, world):
    """-> per rank the episode indices it evaluates: the j-th distinct key of the round (in order of first appearance) goes to
    rank j % world with all its episodes, round order kept.  Pure function of the key sequence."""
    rank_of, out = {}, [[] for _ in range(world)]
    for i, k in enumerate(keys):
        r = rank_of.setdefault(k, len(rank_of) % world)
        out[r].append(i)
    return out


class SyntheticHistoryEpisodes(SyntheticEpisodes):
    """``SyntheticEpisodes`` whose query image and label are a function of the episode's history key and whose keys repeat
    within a round: every class has a pool of ``pool`` queries, episode ``i`` draws one of them (a function of its seed), so a
    1000-episode round over 5 x 60 queries meets most of them several times, as PASCAL-5i val does.  The supports are those
    of ``E(seed)``."""

    def __init__(self, test_n, test_seed, shot, split=0, height=401, width=401, dataset="PASCAL", pool=60):
        super().__init__(test_n, test_seed, shot, split, height, width, dataset)
        self.pool = int(pool)

    def _seed(self, i):
        return self.test_seed + self.round * self.test_n + i

    def history_key(self, i):
        seed = self._seed(i)
        labels = synth.val_labels(max(self.split, 0), self.dataset)
        return int(labels[seed % len(labels)]), int(synth.uniform01(seed, "qpool", 1)[0] * self.pool)

    def task(self, i):
        seed = self._seed(i)
        cls, qi = self.history_key(i)
        ep = synth.make_episode(seed, self.shot, self.height, self.width, index=i, split=self.split, dataset=self.dataset)
        qep = synth.make_episode(1_000_003 * cls + qi, 1, self.height, self.width, index=qi, split=self.split, dataset=self.dataset)
        t = lambda a: torch.from_numpy(a)[None]
        return (t(ep["sup_img"]), t(ep["sup_mask"]), t(qep["qry_img"])), t(qep["qry_mask"]), torch.tensor([cls])


def eval_episodes(dcfg, shot, split):
    """PASCAL-5i from ``data.base_dir`` in the reference's "test_canet" mode, synthetic repeating-key episodes otherwise."""
    if dcfg.get("base_dir"):
        from ..data_kits.pascal_voc import load
        return load(dcfg, "test_canet", split, shot)[0]
    return SyntheticHistoryEpisodes(dcfg["test_n"], dcfg["test_seed"], shot, split, dcfg["height"], dcfg["width"], dcfg["dataset"])


class Evaluator(_Evaluator):
    """The stage-1 evaluator (fused tail, device-side round table, hipGraph replay) with CANet's history loop (module
    docstring).  ``start_eval_loop`` needs a dataset with ``history_key(i)``."""

    def __init__(self, model, device=None, use_graph=True, splitk=None):
        super().__init__(model, device=device, use_graph=use_graph, lanes=1, splitk=splitk)
        self.table, self.slot_of = None, {}

    def _lowres(self, dev_in):
        """A step outside a round (``test_step``): zero history."""
        sup_img, sup_mask, qry_img = dev_in
        self.model.check_inputs(sup_img, qry_img)
        return super()._lowres(dev_in)

    def reset_history(self, capacity, H, W):
        """Forget every key (the reference re-creates ``history_mask_list`` in ``sample_tasks``); the table is allocated once
        per capacity and feature size, so captured graphs keep addressing it.  Rows need no clearing: a key's first episode
        reads slot -1 (zeros)."""
        h, w = self.model.feature_hw(H, W)
        if self.table is None or self.table.shape[0] < capacity or tuple(self.table.shape[-2:]) != (h, w):
            self.table = torch.zeros((max(int(capacity), 1), 2, h, w), dtype=torch.float32, device=self.device)
        self.slot_of = {}

    def test_step_history(self, episodes, keys):
        """``episodes``: list of (inputs, qry_msk), one episode each, with pairwise different ``keys``.  One forward for all of
        them: episode b reads the table row of its key (none yet: zeros) and overwrites it with its softmax.  -> stats f64
        [len(episodes), 8] on the GPU; no host synchronisation."""
        if len(set(keys)) != len(keys):
            raise ValueError("a step must not hold one history key twice (close_groups cuts the round accordingly)")
        read = [self.slot_of.get(k, -1) for k in keys]
        write = [self.slot_of.setdefault(k, len(self.slot_of)) for k in keys]
        if max(write) >= self.table.shape[0]:
            raise ValueError("the history table is too small for this round: call reset_history with the round's key count")
        dev_in = [torch.cat([ep[0][k].to(self.device, non_blocking=True) for ep in episodes]) for k in range(3)]
        labels = [ep[1].view(-1, *ep[1].shape[-2:]) for ep in episodes]
        rs = torch.tensor(read, dtype=torch.int32).to(self.device, non_blocking=True)
        ws = torch.tensor(write, dtype=torch.int32).to(self.device, non_blocking=True)
        with torch.no_grad(), ops.eval_splitk(ops.EVAL_SPLITK if self.splitk is None else self.splitk):
            fn = self.model.lowres_graphed_slots if self.use_graph else self.model.lowres_slots
            return ops.tail_rows(fn(*dev_in, self.table, rs, ws), labels, ws_cache=self._ws)

    def eval_round(self, dataset, batch=1, rank=0, world=1):
        """One round after ``dataset.sample_tasks()``: -> (stats rows [n,8] on the GPU in this rank's episode order, classes)."""
        keys = [dataset.history_key(i) for i in range(len(dataset))]
        mine = assign_ranks(keys, world)[rank]
        my_keys = [keys[i] for i in mine]
        self.reset_history(len(set(my_keys)), dataset.height, dataset.width)
        episodes = self._episodes(dataset, mine)
        rows, classes = [], []
        for group in close_groups(my_keys, batch):
            eps = []
            for _ in group:
                inputs, qry_msk, cls = next(episodes)
                eps.append((inputs, qry_msk))
                classes += [int(c) for c in cls]
            rows.append(self.test_step_history(eps, [my_keys[j] for j in group]))
        empty = torch.empty((0, 8), dtype=torch.float64, device=self.device)
        return (torch.cat(rows) if rows else empty), classes

    def start_eval_loop(self, dataset, num_classes, split, te_epochs=5, logger=None, batch=1, dataset_name="PASCAL"):
        """The reference loop (entry/canet.py:55-103), sharded over ranks by history key; one fetch per round."""
        self.model.eval()
        dataset.reset_sampler()
        world = dist.get_world_size() if dist.is_initialized() else 1
        rank = dist.get_rank() if dist.is_initialized() else 0
        accum = Accumulator(loss=[], miou=[], biou=[])
        val_labels = get_val_labels(split, dataset_name)
        table = DeviceRoundTable(num_classes, self.device)
        timed, calls = 0.0, 0
        for epoch in range(1, te_epochs + 1):
            metric = FewShotMetric(num_classes)
            dataset.sample_tasks()
            t0 = time.time()
            rows, classes = self.eval_round(dataset, batch, rank, world)
            table.reset()
            if len(classes):
                table.add(rows, torch.tensor(classes, dtype=torch.int64, device=self.device))
            table.allreduce()
            metric.stat, loss_tot, n_tot = table.fetch()
            timed += time.time() - t0
            calls += len(classes)
            miou_c, miou = metric.mIoU(val_labels)
            biou_c, biou = metric.mIoU(val_labels, binary=True)
            if logger is not None and rank == 0:
                logger.info(f"[round {epoch}/{te_epochs}] mIoU: {miou * 100:5.2f}  |  bIoU: {biou * 100:5.2f}")
            accum.update(loss=loss_tot / max(n_tot, 1.0), miou=miou_c, biou=biou_c)
        self.cps = calls / timed if timed > 0 else 0.0
        self.round_miou, self.round_biou = np.array(accum.values["miou"]), np.array(accum.values["biou"])
        return accum.mean(["loss", "miou", "biou"])


@ex.command
def test(_config, split, shot, query, exp_id, ckpt):
    import logging
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    logger = logging.getLogger(NAME)
    if split < 0:
        raise ValueError("Argument `split` is required! For example: `python -m pemp_amd.entry.canet test with split=0`")
    if query != 1:
        raise ValueError("CANet takes exactly one query per episode here (query=1)")
    from ..core.snapshots import load_for_eval
    model = ModelClass(logger)
    load_for_eval(model, _config, exp_id, ckpt, logger, wgen_seed=WGEN_SEED)
    model = model.cuda().eval()
    ev = Evaluator(model)
    d = _config["data"]
    data = eval_episodes(d, shot, split)
    loss, miou, biou = ev.start_eval_loop(data, num_classes(d["dataset"]), split, _config["te"]["epochs"], logger,
                                          batch=d["test_bs"], dataset_name=d["dataset"])
    return f"Loss: {loss:.4f}, mIoU: {np.mean(miou) * 100:.2f}, bIoU: {np.mean(biou) * 100:.2f}"


class SyntheticHistoryTrainEpisodes(SyntheticHistoryEpisodes):
    """``SyntheticHistoryEpisodes`` in the training role: the query label comes at the input size (the reference resizes a
    training label with its image, data_kits/pascal_voc.py:401-406)."""

    def task(self, i):
        seed = self._seed(i)
        cls, qi = self.history_key(i)
        hw = (self.height, self.width)
        ep = synth.make_episode(seed, self.shot, self.height, self.width, index=i, split=self.split, dataset=self.dataset)
        qep = synth.make_episode(1_000_003 * cls + qi, 1, self.height, self.width, index=qi, out_hw=hw, split=self.split,
                                 dataset=self.dataset)
        t = lambda a: torch.from_numpy(a)[None]
        return (t(ep["sup_img"]), t(ep["sup_mask"]), t(qep["qry_img"])), t(qep["qry_mask"]), torch.tensor([cls])


class HistorySlots:
    """Host side of the training history: ``key -> table row`` and the reference's history drop.  ``slots(keys)`` names, for
    one batch, the row each episode reads (-1: zeros -- no stored history yet, or a stored one dropped: one draw of a
    ``RandomState(9876)`` per episode that HAS a stored history, in batch order, ``<= 0.3`` drops it; data_kits/pascal_voc.py:
    316,422-427) and the row its softmax goes to (a key twice in a batch: the last episode's stays, as the reference's
    sequential write-back leaves it; the others write nowhere).  The sampler lives as long as the object (the reference seeds
    it in ``reset_sampler``, once); ``clear()`` forgets the keys (``sample_tasks``, every epoch)."""
    DROP = 0.3

    def __init__(self):
        self.sampler = np.random.RandomState(9876)
        self.slot_of = {}

    def clear(self):
        self.slot_of = {}

    def slots(self, keys):
        read = []
        for k in keys:
            s = self.slot_of.get(k, -1)
            if s >= 0 and self.sampler.random_sample() <= self.DROP:
                s = -1
            read.append(s)
        rows = [self.slot_of.setdefault(k, len(self.slot_of)) for k in keys]
        last = {k: j for j, k in enumerate(keys)}
        return read, [r if last[k] == j else -1 for j, (k, r) in enumerate(zip(keys, rows))]


class HeadTrainer(CANetTrainer):
    """``train_step(sup_img, sup_mask, qry_img, keys, qry_msk=...)`` of the reference's CANet Trainer (entry/canet.py:107-116,
    130-140) -> (loss, softmax): ``CANetTrainer`` with the history in a device table addressed by ``HistorySlots``."""

    def __init__(self, model, **kw):
        super().__init__(model, **kw)
        self.history, self.table = HistorySlots(), None

    def start_epoch(self, capacity, H, W):
        """Forget every key; the table is allocated once per capacity and feature size (rows need no clearing: a key's first
        episode reads slot -1)."""
        h, w = self.model.feature_hw(H, W)
        if self.table is None or self.table.shape[0] < capacity or tuple(self.table.shape[-2:]) != (h, w):
            self.table = torch.zeros((max(int(capacity), 1), 2, h, w), dtype=torch.float32, device=self.device)
        self.history.clear()

    def train_step(self, sup_img, sup_mask, qry_img, keys, qry_msk=None):
        qry_msk = qry_msk.view(-1, *qry_msk.shape[-2:])
        if not self.model.use_history:
            return super().train_step(sup_img, sup_mask, qry_img, qry_msk=qry_msk)
        if self.table is None:
            self.start_epoch(len(keys), *sup_img.shape[-2:])
        read, write = self.history.slots(list(keys))
        if max(write) >= self.table.shape[0]:
            raise ValueError("the history table is too small for this epoch: call start_epoch with its key count")
        rs = torch.tensor(read, dtype=torch.int32).to(self.device, non_blocking=True)
        ws = torch.tensor(write, dtype=torch.int32).to(self.device, non_blocking=True)
        return super().train_step(sup_img, sup_mask, qry_img, qry_msk=qry_msk, table=self.table, read_slot=rs, write_slot=ws)


def head_train_batches(trainer, dcfg, shot, split, rank, steps_per_epoch, device):
    """-> ``batches(epoch)`` for ``TrainingLoop``: ``((sup_img, sup_mask, qry_img, history keys), qry_msk)`` per step, from
    synthetic repeating-key episodes; every epoch samples anew and clears the trainer's history."""
    bs = dcfg["bs"]
    data = SyntheticHistoryTrainEpisodes(steps_per_epoch * bs, dcfg["seed"] + 7919 * rank, shot, split, dcfg["height"], dcfg["width"],
                                         dcfg["dataset"])

    def batches(epoch):
        data.sample_tasks()
        keys = [data.history_key(i) for i in range(len(data))]
        trainer.start_epoch(len(set(keys)), data.height, data.width)
        for s in range(steps_per_epoch):
            eps = [data.task(i) for i in range(s * bs, (s + 1) * bs)]
            inputs = tuple(torch.cat([e[0][k] for e in eps]) for k in range(3))
            yield inputs + (keys[s * bs:(s + 1) * bs],), torch.cat([e[1] for e in eps])
    return batches


@ex.command
def train_head(_config, split, shot, query, seed, loss, sigma, exp_id, ckpt, trunk_precision):
    """``python -m pemp_amd.entry.canet train_head with split=0 [shot=5] [trunk_precision=split3]``: CANet's training procedure (entry/canet.py:106-175)
    for the reference's frozen trunk -- the head trains on the HIP path, per-epoch evaluation with the history loop,
    ``ckpt.pth`` / ``bestckpt.pth`` (reference-loadable state_dicts) under ``<g.model_dir>/<tag>/<id>``."""
    from .pemp_stage1 import run_training
    if query != 1:
        raise ValueError("CANet takes exactly one query per episode here (query=1)")
    if _config["data"].get("base_dir"):
        raise ValueError("train_head reads synthetic episodes only: the PASCAL-5i loader (data_kits.pascal_voc.load) has no training "
                         "mode that names the query's history key; leave data.base_dir empty")

    def make_trainer(logger, dev):
        from ..core.snapshots import load_for_eval
        model = ModelClass(logger)
        load_for_eval(model, _config, exp_id, ckpt, logger, wgen_seed=WGEN_SEED)     # the frozen trunk comes from a checkpoint
        return HeadTrainer(model, lr=_config["tr"]["lr"], device=dev, loss=loss, sigma=sigma, trunk_precision=trunk_precision)

    return run_training(_config, NAME, make_trainer, lambda tr, dev: Evaluator(tr.model, device=dev), split, shot, seed, exp_id,
                        val_episodes=eval_episodes, batches=head_train_batches)


@ex.command
def train(_config):
    raise NotImplementedError("CANet is an inference path here: `test` runs it; training (entry/canet.py:106-175) is not ported")


if __name__ == "__main__":
    print(ex.run_commandline())
