"""RPMMs evaluation harness on MI355X (counterpart of the reference's entry/rpmms.py: its configuration, ``Evaluator.test_step``
-> (qry_pred, loss, loss_p1, loss_p2), ``test``).  The stage-1 evaluator (batching, sharding, hipGraph replay, fused upsample +
CE + argmax + tp/fp/fn tail) runs the FINAL pass's feature-resolution logits (``RPMMs.lowres``, element 0).

The reference draws the EM's initial mu per forward: every step here starts with ``model.step_pmm_init()`` (a fresh draw into
the model's ``pmm_mu0`` buffer, outside the captured graph) unless the init is pinned (``model.set_pmm_init``).

The round loop is the shared one: it aggregates the cross-entropy of the final output (what the reference calls ``loss_p1``)
with mIoU and bIoU, and the command's result line says ``Loss_p1``.  The sum of the three passes' losses is returned per step by
``test_step``; aggregating it over a round would need a wider ``DeviceRoundTable``.

``test_bank`` is ``test`` with every class's support enrolled once per round into a support bank (``BankEvaluator`` below).

``train_head`` trains the head behind a FROZEN trunk (``pemp_amd.train_rpmms``): a deliberate departure from the reference, whose
``maybe_fix_params()`` freezes nothing for RPMMs so that its ``train`` also updates the trunk's convs.  ``train`` (the
reference's command name) still raises: trunk training is not built."""
import numpy as np
import torch

from .. import ops
from ..config import Experiment
from ..networks.rpmms import WGEN_SEED, ModelClass, net_ingredient  # noqa: F401
from ..train_rpmms import RPMMsTrainer
from .pemp_stage1 import INGREDIENTS, SyntheticEpisodes, eval_episodes, get_val_labels, num_classes  # noqa: F401
from .pemp_stage1 import BankEvaluator as _BankEvaluator
from .pemp_stage1 import Evaluator as _Evaluator
from .pemp_stage1 import NWayMixin, SemanticMixin

NAME = "PEMP"
ex = Experiment(name=NAME, ingredients=[net_ingredient] + INGREDIENTS[1:])      # RPMMs' own net ingredient; data, tr, te, g, d


@ex.config
def ex_config():
    tag = "rpmms"               # str, configuration tag
    shot = 1                    # int, support samples per episode
    query = 1                   # int, query samples per episode
    split = -1                  # int, split number [0, 1, 2, 3], required
    seed = 1234                 # int, random seed
    ckpt = "bestckpt.pth"       # str, checkpoint file
    exp_id = -1                 # experiment id to load checkpoint
    loss = "ce"                 # str, loss type [ce/cedt]
    sigma = 5.                  # float, sigma of the DT loss
    loss_coef = 1.              # float, coefficient of the auxiliary loss
    trunk_precision = "f32_chain"   # str, frozen-trunk convs of train_head [f32_chain/split3]; test / train ignore it
    p = {"cls": -1, "sup": "", "qry": ""}


class Evaluator(_Evaluator):
    """The stage-1 evaluator on RPMMs' final logits; ``last_outputs`` keeps the step's (out2, out0, out1)."""

    def __init__(self, model, device=None, use_graph=True, splitk=None):
        super().__init__(model, device=device, use_graph=use_graph, lanes=1, splitk=splitk)   # one lane: the steps share pmm_mu0
        self.last_outputs = None

    def _lowres(self, dev_in):
        sup_img, sup_mask, qry_img = dev_in
        self.model.check_inputs(sup_img, qry_img)          # before a graph is captured for a shape the model rejects
        self.model.step_pmm_init()
        with ops.eval_splitk(ops.EVAL_SPLITK if self.splitk is None else self.splitk):
            self.last_outputs = self.model.lowres_graphed(*dev_in) if self.use_graph else self.model.lowres(*dev_in)
        return self.last_outputs[0]

    def test_step(self, inputs, qry_msk, **kwargs):
        """Reference contract (entry/rpmms.py ``test_step``): -> (qry_pred numpy [B,H,W], loss, loss_p1, loss_p2) with loss the
        sum of the three passes' cross-entropies, loss_p1 the final pass's (out2), loss_p2 the second pass's (out1)."""
        am, stats = self.test_step_device(inputs, qry_msk)
        tgt = qry_msk.view(-1, *qry_msk.shape[-2:]).to(self.device, non_blocking=True)
        with torch.no_grad():
            side = [ops.eval_tail(o, tgt, ws_cache=self._ws)[1] for o in self.last_outputs[1:]]       # out0, out1
        st = torch.stack([stats] + side).cpu().numpy()                                                # one host synchronisation
        ce = [float(s[:, 0].sum() / max(s[:, 1].sum(), 1.0)) for s in st]                             # out2, out0, out1
        return am.cpu().numpy(), ce[0] + ce[1] + ce[2], ce[0], ce[2]


@ex.command
def test(_config, split, shot, query, exp_id, ckpt, seed):
    import logging
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    logger = logging.getLogger(NAME)
    if split < 0:
        raise ValueError("Argument `split` is required! For example: `python -m pemp_amd.entry.rpmms test with split=0`")
    if shot != 1 or query != 1:
        raise ValueError("RPMMs is 1-shot with one query per episode (shot=1 query=1), as the reference is (rpmms.py:129, 266-267)")
    torch.manual_seed(seed)
    from ..core.snapshots import load_for_eval
    model = ModelClass(logger)
    load_for_eval(model, _config, exp_id, ckpt, logger, wgen_seed=WGEN_SEED)
    model = model.cuda().eval()
    ev = Evaluator(model)
    d = _config["data"]
    data = eval_episodes(d, shot, split)
    loss, miou, biou = ev.start_eval_loop(data, num_classes(d["dataset"]), split, _config["te"]["epochs"], logger,
                                          batch=d["test_bs"], dataset_name=d["dataset"])
    return f"Loss_p1: {loss:.4f}, mIoU: {np.mean(miou) * 100:.2f}, bIoU: {np.mean(biou) * 100:.2f}"


class BankEvaluator(_BankEvaluator):
    """The enroll-once evaluator (entry.pemp_stage1.BankEvaluator) on RPMMs' support banks, with one difference: it calls
    ``model.step_pmm_init()`` before each enrolment.  That is one draw of the EM's initial mu per class and round, where ``test``
    draws one per step (a pinned init stays as it is on both)."""

    def _enroll(self, slot, cls, sup_img, sup_mask):
        self.model.step_pmm_init()
        super()._enroll(slot, cls, sup_img, sup_mask)


@ex.command
def test_bank(_config, split, shot, query, exp_id, ckpt, seed):
    """``python -m pemp_amd.entry.rpmms test_bank with split=0 ckpt=wgen``: ``test`` with the enroll-once protocol: every class's
    support is enrolled once per round into a support bank (``RPMMs.enroll``), every query of the round is segmented against
    its class (``RPMMs.segment_graphed``)."""
    from .pemp_stage1 import run_test_bank
    if split < 0:
        raise ValueError("Argument `split` is required! For example: `python -m pemp_amd.entry.rpmms test_bank with split=0`")
    if shot != 1 or query != 1:
        raise ValueError("RPMMs is 1-shot with one query per episode (shot=1 query=1), as the reference is (rpmms.py:129, 266-267)")
    return run_test_bank(_config, NAME, ModelClass, split, shot, exp_id, ckpt, seed, evaluator=BankEvaluator, loss_label="Loss_p1",
                         wgen_seed=WGEN_SEED)


class NWayEvaluator(NWayMixin, BankEvaluator):
    """Every query against every enrolled class (entry.pemp_stage1.NWayMixin) over this entry's ``BankEvaluator``: the initial mu
    is drawn before each enrolment as there."""


@ex.command
def test_nway(_config, split, shot, query, exp_id, ckpt, seed):
    """``python -m pemp_amd.entry.rpmms test_nway with split=0 ckpt=wgen``: ``test_bank`` with every query meeting every enrolled
    class; ``Loss_p1`` is ``test_bank``'s, mIoU and bIoU are those of the classes under competition."""
    from .pemp_stage1 import run_test_bank
    if split < 0:
        raise ValueError("Argument `split` is required! For example: `python -m pemp_amd.entry.rpmms test_nway with split=0`")
    if shot != 1 or query != 1:
        raise ValueError("RPMMs is 1-shot with one query per episode (shot=1 query=1), as the reference is (rpmms.py:129, 266-267)")
    return run_test_bank(_config, NAME, ModelClass, split, shot, exp_id, ckpt, seed, evaluator=NWayEvaluator, loss_label="Loss_p1",
                         command="test_nway", wgen_seed=WGEN_SEED)


class SemanticEvaluator(SemanticMixin, BankEvaluator):
    """The semantic scoring of every query against every enrolled class (entry.pemp_stage1.SemanticMixin) over this entry's
    ``BankEvaluator``: the initial mu is drawn before each enrolment as there."""


@ex.command
def test_semantic(_config, split, shot, query, exp_id, ckpt, seed):
    """``python -m pemp_amd.entry.rpmms test_semantic with split=0 ckpt=wgen``: ``test_nway``'s rounds scored as a semantic
    segmentation over the split's classes: mIoU over the classes, mIoU with the background and the pixel accuracy."""
    from .pemp_stage1 import run_test_semantic
    if split < 0:
        raise ValueError("Argument `split` is required! For example: `python -m pemp_amd.entry.rpmms test_semantic with split=0`")
    if shot != 1 or query != 1:
        raise ValueError("RPMMs is 1-shot with one query per episode (shot=1 query=1), as the reference is (rpmms.py:129, 266-267)")
    return run_test_semantic(_config, NAME, ModelClass, split, shot, exp_id, ckpt, seed, evaluator=SemanticEvaluator,
                             wgen_seed=WGEN_SEED)


def head_train_batches(trainer, dcfg, shot, split, rank, steps_per_epoch, device):
    """-> ``batches(epoch)`` for ``TrainingLoop``: synthetic episodes with the query label at the input size (the reference resizes
    a training label with its image).  When an epoch's batches are used up, the reference's per-epoch line (entry/rpmms.py:133,
    141-144: the means of loss / loss_p1 / loss_p2 over the epoch's steps) is logged from what the trainer collected."""
    from .train_stage1 import synthetic_batches

    def batches(epoch):
        trainer.epoch_losses = []
        yield from synthetic_batches(dcfg["bs"], shot, steps_per_epoch, dcfg["seed"] + 7919 * epoch, rank, dcfg["height"], dcfg["width"])
        if trainer.epoch_losses and trainer.logger is not None:
            loss, p1, p2 = torch.stack([torch.stack(row) for row in trainer.epoch_losses]).mean(dim=0).tolist()
            lr = trainer.optimizer.param_groups[0]["lr"] if trainer.optimizer is not None else trainer.lr
            trainer.logger.info(f"[TRAIN] loss: {loss:.5f} - loss_p1: {p1:.5f} - loss_p2: {p2:.5f} - lr: {lr:g}")
    return batches


class HeadTrainer(RPMMsTrainer):
    """``RPMMsTrainer`` that keeps every step's (loss, loss_p1, loss_p2) for the epoch's log line (``head_train_batches``)."""

    def __init__(self, model, logger=None, **kw):
        super().__init__(model, **kw)
        self.logger, self.epoch_losses = logger, []

    def train_step(self, sup_img, sup_mask, qry_img, qry_msk=None):
        out = super().train_step(sup_img, sup_mask, qry_img, qry_msk=qry_msk)
        self.epoch_losses.append(out)
        return out


@ex.command
def train_head(_config, split, shot, query, seed, loss, sigma, exp_id, ckpt, trunk_precision):
    """``python -m pemp_amd.entry.rpmms train_head with split=0 ckpt=<checkpoint | wgen> [trunk_precision=split3]``: RPMMs' training procedure
    (entry/rpmms.py:107-149) for a FROZEN trunk -- the head trains on the HIP path (the reference also updates the trunk's convs:
    not built), per-epoch evaluation, ``ckpt.pth`` / ``bestckpt.pth`` (reference-loadable state_dicts) under
    ``<g.model_dir>/<tag>/<id>``."""
    from .pemp_stage1 import run_training
    if shot != 1 or query != 1:
        raise ValueError("RPMMs is 1-shot with one query per episode (shot=1 query=1), as the reference is (rpmms.py:129, 266-267)")
    if _config["data"].get("base_dir"):
        raise ValueError("train_head reads synthetic episodes only: leave data.base_dir empty")

    def make_trainer(logger, dev):
        from ..core.snapshots import load_for_eval
        model = ModelClass(logger)
        load_for_eval(model, _config, exp_id, ckpt, logger, wgen_seed=WGEN_SEED)     # the frozen trunk comes from a checkpoint
        return HeadTrainer(model.freeze_trunk(), logger=logger, lr=_config["tr"]["lr"], device=dev, loss=loss, sigma=sigma,
                           trunk_precision=trunk_precision)

    return run_training(_config, NAME, make_trainer, lambda tr, dev: Evaluator(tr.model, device=dev), split, shot, seed, exp_id,
                        batches=head_train_batches)


@ex.command
def train(_config):
    raise NotImplementedError("RPMMs is an inference path here: `test` runs it; training (entry/rpmms.py) is not ported")


if __name__ == "__main__":
    print(ex.run_commandline())
