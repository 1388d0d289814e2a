"""PFENet evaluation harness on MI355X (counterpart of the reference's entry/pfenet.py: config :27-45, ``Evaluator.test_step``
:54-60, ``test`` :129-148).  The stage-1 evaluator (batching, sharding, hipGraph replay, fused upsample + CE + argmax +
tp/fp/fn tail) runs the model's feature-resolution logits (``PFENet.lowres``); ``test_bank`` is ``test`` with every class's
supports enrolled once per round (``PFENet.enroll`` / ``segment_graphed``).  ``train_head`` trains the head behind the frozen
trunk (``pemp_amd.train_pfenet``: the reference runs ``layer0 .. layer4`` under ``no_grad``) on synthetic episodes; ``train``, the
reference's whole procedure on PASCAL-5i, raises."""
from ..config import Experiment
from ..networks.pfenet import WGEN_SEED, ModelClass  # noqa: F401
from .pemp_stage1 import INGREDIENTS, SyntheticEpisodes, eval_episodes, get_val_labels, num_classes  # noqa: F401
from .pemp_stage1 import Evaluator as _Evaluator

NAME = "PEMP"
ex = Experiment(name=NAME, ingredients=INGREDIENTS[1:])      # data, tr, te, g, d (the reference's PFENet has no net ingredient)


@ex.config
def ex_config():
    tag = "pfenet"              # str, configuration tag
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
    """The stage-1 evaluator on PFENet's feature-resolution logits (entry/pfenet.py:54-60: forward at the label size, CE,
    argmax)."""

    def _lowres(self, dev_in):
        sup_img, sup_mask, qry_img = dev_in
        self.model.check_inputs(sup_img, qry_img)          # before a graph is captured for a shape the model rejects
        return super()._lowres(dev_in)


@ex.command
def test(_config, split, shot, query, exp_id, ckpt):
    import logging
    import numpy as np
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    logger = logging.getLogger(NAME)
    if split < 0:
        raise ValueError("Argument `split` is required! For example: `python -m pemp_amd.entry.pfenet test with split=0`")
    if query != 1:
        raise ValueError("PFENet takes exactly one query per episode (query=1)")
    from ..core.snapshots import load_for_eval
    model = ModelClass(shot, logger)
    load_for_eval(model, _config, exp_id, ckpt, logger, wgen_seed=WGEN_SEED)
    model = model.cuda().eval()
    ev = Evaluator(model)
    d = _config["data"]
    data = eval_episodes(d, shot, split)
    loss, miou, biou = ev.start_eval_loop(data, num_classes(d["dataset"]), split, _config["te"]["epochs"], logger,
                                          batch=d["test_bs"], dataset_name=d["dataset"])
    return f"Loss: {loss:.4f}, mIoU: {np.mean(miou) * 100:.2f}, bIoU: {np.mean(biou) * 100:.2f}"


@ex.command
def test_bank(_config, split, shot, query, exp_id, ckpt):
    """``python -m pemp_amd.entry.pfenet test_bank with split=0 ckpt=wgen [shot=5]``: ``test`` with the enroll-once protocol
    (entry.pemp_stage1.BankEvaluator): every class's supports are enrolled once per round into a support bank
    (``PFENet.enroll``), every query of the round is segmented against its class (``PFENet.segment_graphed``)."""
    from .pemp_stage1 import run_test_bank
    if query != 1:
        raise ValueError("PFENet takes exactly one query per episode (query=1)")
    return run_test_bank(_config, NAME, lambda logger: ModelClass(shot, logger), split, shot, exp_id, ckpt, wgen_seed=WGEN_SEED)


@ex.command
def test_nway(_config, split, shot, query, exp_id, ckpt):
    """``python -m pemp_amd.entry.pfenet test_nway with split=0 ckpt=wgen [shot=5]``: ``test_bank`` with every query meeting
    every enrolled class (entry.pemp_stage1.NWayEvaluator)."""
    from .pemp_stage1 import NWayEvaluator, run_test_bank
    if query != 1:
        raise ValueError("PFENet takes exactly one query per episode (query=1)")
    return run_test_bank(_config, NAME, lambda logger: ModelClass(shot, logger), split, shot, exp_id, ckpt, evaluator=NWayEvaluator,
                         command="test_nway", wgen_seed=WGEN_SEED)


@ex.command
def test_semantic(_config, split, shot, query, exp_id, ckpt):
    """``python -m pemp_amd.entry.pfenet test_semantic with split=0 ckpt=wgen [shot=5]``: ``test_nway``'s rounds scored as a
    semantic segmentation over the split's classes (entry.pemp_stage1.SemanticEvaluator)."""
    from .pemp_stage1 import run_test_semantic
    if query != 1:
        raise ValueError("PFENet takes exactly one query per episode (query=1)")
    return run_test_semantic(_config, NAME, lambda logger: ModelClass(shot, logger), split, shot, exp_id, ckpt, wgen_seed=WGEN_SEED)


def head_train_batches(trainer, dcfg, shot, split, rank, steps_per_epoch, device):
    """-> ``batches(epoch)`` for ``TrainingLoop``: synthetic episodes with the query label at the input size (the reference resizes
    a training label with its image)."""
    from .train_stage1 import synthetic_batches
    return lambda epoch: synthetic_batches(dcfg["bs"], shot, steps_per_epoch, dcfg["seed"] + 7919 * epoch, rank, dcfg["height"],
                                           dcfg["width"])


@ex.command
def train_head(_config, split, shot, query, seed, loss, sigma, loss_coef, exp_id, ckpt, trunk_precision):
    """``python -m pemp_amd.entry.pfenet train_head with split=0 ckpt=<checkpoint | wgen> [shot=5] [loss_coef=1.] [trunk_precision=split3]``: PFENet's
    training procedure (entry/pfenet.py:63-126) -- the head trains on the HIP path behind the frozen trunk, per-epoch evaluation,
    ``ckpt.pth`` / ``bestckpt.pth`` (reference-loadable state_dicts) under ``<g.model_dir>/<tag>/<id>``."""
    from .pemp_stage1 import run_training
    if query != 1:
        raise ValueError("PFENet takes exactly one query per episode (query=1)")
    if _config["data"].get("base_dir"):
        raise ValueError("train_head reads synthetic episodes only: leave data.base_dir empty")

    def make_trainer(logger, dev):
        from ..core.snapshots import load_for_eval
        from ..train_pfenet import PFENetTrainer
        model = ModelClass(shot, logger)
        load_for_eval(model, _config, exp_id, ckpt, logger, wgen_seed=WGEN_SEED)     # the frozen trunk comes from a checkpoint
        return PFENetTrainer(model, lr=_config["tr"]["lr"], device=dev, loss=loss, sigma=sigma, loss_coef=loss_coef,
                             trunk_precision=trunk_precision)

    return run_training(_config, NAME, make_trainer, lambda tr, dev: Evaluator(tr.model, device=dev), split, shot, seed, exp_id,
                        batches=head_train_batches)


@ex.command
def train(_config):
    raise NotImplementedError("PFENet is an inference path here: `test` runs it; training (entry/pfenet.py:63-126) is not ported")


if __name__ == "__main__":
    print(ex.run_commandline())
