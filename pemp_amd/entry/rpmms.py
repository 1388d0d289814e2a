"""RPMMs evaluation harness on MI355X (counterpart of the reference's entry/rpmms.py: its configuration, ``Evaluator.test_step``
-> (qry_pred, loss, loss_p1, loss_p2), ``test``).  The stage-1 evaluator (batching, sharding, hipGraph replay, fused upsample +
CE + argmax + tp/fp/fn tail) runs the FINAL pass's feature-resolution logits (``RPMMs.lowres``, element 0).

The reference draws the EM's initial mu per forward: every step here starts with ``model.step_pmm_init()`` (a fresh draw into
the model's ``pmm_mu0`` buffer, outside the captured graph) unless the init is pinned (``model.set_pmm_init``).

The round loop is the shared one: it aggregates the cross-entropy of the final output (what the reference calls ``loss_p1``)
with mIoU and bIoU, and the command's result line says ``Loss_p1``.  The sum of the three passes' losses is returned per step by
``test_step``; aggregating it over a round would need a wider ``DeviceRoundTable``.  Training is not
ported: ``train`` raises."""
import numpy as np
import torch

from .. import ops
from ..config import Experiment
from ..networks.rpmms import WGEN_SEED, ModelClass, net_ingredient  # noqa: F401
from .pemp_stage1 import INGREDIENTS, SyntheticEpisodes, eval_episodes, get_val_labels, num_classes  # noqa: F401
from .pemp_stage1 import Evaluator as _Evaluator

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


@ex.command
def train(_config):
    raise NotImplementedError("RPMMs is an inference path here: `test` runs it; training (entry/rpmms.py) is not ported")


if __name__ == "__main__":
    print(ex.run_commandline())
