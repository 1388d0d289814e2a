"""RPMMs on MI355X: inference counterpart of the reference's ``networks/rpmms.py`` (module surface :11-25,350; PMMs :28-141;
constructor :146-211; forward :213-287; loss / prediction :289-319; load_weights :321-347).

The module tree holds the reference's parameters under the reference's ``state_dict`` keys (tests/golden/
state_keys_rpmms.json, with the reference's spelling ``residule``); the forward runs on ``pemp_amd.rpmms_engine`` (HIP kernels
only).  Unlike the reference the constructor reads no ImageNet checkpoint: a trained model comes from ``load_weights`` /
``ckpt``.  A ``train()``-mode forward raises: the head trains through ``pemp_amd.train_rpmms`` (explicit forward / backward behind
a frozen trunk, ``freeze_trunk``), not through autograd.  1-shot, one query: the reference's own ``bmm`` (:129) and ``cat``
(:266-267) fail for anything else.

The initial mu of the EM: the reference draws a fresh normal(0, sqrt(2 / K)) [1,256,K] tensor per forward and per K and
l2-normalises it over the channels (:41-43); foreground and background, and every image of the batch, share it.  Here the
model owns ONE device buffer ``pmm_mu0`` [10,256] (row 0: K = 1, rows 1..3: K = 3, rows 4..9: K = 6) that the EM kernel reads:
``resample_pmm_init`` refills it (torch ops, outside any captured graph; a graph replay reads the buffer's current contents),
``set_pmm_init`` pins it until ``resample_pmm_init`` is called again."""
import math
from pathlib import Path

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops, rpmms_engine
from ..config import Ingredient
from . import backbones
from .pemp_stage1 import _HeadMixin

net_ingredient = Ingredient("net", save_git_info=False)
pretrained_weights = {
    "resnet50": Path(__file__).parents[2] / "data/resnet50-19c8e357.pth",
}
backbone_error = "Not supported backbone '{}'. [resnet50]"
#: Wgen seed of ``ckpt=wgen`` runs and of the fixtures (tests/golden/make_golden_rpmms.py)
WGEN_SEED = 1259
NUM_PRO_LIST = (1, 3, 6)
_NOT_TRAINED = "RPMMs is an inference path here: call model.eval() (training is not ported)"
_ONE_SHOT = ("RPMMs is 1-shot with one query per episode, as the reference is (its bmm(x_t[B], mu[B*S]) at rpmms.py:129 and the "
             "expand + cat at rpmms.py:266-267 fail for anything else)")


@net_ingredient.config
def net_config():
    dist_scalar = 20                        # int, a factor multiplied to cosine distance results
    init_channels = 3                       # int, input channels of the model
    out_channels = 512                      # int, output channels of the feature extractor
    backbone = "resnet50"                   # str, structure of the feature extractor. [resnet50]
    protos = 3                              # int, number of prototypes per class
    drop_rate = 0.5                         # float, drop rate used in the dropout


def _conv_relu_drop(cin, cout, k, pad, dil, drop_rate):
    return nn.Sequential(nn.Conv2d(cin, cout, kernel_size=k, stride=1, padding=pad, dilation=dil, bias=True), nn.ReLU(),
                         nn.Dropout2d(p=drop_rate))


def _residule(cin):
    return nn.Sequential(nn.ReLU(), nn.Conv2d(cin, 256, kernel_size=3, stride=1, padding=1, bias=True),
                         nn.ReLU(), nn.Conv2d(256, 256, kernel_size=3, stride=1, padding=1, bias=True))


class _ASPP(nn.Module):
    """Parameter holder of the reference's tail-less ASPP (backbones.py:279-306, ``tail=False``)."""

    def __init__(self, drop_rate):
        super().__init__()
        self.aspp_0 = _conv_relu_drop(256, 256, 1, 0, 1, drop_rate)
        self.aspp_1 = _conv_relu_drop(256, 256, 1, 0, 1, drop_rate)
        self.aspp_2 = _conv_relu_drop(256, 256, 3, 6, 6, drop_rate)
        self.aspp_3 = _conv_relu_drop(256, 256, 3, 12, 12, drop_rate)
        self.aspp_4 = _conv_relu_drop(256, 256, 3, 18, 18, drop_rate)


class RPMMs(_HeadMixin, backbones.BaseModel):
    num_pro_list = list(NUM_PRO_LIST)

    @net_ingredient.capture
    def __init__(self, logger, init_channels, out_channels, backbone, drop_rate):
        super().__init__()
        if backbone not in pretrained_weights:
            raise ValueError(backbone_error.format(backbone))
        self.model_res = backbones.ResNetParams(init_channels, (3, 4, 6), freeze_bn=True)
        self.layer5 = nn.Sequential(nn.Conv2d(1536, 256, kernel_size=3, stride=1, padding=2, dilation=2, bias=True),
                                    nn.BatchNorm2d(256), nn.ReLU())
        self.layer55 = _conv_relu_drop(256 * 2, 256, 3, 2, 2, drop_rate)
        self.layer56 = _conv_relu_drop(256 + 2, 256, 3, 1, 1, drop_rate)
        self.layer6 = _ASPP(drop_rate)
        self.layer7 = _conv_relu_drop(1280, 256, 1, 0, 1, drop_rate)
        self.layer9 = nn.Conv2d(256, 2, kernel_size=1, stride=1, bias=True)
        self.residule1 = _residule(256 + 2)
        self.residule2 = _residule(256)
        self.residule3 = _residule(256)
        self.register_buffer("pmm_mu0", torch.zeros(ops.RPMMS_COLS, 256), persistent=False)     # not a state_dict entry
        self.pmm_init_pinned = False
        self.resample_pmm_init()
        if logger is not None:
            logger.info(f"           ==> Model {self.__class__.__name__} created")

    # -- the EM's initial mu ---------------------------------------------------------------------------------------------------
    def resample_pmm_init(self, generator=None):
        """A fresh draw for K = 1, 3, 6 in this order, as the reference makes per forward (rpmms.py:41-43): normal(0, sqrt(2 / K)),
        l2-normalised over the channels with the 1e-6 epsilon.  Drawn on the generator's device (default: the buffer's) and
        copied into ``pmm_mu0`` in place; ends a pinned init."""
        dev = generator.device if generator is not None else self.pmm_mu0.device
        rows = []
        for k in NUM_PRO_LIST:
            mu = torch.empty((1, 256, k), dtype=torch.float32, device=dev).normal_(0, math.sqrt(2.0 / k), generator=generator)
            rows.append((mu / (1e-6 + mu.norm(dim=1, keepdim=True)))[0].t())
        self.pmm_mu0.copy_(torch.cat(rows))
        self.pmm_init_pinned = False

    def set_pmm_init(self, mus):
        """Pin the initial mu: ``mus`` = {1: t1, 3: t3, 6: t6}, tensors [256,K] or [1,256,K], already normalised.  Stays until
        ``resample_pmm_init`` is called explicitly (``step_pmm_init`` leaves a pinned init alone)."""
        if set(mus) != set(NUM_PRO_LIST):
            raise ValueError(f"set_pmm_init: one tensor per K in {NUM_PRO_LIST}, got keys {sorted(mus)}")
        rows = []
        for k in NUM_PRO_LIST:
            t = torch.as_tensor(mus[k], dtype=torch.float32)
            t = t[0] if t.dim() == 3 and t.shape[0] == 1 else t
            if tuple(t.shape) != (256, k):
                raise ValueError(f"set_pmm_init: the K = {k} tensor must be [256,{k}] or [1,256,{k}], got {tuple(torch.as_tensor(mus[k]).shape)}")
            rows.append(t.t())
        self.pmm_mu0.copy_(torch.cat(rows))
        self.pmm_init_pinned = True

    def step_pmm_init(self, generator=None):
        """What an evaluation step does first: a fresh draw (the reference draws per forward) unless the init is pinned."""
        if not self.pmm_init_pinned:
            self.resample_pmm_init(generator)

    def freeze_trunk(self):
        """Every ``model_res`` parameter stops receiving gradients: what ``pemp_amd.train_rpmms`` trains behind (the reference's
        ``maybe_fix_params()`` freezes nothing for RPMMs; the HIP path trains the head only).  ``layer5`` stays trainable."""
        for prm in self.model_res.parameters():
            prm.requires_grad = False
        return self

    # -- engine ------------------------------------------------------------------------------------------------------------------
    def _build_engine(self, eng, arena):
        eng["rpmms"] = rpmms_engine.RPMMsEngine(self, arena)

    @staticmethod
    def feature_hw(H, W):
        return rpmms_engine.feature_hw(H, W)

    @staticmethod
    def check_inputs(sup_img, qry_img):
        """The shape contract, checked before anything is launched."""
        if sup_img.dim() != 5 or qry_img.dim() != 5 or sup_img.shape[1] != 1 or qry_img.shape[1] != 1:
            raise ValueError(f"{_ONE_SHOT}; got support {tuple(sup_img.shape)}, query {tuple(qry_img.shape)}")
        if tuple(qry_img.shape[-2:]) != tuple(sup_img.shape[-2:]) or qry_img.shape[0] != sup_img.shape[0]:
            raise ValueError(f"support {tuple(sup_img.shape)} and query {tuple(qry_img.shape)} must share batch and image size")

    def lowres(self, sup_img, sup_mask, qry_img, ret_ind=False):
        """Feature-resolution logits of the three passes, the FINAL one first: (out2, out0, out1), [B,2,h,w] each (the shared
        evaluator reads element 0)."""
        if self.training:
            raise NotImplementedError(_NOT_TRAINED)
        self.check_inputs(sup_img, qry_img)
        self._require_eval_gpu(self, sup_img, sup_mask, qry_img)
        out0, out1, out2 = self._engine_for(sup_img.device)["rpmms"].lowres(sup_img, sup_mask, qry_img)
        return out2, out0, out1

    # -- support banks (pemp_amd.bank.RPMMsBank): enroll supports once, segment many queries --------------------------------
    # ``segment`` / ``segment_lowres`` / ``segment_graphed`` are _HeadMixin's, with this family's bank and checks.
    _bank_family = "rpmms"
    _bank_backbone = "resnet50"

    @staticmethod
    def _bank_class():
        from ..bank import RPMMsBank
        return RPMMsBank

    def _bank_desc(self):
        return dict(family=self._bank_family, backbone=self._bank_backbone, precision=self.__dict__.get("_precision", "f32"), C=256)

    def enroll(self, sup_img, sup_mask, labels=None, out=None):
        """Supports of K classes, ``sup_img`` [K,1,3,H,W] and ``sup_mask`` [K,1,2,H,W] -> ``RPMMsBank``: one supports-only pass
        through the trunk and ``layer5``, the mask resize, the EM and the tap products of the foreground prototypes.  The EM
        starts from ``pmm_mu0`` as it stands: nothing is drawn here, call ``step_pmm_init()`` first when a fresh draw is wanted.
        ``out``: enroll into that bank (same K) in place -- its storage keeps its addresses, so captured graphs that read it see
        the new classes."""
        from ..bank import RPMMsBank
        if out is not None:
            self._check_bank(out, "enroll(out=)")
        self._require_eval_gpu(self)
        if sup_img.dim() != 5 or sup_img.shape[1] != 1:
            raise ValueError(f"{_ONE_SHOT}; got support {tuple(sup_img.shape)}")
        K, S, ch, H, W = sup_img.shape
        if tuple(sup_mask.shape) != (K, S, 2, H, W):
            raise ValueError(f"enroll: sup_mask must be [{K},{S},2,{H},{W}], got {tuple(sup_mask.shape)}")
        self._require_eval_gpu(self, sup_img, sup_mask)
        if out is not None and (len(out) != K or not out.mu.is_cuda):
            raise ValueError(f"enroll(out=): the bank holds {len(out)} classes on {out.mu.device}, {K} are enrolled")
        eng = self._engine_for(sup_img.device)["rpmms"]
        with torch.no_grad():
            if out is None:
                mu, taps = eng.support_side(sup_img, sup_mask)
                desc = self._bank_desc()
                return RPMMsBank(mu, taps, desc["backbone"], desc["precision"], labels=labels)
            eng.support_side(sup_img, sup_mask, out.mu, out.taps)
        if labels is not None:
            out.labels = RPMMsBank._labels(labels, K)
        return out

    def _segment_dev(self, bank, qry_img, index_dev, ret_ind):
        """-> (final logits, None): [N,2,h,w] with an index, [N,K,2,h,w] without.  The three passes of the call stay with the
        engine (``last_bank_passes``: out0, out1, out2 over the pairs, pair n * K + k without an index)."""
        out2 = self._engine_for(qry_img.device)["rpmms"].segment(bank, qry_img, index_dev)[2]
        lead = (qry_img.shape[0],) if index_dev is not None else (qry_img.shape[0], len(bank))
        return out2.view(lead + tuple(out2.shape[1:])), None

    def forward(self, sup_img, sup_mask, qry_img, out_shape=None):
        """The reference's eval forward (rpmms.py:213-254): (support_feature [B,256,h,w], out0, out1, out2), the logits at
        feature resolution [B,2,h,w] (``out_shape`` is not read there either; ``get_pred`` / ``get_loss`` resize)."""
        if self.training:
            raise NotImplementedError(_NOT_TRAINED)
        self.check_inputs(sup_img, qry_img)
        self._require_eval_gpu(self, sup_img, sup_mask, qry_img)
        with torch.no_grad():
            out2, out0, out1 = self.lowres(sup_img, sup_mask, qry_img)
            f5 = self._engine_for(sup_img.device)["rpmms"].last_layer5
            B = sup_img.shape[0]
            return f5[:B].permute(0, 3, 1, 2).contiguous(), out0.clone(), out1.clone(), out2.clone()

    # -- the reference's loss / prediction contracts (rpmms.py:289-319) ----------------------------------------------------------
    def get_loss(self, logits, query_label):
        """-> (sum of the three cross-entropies, CE of out2, CE of out1); ``query_label`` [B,1,H,W]; no ignore index."""
        _, out0, out1, out2 = logits
        b, _, h, w = query_label.size()
        label = query_label.view(b, h, w).long()
        ce = [F.cross_entropy(ops.upsample_bilinear_ac(o.contiguous(), (h, w)), label) for o in (out0, out1, out2)]
        return ce[0] + ce[1] + ce[2], ce[2], ce[1]

    def get_pred(self, logits, query_image):
        """-> (softmax of the final logits at the query image's size, its arg-max)."""
        out2 = logits[3]
        size = tuple(int(v) for v in query_image.size()[-2:])
        out_softmax = F.softmax(ops.upsample_bilinear_ac(out2.contiguous(), size), dim=1)
        return out_softmax, out_softmax.max(dim=1)[1]

    def load_weights(self, ckpt_path, logger):
        weights = torch.load(str(ckpt_path), map_location="cpu")
        if "state_dict" in weights:
            weights = weights["state_dict"]
        try:
            self.load_state_dict(weights)
        except RuntimeError as e:                                 # the reference's key fallback (rpmms.py:328-340)
            cur_weights = self.state_dict()
            for key in list(cur_weights.keys()):
                old_key = key.replace("aspp", "layer6")
                if old_key in weights:
                    cur_weights[key] = weights[old_key]
                else:
                    print("Checkpoint:", str(ckpt_path))
                    raise e
            self.load_state_dict(cur_weights)
        try:
            short_path = Path(ckpt_path).relative_to(Path(__file__).parents[2])
        except ValueError:
            short_path = ckpt_path
        logger.info(f"           ==> Model {self.__class__.__name__} initialized from {short_path}")


ModelClass = RPMMs
