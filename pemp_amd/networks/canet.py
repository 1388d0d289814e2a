"""CANet on MI355X: inference counterpart of the reference's ``networks/canet.py`` (module surface :10-22,234; constructor
:50-125; forward :127-209).

The module tree holds the reference's parameters under the reference's ``state_dict`` keys (tests/golden/
state_keys_canet.json); the forward runs on ``pemp_amd.canet_engine`` (HIP kernels only).  Unlike the reference the
constructor reads no ImageNet checkpoint: a trained model comes from ``load_weights`` / ``ckpt``.  The module's forward is
inference only: a ``train()``-mode forward raises; the head trains through the explicit ``pemp_amd.train_canet.CANetTrainer``
(``entry.canet``'s ``train_head``).  Beside the reference's ``forward`` there is a slot form for the evaluator
(``lowres_slots`` / ``lowres_graphed_slots``): the same forward with the history read from, and the softmax written to, rows
of a device-resident table."""
from pathlib import Path

import torch
import torch.nn as nn

from .. import canet_engine, ops
from ..config import Ingredient
from . import backbones
from .pemp_stage1 import _HeadMixin

net_ingredient = Ingredient("net", save_git_info=False)
pretrained_weights = {
    "resnet50": Path(__file__).parents[2] / "data/resnet50-19c8e357.pth",
}
#: Wgen seed of ``ckpt=wgen`` runs and of the fixtures (tests/golden/make_golden_canet.py): with the default seed the classifier
#: answers "background" everywhere on the synthetic episodes
WGEN_SEED = 1259
_NOT_TRAINED = "CANet is an inference path here: call model.eval() (training is not ported)"


@net_ingredient.config
def net_config():
    init_channels = 3           # int, input channels of the model
    drop_rate = 0.5             # float, Dropout2d rate (train only)
    history = True              # bool, use history_mask or not
    freeze_backbone = True      # bool, freeze backbone parameters or not


def _conv_relu_drop(cin, cout, k, dil, drop_rate):
    pad = dil if k == 3 else 0
    return nn.Sequential(nn.Conv2d(cin, cout, kernel_size=k, stride=1, padding=pad, dilation=dil, bias=True),
                         nn.ReLU(inplace=True), nn.Dropout2d(drop_rate))


def _residual(cin):
    return nn.Sequential(nn.ReLU(), nn.Conv2d(cin, 256, kernel_size=3, stride=1, padding=1, bias=True),
                         nn.ReLU(), nn.Conv2d(256, 256, kernel_size=3, stride=1, padding=1, bias=True))


class CaNet(_HeadMixin, backbones.BaseModel):
    num_classes = 2

    @net_ingredient.capture
    def __init__(self, logger, init_channels, drop_rate, history, freeze_backbone):
        super().__init__()
        self.use_history = history
        self.freeze_backbone = freeze_backbone
        self.encoder = backbones.ResNetParams(init_channels, (3, 4, 6), freeze_bn=True)
        self.layer5 = _conv_relu_drop(512 + 1024, 256, 3, 2, drop_rate)
        self.layer55 = _conv_relu_drop(256 * 2, 256, 3, 2, drop_rate)
        self.aspp_0 = _conv_relu_drop(256, 256, 1, 1, drop_rate)
        self.aspp_1 = _conv_relu_drop(256, 256, 1, 1, drop_rate)
        self.aspp_2 = _conv_relu_drop(256, 256, 3, 6, drop_rate)
        self.aspp_3 = _conv_relu_drop(256, 256, 3, 12, drop_rate)
        self.aspp_4 = _conv_relu_drop(256, 256, 3, 18, drop_rate)
        self.layer6 = _conv_relu_drop(1280, 256, 1, 1, drop_rate)
        self.residual_1 = _residual(256 + 2 if self.use_history else 256)
        self.residual_2 = _residual(256)
        self.residual_3 = _residual(256)
        self.layer7 = nn.Conv2d(256, self.num_classes, kernel_size=1, stride=1, bias=True)
        for m in self.modules():                                  # canet.py:211-214
            if isinstance(m, nn.Conv2d):
                m.weight.data.normal_(0, 0.01)
        if logger is not None:
            logger.info(f"           ==> Model {self.__class__.__name__} created")

    def maybe_fix_params(self, freeze_backbone=None):
        """canet.py:219-231: the stem conv and the three stages stop receiving gradients."""
        if self.freeze_backbone if freeze_backbone is None else freeze_backbone:
            for mod in (self.encoder.conv1, self.encoder.layer1, self.encoder.layer2, self.encoder.layer3):
                for prm in mod.parameters():
                    prm.requires_grad = False

    def _build_engine(self, eng, arena):
        eng["canet"] = canet_engine.CANetEngine(self, arena)

    @staticmethod
    def feature_hw(H, W):
        return canet_engine.feature_hw(H, W)

    def check_inputs(self, sup_img, qry_img, history_mask=None):
        """The shape contract, checked before anything is launched."""
        if qry_img.dim() != 5 or qry_img.shape[1] != 1:
            raise ValueError(f"CANet takes exactly one query per episode here (query=1), got qry_img {tuple(qry_img.shape)}")
        if sup_img.dim() != 5 or tuple(qry_img.shape[-2:]) != tuple(sup_img.shape[-2:]) or qry_img.shape[0] != sup_img.shape[0]:
            raise ValueError(f"support {tuple(sup_img.shape)} and query {tuple(qry_img.shape)} must share batch and image size")
        if history_mask is not None:
            h, w = self.feature_hw(*sup_img.shape[-2:])
            if tuple(history_mask.shape) != (sup_img.shape[0], 1, 2, h, w):
                raise ValueError(f"history_mask must be [B,1,2,{h},{w}] (the trunk's feature size), got {tuple(history_mask.shape)}")

    def lowres(self, sup_img, sup_mask, qry_img, history_mask=None, ret_ind=False):
        """Feature-resolution logits [B,2,h,w] (everything before the final F.interpolate, canet.py:156-159) -> (logits, None).
        ``history_mask`` [B,1,2,h,w] or None (zeros, what the loader passes first, data_kits/pascal_voc.py:423-424)."""
        if self.training:
            raise NotImplementedError(_NOT_TRAINED)
        self.check_inputs(sup_img, qry_img, history_mask)
        eng = self._engine_for(sup_img.device)
        hist = None
        if history_mask is not None and self.use_history:
            hist = history_mask.reshape(history_mask.shape[0], *history_mask.shape[-3:]).float().contiguous()
        return eng["canet"].lowres(sup_img, sup_mask, qry_img, history=hist), None

    def lowres_slots(self, sup_img, sup_mask, qry_img, table, read_slot, write_slot):
        """The slot form: episode b reads its history from row ``read_slot[b]`` of ``table`` [nslots,2,h,w] (< 0: zeros) and,
        after the forward, its softmax goes to row ``write_slot[b]`` (< 0: nowhere).  Slots are device int32 [B]; the caller
        names no write slot twice.  -> logits [B,2,h,w]."""
        if self.training:
            raise NotImplementedError(_NOT_TRAINED)
        self.check_inputs(sup_img, qry_img)
        self._require_eval_gpu(self, sup_img, sup_mask, qry_img, table, read_slot, write_slot)
        h, w = self.feature_hw(*sup_img.shape[-2:])
        if table.dim() != 4 or tuple(table.shape[1:]) != (2, h, w):
            raise ValueError(f"the history table must be [nslots,2,{h},{w}], got {tuple(table.shape)}")
        eng = self._engine_for(sup_img.device)
        if not self.use_history:
            return eng["canet"].lowres(sup_img, sup_mask, qry_img)
        pred = eng["canet"].lowres(sup_img, sup_mask, qry_img, history=table, slot=read_slot)
        ops.canet_history_update(pred, table=table, slot=write_slot)
        return pred

    def lowres_graphed_slots(self, sup_img, sup_mask, qry_img, table, read_slot, write_slot):
        """``lowres_slots`` replayed from a captured hipGraph (one per input signature and table).  The images and the slots
        are copied into static buffers before each replay, so a replay may name other slots than the captured call; the
        table is addressed in place.  The returned tensor is the graph's static output."""
        self._require_eval_gpu(self, sup_img, sup_mask, qry_img, table, read_slot, write_slot)
        inputs = (sup_img, sup_mask, qry_img, read_slot, write_slot)
        key = ("slots", table.data_ptr(), tuple(table.shape)) + tuple((tuple(t.shape), t.dtype) for t in inputs) + (ops.EVAL_SPLITK,)
        eng = self._engine_for(sup_img.device)
        none = None if key in eng.get("graphs", ()) else torch.full_like(write_slot, -1)      # the warm-up writes no table row
        return self._replay(eng, key, inputs, lambda s: self.lowres_slots(*s[:3], table, s[3], none),
                            lambda s: self.lowres_slots(*s[:3], table, *s[3:]))

    def forward(self, sup_img, sup_mask, qry_img, out_shape=None, history_mask=None):
        """Same contract as the reference's eval forward (canet.py:127-161): ``out_shape`` False -> the feature-resolution
        logits [B,2,h,w]; None -> the input size; a tuple -> that size (bilinear, align_corners)."""
        if self.training:
            raise NotImplementedError(_NOT_TRAINED)
        self.check_inputs(sup_img, qry_img, history_mask)
        self._require_eval_gpu(self, *[t for t in (sup_img, sup_mask, qry_img, history_mask) if t is not None])
        with torch.no_grad():
            pred, _ = self.lowres(sup_img, sup_mask, qry_img, history_mask)
            if out_shape is False:
                return pred.clone()
            if out_shape is None:
                out_shape = tuple(sup_img.shape[-2:])
            return self._finish(pred, None, tuple(int(v) for v in out_shape))


ModelClass = CaNet
