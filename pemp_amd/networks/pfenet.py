"""PFENet on MI355X: inference counterpart of the reference's ``networks/pfenet.py`` (module surface :10-12,289; constructor
:52-155; forward :157-287) and its deep-base ResNet-50 (``networks/pfe_resent.py``: Bottleneck :62-98, ResNet :101-160).

The module tree holds the reference's parameters under the reference's ``state_dict`` keys (tests/golden/
state_keys_pfenet.json); the forward runs on ``pemp_amd.pfenet_engine`` (HIP kernels only).  Unlike the reference the
constructor reads no ImageNet checkpoint: a trained model comes from ``load_weights`` / ``ckpt``.  The module's forward is
inference only: a ``train()``-mode forward raises; the head trains through ``pemp_amd.train_pfenet.PFENetTrainer``."""
from pathlib import Path

import torch
import torch.nn as nn

from .. import pfenet_engine
from . import backbones
from .pemp_stage1 import _HeadMixin

pretrained_weights = {
    "resnet50v2": Path(__file__).parents[2] / "data/resnet50_v2.pth",
}
REDUCE = 256
CLASSES = 2
ZOOM = 8
#: Wgen seed of ``ckpt=wgen`` runs and of the fixtures (tests/golden/make_golden_pfenet.py): with the default seed the classifier
#: answers "background" everywhere on the synthetic episodes
WGEN_SEED = 1259


class Bottleneck(nn.Module):
    """Parameter holder of pfe_resent.Bottleneck (v1.5: stride and dilation on the 3x3 conv)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample


def _layer(inplanes, planes, blocks, stride, dilation):
    """One stage as PFENet leaves it (pfenet.py:68-77): layer 3 / 4 keep stride 1 (downsample too) and dilate their 3x3s."""
    ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, kernel_size=1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
    mods = [Bottleneck(inplanes, planes, stride, dilation, ds)] + [Bottleneck(planes * 4, planes, 1, dilation) for _ in range(1, blocks)]
    return nn.Sequential(*mods)


def _conv_relu(cin, cout, k):
    return [nn.Conv2d(cin, cout, kernel_size=k, padding=k // 2, bias=False), nn.ReLU(inplace=True)]


class PFENet(_HeadMixin, backbones.BaseModel):
    def __init__(self, shot, logger):
        super().__init__()
        self.zoom_factor = ZOOM
        self.criterion = nn.CrossEntropyLoss(ignore_index=255)
        self.shot = shot
        self.ppm_scales = list(pfenet_engine.PYRAMID_BINS)
        self.layer0 = nn.Sequential(
            nn.Conv2d(3, 64, 3, stride=2, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
            nn.Conv2d(64, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
            nn.Conv2d(64, 128, 3, padding=1, bias=False), nn.BatchNorm2d(128), nn.ReLU(inplace=True),
            nn.MaxPool2d(kernel_size=3, stride=2, padding=1))
        self.layer1 = _layer(128, 64, 3, 1, 1)
        self.layer2 = _layer(256, 128, 4, 2, 1)
        self.layer3 = _layer(512, 256, 6, 1, 2)
        self.layer4 = _layer(1024, 512, 3, 1, 4)
        self.cls = nn.Sequential(*_conv_relu(REDUCE, REDUCE, 3), nn.Dropout2d(p=0.1), nn.Conv2d(REDUCE, CLASSES, kernel_size=1))
        self.down_query = nn.Sequential(*_conv_relu(1024 + 512, REDUCE, 1), nn.Dropout2d(p=0.5))
        self.down_supp = nn.Sequential(*_conv_relu(1024 + 512, REDUCE, 1), nn.Dropout2d(p=0.5))
        self.pyramid_bins = self.ppm_scales
        self.avgpool_list = [nn.AdaptiveAvgPool2d(b) for b in self.pyramid_bins]
        nb = len(self.pyramid_bins)
        self.init_merge = nn.ModuleList([nn.Sequential(*_conv_relu(2 * REDUCE + 1, REDUCE, 1)) for _ in range(nb)])
        self.beta_conv = nn.ModuleList([nn.Sequential(*_conv_relu(REDUCE, REDUCE, 3), *_conv_relu(REDUCE, REDUCE, 3))
                                        for _ in range(nb)])
        self.inner_cls = nn.ModuleList([nn.Sequential(*_conv_relu(REDUCE, REDUCE, 3), nn.Dropout2d(p=0.1),
                                                      nn.Conv2d(REDUCE, CLASSES, kernel_size=1)) for _ in range(nb)])
        self.res1 = nn.Sequential(*_conv_relu(REDUCE * nb, REDUCE, 1))
        self.res2 = nn.Sequential(*_conv_relu(REDUCE, REDUCE, 3), *_conv_relu(REDUCE, REDUCE, 3))
        self.GAP = nn.AdaptiveAvgPool2d(1)
        self.alpha_conv = nn.ModuleList([nn.Sequential(nn.Conv2d(2 * REDUCE, REDUCE, kernel_size=1, bias=False), nn.ReLU())
                                         for _ in range(nb - 1)])
        if logger is not None:
            logger.info(f"           ==> Model {self.__class__.__name__} created")

    def _build_engine(self, eng, arena):
        eng["pfenet"] = pfenet_engine.PFENetEngine(self, arena)

    @staticmethod
    def check_inputs(sup_img, qry_img):
        """The reference's shape contract, checked before anything is launched."""
        H, W = sup_img.shape[-2:]
        if qry_img.dim() != 5 or qry_img.shape[1] != 1:
            raise ValueError(f"PFENet takes exactly one query per episode, got qry_img {tuple(qry_img.shape)}")
        if H != W or tuple(qry_img.shape[-2:]) != (H, W):
            raise ValueError(f"PFENet needs square inputs of one size (its views assume H == W, pfenet.py:204,222,225), "
                             f"got support {H}x{W}, query {tuple(qry_img.shape[-2:])}")
        if (H - 1) % 8 != 0:
            raise ValueError(f"PFENet needs (H - 1) % 8 == 0 (pfenet.py:164), got H = {H}")

    def lowres(self, sup_img, sup_mask, qry_img, ret_ind=False):
        """Feature-resolution logits [B,2,h,w] (everything before the final F.interpolate, :273-274) -> (logits, None)."""
        if self.training:
            raise NotImplementedError("PFENet is an inference path here: call model.eval() (training is not ported)")
        self.check_inputs(sup_img, qry_img)
        if sup_img.shape[1] != self.shot:
            raise ValueError(f"the model was built for {self.shot} shot(s), got {sup_img.shape[1]}")
        eng = self._engine_for(sup_img.device)
        return eng["pfenet"].lowres(sup_img, sup_mask, qry_img), None

    # -- support banks (pemp_amd.bank.PFENetBank): enroll supports once, segment many queries --------------------------------
    # ``segment`` / ``segment_lowres`` / ``segment_graphed`` are _HeadMixin's, with this family's bank and checks.
    _bank_family = "pfenet"
    _bank_backbone = "resnet50v2"         # the deep-base ResNet-50 (pretrained_weights above)

    @staticmethod
    def _bank_class():
        from ..bank import PFENetBank
        return PFENetBank

    def _bank_desc(self):
        return dict(family=self._bank_family, backbone=self._bank_backbone, precision=self.__dict__.get("_precision", "f32"),
                    S=int(self.shot), C=2048)

    @staticmethod
    def _check_size(H, W, what):
        if H != W:
            raise ValueError(f"{what}: PFENet needs square inputs (its views assume H == W, pfenet.py:204,222,225), got {H}x{W}")
        if (H - 1) % 8 != 0:
            raise ValueError(f"{what}: PFENet needs (H - 1) % 8 == 0 (pfenet.py:164), got H = {H}")

    def _bank_query_check(self, bank, qry_img, what):
        H, W = qry_img.shape[-2:]
        self._check_size(H, W, what)
        hw = pfenet_engine.feat_size(H) ** 2
        if hw != bank.HW:
            raise ValueError(f"{what}: the bank was enrolled at HW = {bank.HW} feature pixels, a {H}x{W} query has {hw}")

    def enroll(self, sup_img, sup_mask, labels=None, out=None, capacity=None):
        """Supports of K classes, ``sup_img`` [K,S,3,H,W] and ``sup_mask`` [K,S,2,H,W] (S = ``self.shot``) -> ``PFENetBank``: one
        supports-only pass through the trunk and the masked layer 4, ``down_supp`` + Weighted GAP, and the pack of the prior's
        support operand (its foreground rows).  ``capacity``: rows per (class, shot) slot, a multiple of 64; default: the largest
        count enrolled, rounded up to 64 (one host read of the counts).  ``out``: enroll into that bank (same K) in place --
        its storage keeps its addresses, so captured graphs that read it see the new classes.  ValueError when a class needs
        more rows than the capacity, before anything is written."""
        from ..bank import PFENetBank
        if out is not None:
            self._check_bank(out, "enroll(out=)")
        self._require_eval_gpu(self, sup_img, sup_mask)
        if sup_img.dim() != 5:
            raise ValueError(f"enroll: sup_img must be [K,S,3,H,W], got {tuple(sup_img.shape)}")
        K, S, ch, H, W = sup_img.shape
        if tuple(sup_mask.shape) != (K, S, 2, H, W):
            raise ValueError(f"enroll: sup_mask must be [{K},{S},2,{H},{W}], got {tuple(sup_mask.shape)}")
        if S != self.shot:
            raise ValueError(f"the model was built for {self.shot} shot(s), got {S}")
        self._check_size(H, W, "enroll")
        fs = pfenet_engine.feat_size(H)
        if out is not None:
            if len(out) != K or not out.rows.is_cuda:
                raise ValueError(f"enroll(out=): the bank holds {len(out)} classes on {out.rows.device}, {K} are enrolled")
            if out.HW != fs * fs:
                raise ValueError(f"enroll(out=): the bank was enrolled at HW = {out.HW} feature pixels, these supports have {fs * fs}")
            if capacity is not None and int(capacity) != out.cap:
                raise ValueError(f"enroll(out=): the bank's capacity is {out.cap}, not {capacity}")
        elif capacity is not None and (int(capacity) < 64 or int(capacity) % 64):
            raise ValueError(f"enroll: capacity must be a positive multiple of 64, got {capacity}")
        eng = self._engine_for(sup_img.device)["pfenet"]
        with torch.no_grad():
            counts = eng.support_counts(sup_mask, (fs, fs)).cpu()              # the one host read: enrolment is off the hot path
            need = int(counts.max())
            cap = out.cap if out is not None else (-(-need // 64) * 64 if capacity is None else int(capacity))
            if need > cap:
                raise ValueError(f"enroll: a class needs {need} rows per shot, the bank's capacity is {cap}")
            if out is None:
                rows, norms, count, svec, hw = eng.enroll_supports(sup_img, sup_mask, cap=cap)
                desc = self._bank_desc()
                return PFENetBank(rows, norms, count, svec, hw, desc["backbone"], desc["precision"], labels=labels, count_host=counts)
            eng.enroll_supports(sup_img, sup_mask, out.rows, out.norms, out.count, out.svec)
            out.count_host.copy_(counts)
        if labels is not None:
            out.labels = PFENetBank._labels(labels, K)
        return out

    def _segment_dev(self, bank, qry_img, index_dev, ret_ind):
        return self._engine_for(qry_img.device)["pfenet"].segment(bank, qry_img, index_dev), None

    def forward(self, sup_img, sup_mask, qry_img, qry_mask=None, out_shape=None):
        """Same contract as the reference's eval forward (pfenet.py:157-287): logits [B,2,Ho,Wo], ``out_shape`` default
        ((H - 1) / 8 * 8 + 1, ...) = (H, W).  ``qry_mask`` is only read by the reference's training loss."""
        if self.training:
            raise NotImplementedError("PFENet is an inference path here: call model.eval() (training is not ported)")
        self.check_inputs(sup_img, qry_img)
        self._require_eval_gpu(self, sup_img, sup_mask, qry_img)
        H, W = sup_img.shape[-2:]
        if out_shape is None:
            out_shape = (int((H - 1) / 8 * self.zoom_factor + 1), int((W - 1) / 8 * self.zoom_factor + 1))
        with torch.no_grad():
            pred, _ = self.lowres(sup_img, sup_mask, qry_img)
            return self._finish(pred, None, tuple(int(v) for v in out_shape))


ModelClass = PFENet
