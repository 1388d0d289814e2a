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
