"""RPMMs inference engine (reference: networks/rpmms.py:213-287): CANet's trunk once and CANet's tail three times, behind the
prototype mixture models, as one chain of libpemp_hip.so launches on one stream from a static ``Arena`` (hipGraph capture
works as for the other models).  1-shot, one query (the reference's own limits, rpmms.py:129,266-267).

Layout choices (RPMMs):
- the trunk writes ``cat(layer2, layer3)`` into one [2B,h,w,1536] buffer (supports first), ``layer5`` runs once over it with its
  BatchNorm folded;
- the EM of the three mixtures K = 1 | 3 | 6, foreground and background, is ONE chain of launches over the support features
  (``ops.rpmms_em``): the ten columns share every read of x; the initial mu is the model's ``pmm_mu0`` buffer;
- ``layer55(cat(query, vec_i))`` summed over a mixture's prototypes needs ONE conv of the query with the query half of the
  weights (``base``, shared by the three mixtures); the prototype half is ten 9-tap GEMVs and, per pixel, the taps that fall
  inside the image (``ops.rpmms_proto_sum``; ``ops.canet_zterm``'s trick with the ReLU inside the sum);
- the three ``layer56`` inputs are three [B,h,w,288] buffers (256 sums, P_b, P_f, 30 zero channels: the conv engine takes
  Cin % 32 == 0) behind one another: ``layer56`` is one conv launch over 3B images;
- the three ``Segmentation`` passes are ``canet_engine.CANetTail`` run in order on B images each, the softmax of a pass
  (``ops.canet_history_update``) being the next one's history channels; the reference's ``interpolate`` of the history
  (:274) is the identity at feature size;
- ``layer7`` is the 1280 -> 256 1x1 + ReLU behind the tail-less ASPP: exactly what ``ASPPEngine`` folds as its ``layer6``, and
  ``layer9`` (256 -> 2) is the tail's classifier;
- support banks (``pemp_amd.bank.RPMMsBank``): ``support_side`` runs what depends on the supports alone (trunk, ``layer5``, mask
  resize, EM, tap products) for K classes, ``segment`` the rest for N queries against them -- ``ops.rpmms_bank_l56`` makes
  ``layer56``'s input of every (query, class) pair in one launch, bit for bit the two episode kernels.
"""
import torch

from . import ops
from .canet_engine import HIST_CIN, MID, CANetTail, feature_hw
from .engine import ResNetEngine, conv_params, pack_episode, pack_padded_in

PASSES = 3


class RPMMsEngine:
    """The whole eval forward: ``lowres(sup_img, sup_mask, qry_img)`` -> [out0, out1, out2], logits [B,2,h,w] each."""
    last_aspp_in = property(lambda self: self.tail.last_aspp_in)          # of the last pass

    def __init__(self, model, arena):
        self.arena = arena
        self.model = model
        self.trunk = ResNetEngine(model.model_res, arena)
        self.l5 = conv_params(model.layer5[0], model.layer5[1], relu=True)
        c55 = model.layer55[0]
        self.l55_q = conv_params(c55, None, relu=False, in_slice=(0, MID))
        self.l55_q.shift = None                                   # the bias joins the prototype terms inside the ReLU
        self.b55 = c55.bias.detach().float().contiguous()
        self.wz = ops.pack_canet_zweights(c55.weight[:, MID:])
        self.dil55 = c55.dilation[0]
        self.l56 = pack_padded_in(model.layer56[0], HIST_CIN, True)
        self.tail = CANetTail(arena, (model.residule1, model.residule2, model.residule3), model.layer6, model.layer7[0], model.layer9)

    # lowres() is the support side, the query side and the three passes behind one another on ONE trunk pass over the 2B
    # images; support_side / segment (support banks, pemp_amd.bank.RPMMsBank) run the sides apart, on the same kernels.

    def _layer5(self, groups):
        """Image groups -> layer5 of all of them, NHWC [n,h,w,256]."""
        a = self.arena
        x4 = pack_episode(a, groups)
        n, H, W = x4.shape[:3]
        h, w = feature_hw(H, W)
        cat23 = a.get("rp_cat23", (n, h, w, 1536))
        self.trunk.forward(x4, stage_outs={1: cat23[..., :512], 2: cat23[..., 512:]})
        return ops.conv2d(cat23, self.l5, out=a.get("rp_l5", (n, h, w, MID)))

    def _em(self, f5_s, sup_mask, out):
        """The mask resize and the EM over the supports' layer5 ``f5_s`` [B,h,w,256] -> mu [B,2,10,256] in ``out``."""
        a = self.arena
        B, h, w, _ = f5_s.shape
        H, W = sup_mask.shape[-2:]
        fg = sup_mask.reshape(B, 2, H, W)[:, :1].permute(0, 2, 3, 1)                 # the foreground plane as [B,H,W,1]
        m = ops.resize_bilinear_ac(fg, (h, w), out=a.get("rp_mask", (B, h, w, 1)))
        return ops.rpmms_em(f5_s, m.view(B, h, w), self.model.pmm_mu0, out=out,
                            work=a.get("rp_em_work", (ops.rpmms_em_work_floats(B, h, w, MID),)))

    def _passes(self, x56, key):
        """``layer56`` as one conv over the 3P images of ``x56`` [3,P,h,w,288] and the three ``Segmentation`` passes over P images
        each -> [out0, out1, out2]."""
        a = self.arena
        _, P, h, w, _ = x56.shape
        f56 = ops.conv2d(x56.view(PASSES * P, h, w, HIST_CIN), self.l56, out=a.get("rp_l56", (PASSES * P, h, w, MID)))
        preds, hist = [], None
        for p in range(PASSES):
            preds.append(self.tail.forward(f56[p * P:(p + 1) * P], a.get((key, p), (P, 2, h, w)), hist))
            if p + 1 < PASSES:
                hist = ops.canet_history_update(preds[p], out=a.get("rp_hist", (P, 2, h, w)))
        return preds

    def lowres(self, sup_img, sup_mask, qry_img):
        """sup_img [B,1,3,H,W], sup_mask [B,1,2,H,W] (plane 0: foreground), qry_img [B,1,3,H,W] on the device."""
        a = self.arena
        B = sup_img.shape[0]
        f5 = self._layer5((sup_img.flatten(0, 1), qry_img.flatten(0, 1)))
        h, w = f5.shape[1:3]
        self.last_layer5 = f5
        mu = self._em(f5[:B], sup_mask, a.get("rp_mu", (B, 2, ops.RPMMS_COLS, MID)))
        self.last_mu = mu
        base = ops.conv2d(f5[B:], self.l55_q, out=a.get("rp_base", (B, h, w, MID)))
        x56 = a.get("rp_l56_in", (PASSES, B, h, w, HIST_CIN), zero=True)            # channels 258.. stay zero
        ops.rpmms_proto_sum(self.wz, mu, base, self.b55, x56[..., :MID], dil=self.dil55,
                            taps=a.get("rp_T", (B, ops.RPMMS_COLS, 9, MID)))
        ops.rpmms_prob_map(f5[B:], mu, x56)
        self.last_layer56_in = x56
        return self._passes(x56, "rp_pred")

    def support_side(self, sup_img, sup_mask, mu=None, taps=None):
        """The support side of ``lowres`` for K classes: sup_img [K,1,3,H,W], sup_mask [K,1,2,H,W] -> (mu [K,2,10,256], taps
        [K,10,9,256]): the trunk and ``layer5`` over the K supports, the mask resize, the EM from the model's ``pmm_mu0`` as it
        stands, and the tap products of the foreground prototypes.  Written into the given tensors (a bank's storage) or into
        new ones."""
        K = sup_img.shape[0]
        f5 = self._layer5((sup_img.flatten(0, 1),))
        if mu is None:
            mu = torch.empty((K, 2, ops.RPMMS_COLS, MID), dtype=torch.float32, device=f5.device)
        self._em(f5, sup_mask, mu)
        return mu, ops.rpmms_proto_taps(self.wz, mu, out=taps)

    def segment(self, bank, qry_img, index_dev):
        """The query side of ``lowres`` against an ``RPMMsBank``: qry_img [N,3,H,W]; ``index_dev`` int32 [N] on the device (query n
        meets class index[n]), P = N pairs; None (every query meets every class), P = N * K pairs, pair n * K + k
        -> [out0, out1, out2], logits [P,2,h,w] each.  The trunk, ``layer5`` and ``base`` run once per query."""
        a = self.arena
        N, K = qry_img.shape[0], len(bank)
        P = N if index_dev is not None else N * K
        f5 = self._layer5((qry_img,))
        h, w = f5.shape[1:3]
        base = ops.conv2d(f5, self.l55_q, out=a.get("rp_base", (N, h, w, MID)))
        x56 = a.get("rp_l56_in", (PASSES, P, h, w, HIST_CIN), zero=True)            # channels 258.. stay zero
        ops._rpmms_bank_l56(f5, base, self.b55, bank.mu, bank.taps, x56, index_dev, dil=self.dil55)
        self.last_bank_l56_in = x56
        self.last_bank_passes = self._passes(x56, "rp_bpred")
        return self.last_bank_passes
