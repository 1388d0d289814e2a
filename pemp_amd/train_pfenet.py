"""Training step of PFENet's head on MI355X: counterpart of ``Trainer.train_step`` in the reference's entry/pfenet.py:63-71 for
``networks/pfenet.py`` in ``train()`` mode.

The trunk (``layer0 .. layer4``) runs under ``no_grad`` in the reference (pfenet.py:169-194), so only the head has a backward:
``down_query``, ``down_supp``, the feature enrichment module (``init_merge``, ``alpha_conv``, ``beta_conv``, ``inner_cls``),
``res1``, ``res2`` and ``cls``.  The trunk's forward is NOT the inference trunk, though: ``no_grad`` stops gradients, not
BatchNorm's train mode, and nothing puts the trunk into ``eval()``.  The reference calls it once for the B queries and once per
shot for that shot's B supports; every call normalises with its own batch's statistics and moves the running statistics
(momentum 0.1), in the order query, shot 0, shot 1, ...; ``num_batches_tracked`` grows by S + 1 per step.  ``layer4`` sees
``layer3`` for the queries and ``layer3 * mask`` for a shot.  The trunk therefore runs S + 1 times on the train-mode conv ->
batch-statistics BatchNorm chain of ``train_engine.HeadTrainEngine`` (forward only, weights packed once, no tape), and the per-epoch
evaluation sees the moved running statistics, as the reference's does.

Head layout (forward as ``pfenet_engine.PFENetEngine.lowres``):

* ``down_query`` / ``down_supp`` read ``cat(layer3, layer2)`` [.,h,w,1536]; Dropout2d after each (``down_supp.2`` draws once per
  shot: rows b * S + s of one [B * S, 256] mask);
* the support vector is ``ops.weighted_gap`` (mean over the shots), its adjoint ``train_ops.weighted_gap_bwd``;
* ``init_merge[k]`` sees [query 256 | support 256 | prior 1]: the query and prior columns run as a conv over a 320-channel
  buffer (256 pooled query channels, the prior in channel 256, zeros after; the forward conv reads 288 of them, the
  weight-gradient kernel all 320), the support columns as a per-image shift.  Backward: the weight gradient's columns 0..255
  and 256 go to weight columns 0..255 and 512, the input gradient uses rows 0..255 of the mirrored weight (the prior has no
  gradient), and the support columns of all four bins go through ``train_ops.pfenet_merge_support_bwd`` in one call;
* the four pooled inputs' gradients return to ``down_query``'s output in one ``train_ops.adaptive_avgpool_bwd_multi``;
* ``relu(conv(x)) + x`` (``alpha_conv``, ``beta_conv``, ``res2``): ``relu_bias_bwd`` on the conv branch plus the skip add;
* the bins run backward 3 -> 0: bin k's ``alpha_conv`` input gradient is resized (``train_ops.resize_bilinear_ac_bwd`` with its
  ``add`` operand) onto the ``res1`` input gradient of bin k - 1, which then goes back through bin k - 1's own resize;
* ``cls[3]`` and ``inner_cls[k][3]`` (256 -> 2) run forward as 64-channel padded convs, backward on ``train_ops.canet_cls_bwd``;
* losses: bilinear upsample + CE fused (``ops.eval_tail``), gradients at the low-resolution logits by
  ``train_ops.upsample_ce_bwd``; the auxiliary heads are always plain CE, each scaled by ``loss_coef / 4``.

Dropout2d: Philox masks per (image, channel), or given uniforms (``eng.draws``, keyed by the reference's module names
``down_query.2, down_supp.2, cls.2, inner_cls.0.2 .. inner_cls.3.2``; ``down_supp.2`` rows in the engine's support order
b * S + s) for the parity tests.  ``eng.drop_scale`` = 0 switches every Dropout2d off.
"""
import torch

from . import ops, train_ops as T
from .ops import ConvParams
from .pfenet_engine import MERGE_CIN, PYRAMID_BINS, REDUCE
from .train_engine import HeadTrainEngine, Stage1Trainer, _BN, _Cls2, _Conv, _SliceWgrad, _enqueue_wgrad, check_trunk_precision, conv2d

MERGE_WGRAD = 320                       # what the weight-gradient kernel of init_merge reads (Cin % 64); channels 257.. are zero
TRUNK = ("layer0", "layer1", "layer2", "layer3", "layer4")


class PFENetHeadTrainEngine(HeadTrainEngine):
    """S + 1 train-mode forward passes of the frozen deep-base trunk, forward + backward of PFENet's head."""

    def __init__(self, model, device, trunk_precision="f32_chain"):
        check_trunk_precision(trunk_precision)
        for name in TRUNK:
            for p in getattr(model, name).parameters():
                p.requires_grad = False                                   # the reference's optimizer skips them: their .grad is None
        super().__init__(model, device, [getattr(model, name) for name in TRUNK], trunk_precision)
        self.drop_scale, self.skip_aux = 1.0, False
        self.w_merge = [torch.zeros((REDUCE, MERGE_CIN), dtype=torch.float32, device=device) for _ in self.merge]
        self.merge_in = {}

    def _init_handles(self, model):
        f, l0, device = self.flat, model.layer0, self.device
        self.stem = [(self._frozen_conv(l0[0], stem=True), _BN(l0[1])), (self._frozen_conv(l0[3]), _BN(l0[4])),
                     (self._frozen_conv(l0[6]), _BN(l0[7]))]
        self.blocks = self._frozen([*model.layer1, *model.layer2, *model.layer3])
        self.blocks4 = self._frozen(model.layer4)
        self.f2_block = len(model.layer1) + len(model.layer2) - 1         # layer2's last block: channels 1024.. of cat(layer3, layer2)
        self.down_q, self.down_s = _Conv(f, model.down_query[0]), _Conv(f, model.down_supp[0])
        self.p_down, self.p_cls = float(model.down_query[2].p), float(model.cls[2].p)
        self.merge = [m[0] for m in model.init_merge]
        self.alpha = [_Conv(f, m[0]) for m in model.alpha_conv]
        self.beta = [(_Conv(f, m[0]), _Conv(f, m[2])) for m in model.beta_conv]
        self.inner0 = [_Conv(f, m[0]) for m in model.inner_cls]
        self.inner3 = [_Cls2(f, m[3], device) for m in model.inner_cls]
        self.res1 = _Conv(f, model.res1[0])
        self.res2 = (_Conv(f, model.res2[0]), _Conv(f, model.res2[2]))
        self.cls0, self.cls3 = _Conv(f, model.cls[0]), _Cls2(f, model.cls[3], device)

    # -- forward --------------------------------------------------------------------------------
    def _trunk_pass(self, images, mask=None):
        """One call of layer0 .. layer4 on [n,3,H,W] images with this batch's statistics -> (layer2, layer3, layer4) NHWC;
        ``mask`` [n,h,w]: layer 4 reads layer3 * mask (pfenet.py:193).  Nothing is kept for a backward."""
        torch._foreach_add_(self.bn_counters, 1)                          # every trunk BatchNorm runs once per call
        x = self._pack([images])
        for conv, bn in self.stem:
            x, _ = self._cbn_fwd(x, conv, bn, relu=True)
        x, _ = T.maxpool_idx(x, 3, 2, 1, ceil_mode=False)
        f3, f2 = self._frozen_blocks(x, self.blocks, tap=self.f2_block)
        return f2, f3, self._frozen_blocks(f3 if mask is None else ops.scale_add(f3, mask=mask), self.blocks4)[0]

    def trunk_forward(self, sup_img, sup_mask, qry_img):
        """The S + 1 trunk passes in the reference's order (query, shot 0, shot 1, ...) -> cat(layer3, layer2) of the queries
        [B,h,w,1536] and of the supports [B*S,h,w,1536] (row b * S + s), the support masks at feature resolution [B*S,h,w] and the
        prior [B,h,w]."""
        B, S, _, H, W = sup_img.shape
        ns = B * S
        f2, f3, f4q = self._trunk_pass(qry_img.flatten(0, 1))
        h, w = f3.shape[1:3]
        cat_q = torch.cat((f3, f2), dim=3)
        self.last_layer3, self.last_layer4 = f3, f4q
        fg = sup_mask.reshape(ns, 2, H, W)[:, 0].float().unsqueeze(-1)
        mfeat = ops.resize_bilinear_ac(fg, (h, w), out=self._new(ns, h, w, 1), binarize=True).view(ns, h, w)
        cat_s, f4s = self._new(ns, h, w, 1536), self._new(ns, h, w, f4q.shape[3])
        for s in range(S):
            f2, f3, f4 = self._trunk_pass(sup_img[:, s], mask=mfeat[s::S].contiguous())
            cat_s[s::S, ..., :1024] = f3
            cat_s[s::S, ..., 1024:] = f2
            f4s[s::S] = f4
        prior = ops.prior_mask(f4q, f4s, mfeat, S, ws_cache=self.ws)
        self.last_head_inputs = (cat_q, cat_s, mfeat, prior)
        return self.last_head_inputs

    def head_forward(self, cat_q, cat_s, mfeat, prior, S):
        """-> (low-resolution logits [B,2,h,w], the four inner logits [B,2,bin,bin]); keeps the tape for ``backward``."""
        f = self.flat
        B, h, w, _ = cat_q.shape
        f.refresh_dgrad_mirror()
        self.rng.begin_step()
        yq = conv2d(cat_q, self.down_q.fwd_params(relu=True))
        dq, mq = self._drop(yq, ("down_query.2",), self.p_down * self.drop_scale)
        ys = conv2d(cat_s, self.down_s.fwd_params(relu=True))
        ds, ms = self._drop(ys, ("down_supp.2",), self.p_down * self.drop_scale)
        svec = ops.weighted_gap(ds, mfeat, S)
        self.last_supp_vec = svec
        tape = dict(cat_q=cat_q, cat_s=cat_s, mfeat=mfeat, S=S, yq=yq, mq=mq, ys=ys, ms=ms, svec=svec, bins=[])
        res1_in = self._new(B, h, w, REDUCE * len(PYRAMID_BINS))
        inner = []
        for idx, bn in enumerate(PYRAMID_BINS):
            inp = self.merge_in.get((idx, B))
            if inp is None:                                               # channels 257.. are zero and stay zero
                inp = self.merge_in[(idx, B)] = torch.zeros((B, bn, bn, MERGE_WGRAD), dtype=torch.float32, device=self.device)
            ops.adaptive_avgpool(dq, bn, out=inp[..., :REDUCE])
            ops.resize_bilinear_ac(prior.unsqueeze(-1), bn, out=inp[..., REDUCE:REDUCE + 1])
            if idx == 0:
                self.last_prior_bin0 = inp[..., REDUCE]
            wm = f.krsc(self.merge[idx].weight)                           # [256, 513]: query | support | prior
            self.w_merge[idx][:, :REDUCE].copy_(wm[:, :REDUCE])
            self.w_merge[idx][:, REDUCE].copy_(wm[:, 2 * REDUCE])
            ws_k = wm[:, REDUCE:2 * REDUCE].contiguous()
            shift = conv2d(svec.view(B, 1, 1, REDUCE), ConvParams(ws_k, None, None, REDUCE, REDUCE, 1, 1, 1, 0, 1, REDUCE, False, False))
            rec = self._new(B, bn, bn, 2 * REDUCE)
            m0 = conv2d(inp[..., :MERGE_CIN], ConvParams(self.w_merge[idx], None, None, MERGE_CIN, REDUCE, 1, 1, 1, 0, 1, MERGE_CIN,
                                                        False, True),
                        out=rec[..., :REDUCE], shift_override=shift.view(B, REDUCE), per_image_shift=True)
            r = dict(inp=inp, m0=m0)
            if idx >= 1:
                ops.resize_bilinear_ac(res1_in[..., (idx - 1) * REDUCE:idx * REDUCE], bn, out=rec[..., REDUCE:])
                t = conv2d(rec, self.alpha[idx - 1].fwd_params(relu=True))
                m2 = ops.scale_add(t, residual=m0)
                r.update(rec=rec, t=t)
            else:
                m2 = m0
            b0, b1 = self.beta[idx]
            t1 = conv2d(m2, b0.fwd_params(relu=True))
            t2 = conv2d(t1, b1.fwd_params(relu=True))
            m3 = ops.scale_add(t2, residual=m2)
            r.update(m2=m2, t1=t1, t2=t2, m3=m3)
            if not self.skip_aux:
                i0 = conv2d(m3, self.inner0[idx].fwd_params(relu=True))
                i0d, mi = self._drop(i0, (f"inner_cls.{idx}.2",), self.p_cls * self.drop_scale)
                inner.append(self.inner3[idx].forward(i0d, self._new(B, 2, bn, bn)))
                r.update(i0=i0, mi=mi, i0d=i0d)
            ops.resize_bilinear_ac(m3, (h, w), out=res1_in[..., idx * REDUCE:(idx + 1) * REDUCE])
            tape["bins"].append(r)
        q1 = conv2d(res1_in, self.res1.fwd_params(relu=True))
        r0 = conv2d(q1, self.res2[0].fwd_params(relu=True))
        r1 = conv2d(r0, self.res2[1].fwd_params(relu=True))
        q2 = ops.scale_add(r1, residual=q1)
        c0 = conv2d(q2, self.cls0.fwd_params(relu=True))
        c0d, mc = self._drop(c0, ("cls.2",), self.p_cls * self.drop_scale)
        pred = self.cls3.forward(c0d, self._new(B, 2, h, w))
        tape.update(res1_in=res1_in, q1=q1, r0=r0, r1=r1, q2=q2, c0=c0, mc=mc, c0d=c0d)
        self.tape = tape
        return pred, inner

    def forward(self, sup_img, sup_mask, qry_img):
        """sup_img [B,S,3,H,W], sup_mask [B,S,2,H,W], qry_img [B,1,3,H,W] -> (low-resolution logits, inner logits)."""
        S = sup_img.shape[1]
        return self.head_forward(*self.trunk_forward(sup_img, sup_mask, qry_img), S)

    # -- backward -------------------------------------------------------------------------------
    def backward(self, dpred, dinner):
        """``dpred`` [B,2,h,w] and ``dinner`` (four [B,2,bin,bin], or None with ``skip_aux``): the gradients at the low-resolution
        logits of ``cls`` and of the ``inner_cls`` heads.  Fills the flat gradient buffer."""
        f, tp, ws = self.flat, self.tape, self.ws
        self._begin_backward()
        B, _, h, w = dpred.shape
        new = lambda t: torch.empty(t.shape, dtype=torch.float32, device=self.device)

        def relu_bwd(dy, y, add=None):         # (dy (+ add)) * (y > 0): the head's convs in front of a ReLU have no bias
            g = new(y)
            T.relu_bias_bwd(dy, y, g, add=add, relu=True, want_dbias=False)
            return g

        def conv_bwd(c, x, g, residual=None):  # weight gradient (side stream) and input gradient (+ residual) of conv c
            c.wgrad(x, g, ws)
            return conv2d(g, c.dgrad_params(), residual=residual)

        # cls, res2, res1
        g = relu_bwd(self._drop_bwd(self.cls3.backward(dpred, tp["c0d"], ws), tp["mc"]), tp["c0"])
        dq2 = conv_bwd(self.cls0, tp["q2"], g)
        dr0 = conv_bwd(self.res2[1], tp["r0"], relu_bwd(dq2, tp["r1"]))
        dq1 = conv_bwd(self.res2[0], tp["q1"], relu_bwd(dr0, tp["r0"]), residual=dq2)                # + the skip path
        dres1 = conv_bwd(self.res1, tp["res1_in"], relu_bwd(dq1, tp["q1"]))                          # [B,h,w,1024]
        # the FEM, last bin first: bin idx's alpha_conv input gradient lands on bin idx - 1's slice of dres1
        g0s, gqs = [None] * len(PYRAMID_BINS), [None] * len(PYRAMID_BINS)
        for idx in range(len(PYRAMID_BINS) - 1, -1, -1):
            r, bn = tp["bins"][idx], PYRAMID_BINS[idx]
            dm3 = T.resize_bilinear_ac_bwd(dres1[..., idx * REDUCE:(idx + 1) * REDUCE], size=bn)
            if dinner is not None:
                g = relu_bwd(self._drop_bwd(self.inner3[idx].backward(dinner[idx], r["i0d"], ws), r["mi"]), r["i0"])
                dm3 = conv_bwd(self.inner0[idx], r["m3"], g, residual=dm3)
            b0, b1 = self.beta[idx]
            dt1 = conv_bwd(b1, r["t1"], relu_bwd(dm3, r["t2"]))
            dm2 = conv_bwd(b0, r["m2"], relu_bwd(dt1, r["t1"]), residual=dm3)
            if idx >= 1:
                drec = conv_bwd(self.alpha[idx - 1], r["rec"], relu_bwd(dm2, r["t"]))                # [B,bin,bin,512]
                prev = dres1[..., (idx - 1) * REDUCE:idx * REDUCE]
                T.resize_bilinear_ac_bwd(drec[..., REDUCE:], add=prev, out=prev)
                g0 = relu_bwd(drec[..., :REDUCE], r["m0"], add=dm2)
            else:
                g0 = relu_bwd(dm2, r["m0"])
            g0s[idx] = g0
            wconv = self.merge[idx].weight
            dw = f.krsc_grad(wconv)                                       # [256, 513]: query | support | prior
            copies = [(dw[:, :REDUCE], slice(REDUCE)), (dw[:, 2 * REDUCE], REDUCE)]      # from columns 0..255 and 256 of the dense gradient
            _enqueue_wgrad(f, _SliceWgrad(MERGE_WGRAD, REDUCE, copies), r["inp"], g0, ws)
            wd = f.dgrad_krsc(wconv)[:REDUCE]                             # rows 0..255 of the mirrored weight: the query channels
            gqs[idx] = conv2d(g0, ConvParams(wd, None, None, REDUCE, REDUCE, 1, 1, 1, 0, 1, wd.shape[1], False, False))
        # support vector and down_supp (weight gradient only: the trunk is frozen)
        wms, dwms = [f.krsc(m.weight)[:, REDUCE:2 * REDUCE] for m in self.merge], [f.krsc_grad(m.weight)[:, REDUCE:2 * REDUCE] for m in self.merge]
        dsvec = T.pfenet_merge_support_bwd(g0s, wms, tp["svec"], dwms, ws_cache=ws)
        dds = T.weighted_gap_bwd(dsvec, tp["mfeat"], tp["S"], new(tp["ys"]))
        self.down_s.wgrad(tp["cat_s"], relu_bwd(self._drop_bwd(dds, tp["ms"]), tp["ys"]), ws)
        # down_query
        ddq = T.adaptive_avgpool_bwd_multi(gqs, new(tp["yq"]))
        self.down_q.wgrad(tp["cat_q"], relu_bwd(self._drop_bwd(ddq, tp["mq"]), tp["yq"]), ws)
        f.join_side_stream()
        self.tape = None


class PFENetTrainer(Stage1Trainer):
    """``train_step`` of the reference's PFENet Trainer (entry/pfenet.py:63-71): forward, ``loss = CE(out, y)``, ``loss + aux_loss *
    loss_coef`` backward through the head, SGD step without gradient clipping -> (loss, aux_loss).  Eager only; ``query = 1``, any
    ``shot``.  ``loss = cedt`` weights the main loss only: the auxiliary loss is the model's own plain CE (pfenet.py:59,282)."""

    def __init__(self, model, lr=1e-3, momentum=0.9, weight_decay=5e-4, device=None, loss="ce", sigma=5.0, loss_coef=1.0,
                 use_graph=False, trunk_precision="f32_chain"):
        self._eager_only(use_graph, "PFENet")
        check_trunk_precision(trunk_precision)
        self._setup(model, device, lr, momentum, weight_decay, 0.0, loss, sigma, False)
        self.eng = PFENetHeadTrainEngine(model, self.device, trunk_precision)
        self.loss_coef = float(loss_coef)

    def losses_backward(self, pred, inner, tgt):
        """Main and auxiliary loss of given logits and their backward through the head -> (loss, aux_loss)."""
        eng = self.eng
        loss, _, dpred = self._ce_upsampled(pred, tgt, self.loss_obj.weight_map(tgt))      # (no weight map for plain CE)
        aux, dinner = torch.zeros((), dtype=torch.float64, device=pred.device), None
        if inner:
            dinner = []
            for lg in inner:                                      # always nn.CrossEntropyLoss(ignore_index=255), mean over the heads
                ce, _, d = self._ce_upsampled(lg, tgt)
                aux = aux + ce
                dinner.append(d.mul_(self.loss_coef / len(inner)))
            aux = aux / len(inner)
        eng.backward(dpred, dinner)
        return loss.float(), aux.float()

    def forward_backward(self, sup_img, sup_mask, qry_img, qry_msk):
        """Fills the flat gradient buffer -> (loss, aux_loss, low-resolution logits [B,2,h,w])."""
        eng = self.eng
        self.model.check_inputs(sup_img, qry_img)
        if sup_img.shape[1] != self.model.shot:
            raise ValueError(f"the model was built for {self.model.shot} shot(s), got {sup_img.shape[1]}")
        eng.flat.attach_grads()
        eng.flat.grad.zero_()
        pred, inner = eng.forward(sup_img, sup_mask, qry_img)
        self.last_inner = inner
        tgt = qry_msk.reshape(-1, *qry_msk.shape[-2:]).contiguous()
        loss, aux = self.losses_backward(pred, inner, tgt)
        return loss, aux, pred

    def train_step(self, sup_img, sup_mask, qry_img, qry_msk=None):
        return self._step((sup_img, sup_mask, qry_img, qry_msk), self.forward_backward)[:2]
