"""Training step of CANet's head on MI355X: counterpart of ``Trainer.train_step`` in the reference's entry/canet.py:107-116 for
``networks/canet.py`` in ``train()`` mode with ``freeze_backbone = True`` (the reference's setting).

The trunk has the stages [3, 4, 6] only and none of its parameters trains (``maybe_fix_params`` freezes the convs, ``freeze_bn``
the BatchNorms' affine parameters), so only the head has a backward: ``layer5``, ``layer55``, the three pre-activation
residual blocks, the ASPP, ``layer6``, ``layer7``.  The trunk's forward is NOT the inference trunk, though: ``freeze_bn`` only
sets ``requires_grad = False`` (networks/backbones.py:56-62,93-95), the reference never calls ``eval()`` on the encoder, so in a
training step its BatchNorms normalise with the statistics of the batch -- all B(S+1) images -- and move their running
statistics (momentum 0.1); the reference-made fixtures (tests/golden/make_golden_canet_train.py) are reproduced only that way.
The trunk therefore runs on the train-mode conv -> batch-statistics BatchNorm chain of ``train_engine.HeadTrainEngine`` (forward
only, weights packed once), and the per-epoch evaluation sees the moved running statistics, as the reference's does.

Layout (forward as ``canet_engine``):

* ``layer5`` runs over all B(S+1) images, [all supports | all queries], then Dropout2d;
* ``layer55`` = conv over the 256 query channels with ``ops.canet_zterm``'s R as residual.  Backward: weight gradient and
  input gradient of the query half through the conv kernels, the z half through ``train_ops.canet_zterm_bwd`` (tap sums of the
  gradient -> dz, dWz), then ``train_ops.canet_support_vector_bwd`` writes the support rows of layer5's output gradient;
* ``residual_1``'s first conv sees 258 channels (256 features + 2 history): its weight is re-packed every step into a
  288-channel form for the forward conv, its input lives in a 320-channel buffer (channels 258.. zero) that the weight-gradient
  kernel reads whole, and its input gradient uses the first 256 rows of the mirrored weight (the history has no gradient);
* the ASPP + ``layer6`` are ``train_stage2._ASPPNoBN`` (the mixin of the stage-2 engine: same module shapes) with layer6's ReLU;
* ``layer7`` (256 -> 2) is a ``train_engine._Cls2``: forward as a 64-channel padded conv, backward on ``train_ops.canet_cls_bwd``;
* loss: bilinear upsample + CE fused (``ops.eval_tail``), its gradient at the low-resolution logits by
  ``train_ops.upsample_ce_bwd``.

Dropout2d follows stage 2: Philox masks per (image, channel), or given uniforms (``eng.draws``, keyed by the reference's module
names ``layer5.2, layer55.2, aspp_0.2 .. aspp_4.2, layer6.2``, rows in the engine's image order) for the parity tests.
"""
import torch

from . import canet_engine, ops, train_ops as T
from .ops import ConvParams
from .train_engine import HeadTrainEngine, Stage1Trainer, _BN, _Cls2, _Conv, _SliceWgrad, _enqueue_wgrad, check_trunk_precision, conv2d
from .train_stage2 import _ASPPNoBN

MID = canet_engine.MID
HIST_FWD = canet_engine.HIST_CIN        # 288: what the forward conv of residual_1 reads (Cin % 32)
HIST_WGRAD = 320                        # ... and what its weight-gradient kernel reads (Cin % 64); channels 258.. are zero


_FROZEN_TRUNK = ("CANet trunk training (freeze_backbone=False) is not built: the HIP path trains the head behind a frozen trunk, "
                 "as the reference's configuration does")


class CANetHeadTrainEngine(_ASPPNoBN, HeadTrainEngine):
    """Train-mode forward of the frozen trunk, forward + backward of CANet's head; the ASPP is stage 2's."""
    aspp_drop_names = tuple(f"aspp_{i}.2" for i in range(5))

    def __init__(self, model, device, trunk_precision="f32_chain"):
        if not model.freeze_backbone:
            raise ValueError(_FROZEN_TRUNK)
        check_trunk_precision(trunk_precision)
        model.maybe_fix_params()
        super().__init__(model, device, [model.encoder], trunk_precision)
        self.drop_rate2 = float(model.layer5[2].p)
        self.use_history = bool(model.use_history)
        self.w_hist = torch.zeros((MID, 9, HIST_FWD), dtype=torch.float32, device=device) if self.use_history else None
        self.hist_in = {}

    def _init_handles(self, model):
        f, bb = self.flat, model.encoder
        self.stem = (self._frozen_conv(bb.conv1, stem=True), _BN(bb.bn1))
        self.blocks = self._frozen([*bb.layer1, *bb.layer2, *bb.layer3])
        self.f2_block = len(bb.layer1) + len(bb.layer2) - 1               # layer2's last block: the first half of cat((f2, f3))
        self.l5, self.l55 = _Conv(f, model.layer5[0]), _Conv(f, model.layer55[0])
        self.res = [(_Conv(f, seq[1]), _Conv(f, seq[3])) for seq in (model.residual_1, model.residual_2, model.residual_3)]
        self.aspp_conv = [_Conv(f, getattr(model, f"aspp_{i}")[0]) for i in range(5)]
        self.l6, self.l7 = model.layer6[0], _Cls2(f, model.layer7, self.device)
        self.midc = MID

    # -- forward --------------------------------------------------------------------------------
    def _trunk_forward(self, images_list):
        """[n_i,3,H,W] image groups -> cat((f2, f3)) NHWC [n,h,w,1536]; nothing is kept for a backward."""
        torch._foreach_add_(self.bn_counters, 1)                          # every BatchNorm runs exactly once per step
        y, _ = self._cbn_fwd(self._pack(images_list), *self.stem, relu=True)
        x, _ = T.maxpool_idx(y, 3, 2, 1, ceil_mode=True)
        f3, f2 = self._frozen_blocks(x, self.blocks, tap=self.f2_block)
        return torch.cat((f2, f3), dim=3)

    def forward(self, sup_img, sup_mask, qry_img, history=None, slot=None):
        """sup_img [B,S,3,H,W], sup_mask [B,S,2,H,W], qry_img [B,1,3,H,W]; ``history``: None (zeros), [B,2,h,w], or -- with
        ``slot`` int32 [B] -- a table [nslots,2,h,w] read at row slot[b] (< 0: zeros) -> low-resolution logits [B,2,h,w]."""
        f = self.flat
        B, S, _, H, W = sup_img.shape
        ns, n = B * S, B * S + B
        tape = {}
        f.refresh_dgrad_mirror()
        self.rng.begin_step()
        cat23 = self._trunk_forward([sup_img.flatten(0, 1), qry_img.flatten(0, 1)])
        h, w = cat23.shape[1:3]
        self.last_cat23 = cat23
        msk = sup_mask.reshape(ns, 2, H, W).float().contiguous()
        y5 = conv2d(cat23, self.l5.fwd_params(relu=True))
        f5, m5 = self._drop(y5, ("layer5.2",), self.drop_rate2)
        z = ops.canet_support_vector(f5[:ns], msk, S)
        c55 = self.l55
        w55 = f.krsc(c55.conv.weight).view(MID, 9, 2 * MID)
        R = ops.canet_zterm(w55[:, :, MID:].permute(1, 0, 2).contiguous(), z, h, w, c55.dil)
        pq = ConvParams(w55[:, :, :MID].reshape(MID, 9 * MID), None, c55.conv.bias.data, MID, MID, 3, 3, 1, c55.pad, c55.dil, 9 * MID,
                        False, True)
        y55 = conv2d(f5[ns:], pq, residual=R)
        out, m55 = self._drop(y55, ("layer55.2",), self.drop_rate2)
        tape.update(cat23=cat23, y5=y5, m5=m5, f5=f5, msk=msk, z=z, w55=w55, y55=y55, m55=m55, S=S, blocks=[])
        for k, (c1, c2) in enumerate(self.res):
            if k == 0 and self.use_history:
                inp = self.hist_in.get((B, h, w))
                if inp is None:                                           # channels 258.. are zero and stay zero
                    inp = self.hist_in[(B, h, w)] = torch.zeros((B, h, w, HIST_WGRAD), dtype=torch.float32, device=self.device)
                ops.canet_block_input(out, inp, history=history, slot=slot, with_history=True)
                self.w_hist[:, :, :c1.cin].copy_(f.krsc(c1.conv.weight).view(MID, 9, c1.cin))
                p1 = ConvParams(self.w_hist.view(MID, 9 * HIST_FWD), None, c1.conv.bias.data, HIST_FWD, MID, 3, 3, 1, c1.pad, c1.dil,
                                9 * HIST_FWD, False, True)
                t = conv2d(inp[..., :HIST_FWD], p1)
            else:
                inp = ops.canet_block_input(out, self._new(B, h, w, MID))
                t = conv2d(inp, c1.fwd_params(relu=True))
            nxt = conv2d(t, c2.fwd_params(relu=False), residual=out)
            tape["blocks"].append(dict(inp=inp, t=t))
            out = nxt
        y6 = self._aspp_forward(out, tape, out_relu=True)
        x6, m6 = self._drop(y6, ("layer6.2",), self.drop_rate2)
        pred = self.l7.forward(x6, self._new(B, 2, h, w))
        tape.update(y6=y6, m6=m6, x6=x6)
        self.tape = tape
        return pred

    # -- backward -------------------------------------------------------------------------------
    def backward(self, dpred):
        """``dpred`` [B,2,h,w]: the gradient at the low-resolution logits.  Fills the flat gradient buffer."""
        f, tp, ws = self.flat, self.tape, self.ws
        self._begin_backward()
        B, _, h, w = dpred.shape
        # layer7, layer6
        dx6 = self.l7.backward(dpred, tp["x6"], ws)
        g6 = torch.empty_like(dx6)
        T.relu_bias_bwd(self._drop_bwd(dx6, tp["m6"]), tp["y6"], g6, relu=True, want_dbias=False)     # _aspp_backward: layer6's bias
        d = self._aspp_backward(g6)
        # residual blocks, last to first: out_k = out_{k-1} + conv2(relu(conv1(relu(out_{k-1}))))
        for k in (2, 1, 0):
            (c1, c2), rec = self.res[k], tp["blocks"][k]
            c2.conv.bias.grad.copy_((ops.global_avgpool(d) * float(h * w)).sum(dim=0))
            c2.wgrad(rec["t"], d, ws)
            g1 = torch.empty_like(rec["t"])
            T.relu_bias_bwd(conv2d(d, c2.dgrad_params()), rec["t"], g1, relu=True, ws_cache=ws, out=c1.conv.bias.grad)
            inp = rec["inp"]
            if inp.shape[-1] != MID:           # the history block: padded input, 258 live weight channels, no history gradient
                dw1 = f.krsc_grad(c1.conv.weight).view(MID, 9, c1.cin)
                _enqueue_wgrad(f, _SliceWgrad(HIST_WGRAD, MID, [(dw1, slice(c1.cin))], 3, c1.pad, c1.dil), inp, g1, ws)
                wd = f.dgrad_krsc(c1.conv.weight)[:MID]
                dprm = ConvParams(wd, None, None, MID, MID, 3, 3, 1, c1.dil * 2 - c1.pad, c1.dil, wd.shape[1], False, False)
            else:
                c1.wgrad(inp, g1, ws)
                dprm = c1.dgrad_params()
            dprev = torch.empty_like(d)
            T.relu_bias_bwd(conv2d(g1, dprm), inp[..., :MID], dprev, relu=True, want_dbias=False)      # relu(out) > 0 <=> out > 0
            T.relu_bias_bwd(d, None, dprev, add=dprev, relu=False, want_dbias=False)                  # + the skip path
            d = dprev
        # layer55
        c55, S = self.l55, tp["S"]
        ns = B * S
        g55 = torch.empty_like(d)
        T.relu_bias_bwd(self._drop_bwd(d, tp["m55"]), tp["y55"], g55, relu=True, ws_cache=ws, out=c55.conv.bias.grad)
        dw55 = f.krsc_grad(c55.conv.weight).view(MID, 9, 2 * MID)
        fq = tp["f5"][ns:]
        _enqueue_wgrad(f, _SliceWgrad(MID, MID, [(dw55[:, :, :MID], slice(None))], 3, c55.pad, c55.dil), fq, g55, ws)
        df5 = torch.empty_like(tp["f5"])
        wd = f.dgrad_krsc(c55.conv.weight)[:MID]
        conv2d(g55, ConvParams(wd, None, None, MID, MID, 3, 3, 1, c55.dil * 2 - c55.pad, c55.dil, wd.shape[1], False, False),
               out=df5[ns:])
        _, dz = T.canet_zterm_bwd(g55, tp["w55"][:, :, MID:], tp["z"], dw55[:, :, MID:], c55.dil, ws_cache=ws)
        T.canet_support_vector_bwd(dz, tp["msk"], S, df5[:ns])
        # layer5 (weight gradient only: the trunk is frozen)
        g5 = torch.empty_like(df5)
        T.relu_bias_bwd(self._drop_bwd(df5, tp["m5"]), tp["y5"], g5, relu=True, ws_cache=ws, out=self.l5.conv.bias.grad)
        self.l5.wgrad(tp["cat23"], g5, ws)
        f.join_side_stream()
        self.tape = None


class CANetTrainer(Stage1Trainer):
    """``train_step`` of the reference's CANet Trainer (entry/canet.py:107-116): forward, CE on the bilinearly up-sampled logits,
    backward through the head, SGD step without gradient clipping -> (loss, softmax of the low-resolution logits).  Eager only;
    ``query = 1``, any ``shot``."""

    def __init__(self, model, lr=1e-3, momentum=0.9, weight_decay=5e-4, device=None, loss="ce", sigma=5.0, use_graph=False,
                 trunk_precision="f32_chain"):
        self._eager_only(use_graph, "CANet")
        check_trunk_precision(trunk_precision)
        if not model.freeze_backbone:
            raise ValueError(_FROZEN_TRUNK)
        self._setup(model, device, lr, momentum, weight_decay, 0.0, loss, sigma, False)
        self.eng = CANetHeadTrainEngine(model, self.device, trunk_precision)

    def forward_backward(self, sup_img, sup_mask, qry_img, qry_msk, history_mask=None, table=None, read_slot=None):
        """Fills the flat gradient buffer -> (loss, low-resolution logits [B,2,h,w]).  The history: ``history_mask`` [B,1,2,h,w]
        (None: zeros), or row ``read_slot[b]`` (device int32 [B]; < 0: zeros) of a device table [nslots,2,h,w]."""
        eng = self.eng
        self.model.check_inputs(sup_img, qry_img, history_mask)
        hist = slot = None
        if eng.use_history:
            if table is not None:
                hist, slot = table, read_slot
            elif history_mask is not None:
                hist = history_mask.reshape(history_mask.shape[0], *history_mask.shape[-3:]).float().contiguous()
        eng.flat.attach_grads()
        eng.flat.grad.zero_()
        pred = eng.forward(sup_img, sup_mask, qry_img, history=hist, slot=slot)
        tgt = qry_msk.reshape(-1, *qry_msk.shape[-2:]).contiguous()
        loss, _, dpred = self._ce_upsampled(pred, tgt, self.loss_obj.weight_map(tgt))      # (no weight map for plain CE)
        eng.backward(dpred)
        return loss.float(), pred

    def train_step(self, sup_img, sup_mask, qry_img, qry_msk=None, history_mask=None, table=None, read_slot=None, write_slot=None):
        """-> (loss, softmax of the low-resolution logits [B,2,h,w]); with a ``table`` the softmax also goes to its rows
        ``write_slot[b]`` (< 0: nowhere), the later history of those episodes."""
        if history_mask is not None:
            history_mask = history_mask.to(self.device)
        loss, pred = self._step((sup_img, sup_mask, qry_img, qry_msk),
                                lambda *ins: self.forward_backward(*ins, history_mask=history_mask, table=table, read_slot=read_slot))
        prob = ops.canet_history_update(pred, table=table if write_slot is not None else None, slot=write_slot,
                                        out=torch.empty_like(pred))
        return loss, prob

