"""Training step of RPMMs' head on MI355X: counterpart of ``Trainer.train_step`` in the reference's entry/rpmms.py:107-115 for
``networks/rpmms.py:213-311`` in ``train()`` mode -- with ONE deliberate departure: the trunk is frozen.  The reference's
``maybe_fix_params()`` freezes nothing for RPMMs, so its ``train`` also updates ``model_res``'s convs; here every ``model_res``
parameter has ``requires_grad = False`` (``RPMMs.freeze_trunk()``) and only the head has a backward, as in the PFENet and CANet
trainers.  Trunk training is not built.

RPMMs training is not "CANet training three times" (RPMMs head training):

1. Only the query carries a gradient: the EM and the probability maps run under ``no_grad`` in the reference (rpmms.py:73,126),
   so the prototypes and ``Prob_map`` are constants of the step and the support features need no backward.
2. The history carries a gradient: ``Pseudo_mask = out_softmax`` (rpmms.py:250-251) is not detached, so pass p + 1's
   ``residule1`` sends a gradient through its two history channels and the softmax into pass p's logits, where it adds to the
   gradient of pass p's own cross-entropy (``train_ops.rpmms_history_bwd``).  Pass 0's history is zeros and has none.
3. ``layer55``'s Dropout2d is drawn once per prototype: ten [B,256] masks per forward, applied before the sum over a mixture's
   prototypes (``train_ops.rpmms_proto_sum_train``: the eval engine's one conv + tap sums with a multiplier per (image,
   column, channel) inside the sum; its adjoint ``rpmms_proto_sum_bwd`` recomputes the ten pre-activations and never
   materialises ten gradients).  ``layer56.2``, the five ``layer6.aspp_k.2`` and ``layer7.2`` draw once per pass.
4. BatchNorm sees two batches: ``extract_feature_res`` runs on the supports, then on the queries (rpmms.py:222-225), and nobody
   calls ``eval()`` on the trunk: every trunk BatchNorm and the trainable ``layer5[1]`` normalise the B supports with their
   statistics and the B queries with theirs; the running statistics move twice per step, supports first.

The tail (``residule1..3``, ASPP, ``layer7``, ``layer9``) is shared by the three passes: every gradient writer here overwrites
its destination, so after each pass's backward (order 2, 1, 0) the tail's span of the flat gradient buffer is added into an
accumulator, and the sum 2 + 1 + 0 is copied back at the end.

Dropout2d draws for parity tests: ``eng.draws`` keyed by the reference's module names, ``layer55.2`` [10,B,256] (call order =
column order of ``ops.RPMMS_GROUPS``), ``layer56.2`` / ``layer6.aspp_k.2`` / ``layer7.2`` [3,B,256] (by pass)."""
import torch

from . import ops, train_ops as T
from .canet_engine import MID
from .ops import ConvParams
from .rpmms_engine import PASSES
from .train_canet import HIST_FWD, HIST_WGRAD
from .train_engine import HeadTrainEngine, Stage1Trainer, _BN, _Cls2, _Conv, _SliceWgrad, _enqueue_wgrad, check_trunk_precision, conv2d
from .train_stage2 import _ASPPNoBN

_FROZEN_TRUNK = ("RPMMs trunk training is not built: the HIP path trains the head behind a frozen trunk -- call "
                 "model.freeze_trunk() first (a departure from the reference, whose maybe_fix_params() freezes nothing for RPMMs)")


def _check_frozen(model):
    if any(p.requires_grad for p in model.model_res.parameters()):
        raise ValueError(_FROZEN_TRUNK)


class RPMMsHeadTrainEngine(_ASPPNoBN, HeadTrainEngine):
    """Train-mode forward of the frozen trunk (two batches), forward + backward of RPMMs' head; the ASPP is stage 2's."""
    aspp_drop_names = tuple(f"layer6.aspp_{i}.2" for i in range(5))

    def __init__(self, model, device, trunk_precision="f32_chain"):
        _check_frozen(model)
        super().__init__(model, device, [model.model_res], trunk_precision)
        self.drop_rate2 = float(model.layer55[2].p)
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
        self.w_hist, self.w_56 = z(MID, 9, HIST_FWD), z(MID, 9, HIST_FWD)      # 258 live input channels of 288, re-packed per step
        self.w_hd = z(64, 9 * MID)                 # rows 256..257 of residule1.1's mirrored weight, padded to 64 output channels
        self.pad_in, self._pass = {}, 0
        at = {id(p): o for p, o in zip(self.flat.params, self.flat.offs)}
        self.tail_lo = at[id(model.layer6.aspp_0[0].weight)]          # layer6, layer7, layer9, residule1..3: shared by the passes
        if any(at[id(p)] >= self.tail_lo for m in (model.layer5, model.layer55, model.layer56) for p in m.parameters()):
            raise ValueError("RPMMs: the per-pass tail must be the end of the flat parameter layout")

    def _init_handles(self, model):
        f, bb = self.flat, model.model_res
        self.stem = (self._frozen_conv(bb.conv1, stem=True), _BN(bb.bn1))
        self.blocks = self._frozen([*bb.layer1, *bb.layer2, *bb.layer3])
        self.f2_block = len(bb.layer1) + len(bb.layer2) - 1               # layer2's last block: the first half of cat((f2, f3))
        self.l5, self.bn5 = _Conv(f, model.layer5[0]), _BN(model.layer5[1])
        self.l55, self.l56 = _Conv(f, model.layer55[0]), _Conv(f, model.layer56[0])
        self.res = [(_Conv(f, seq[1]), _Conv(f, seq[3])) for seq in (model.residule1, model.residule2, model.residule3)]
        self.aspp_conv = [_Conv(f, getattr(model.layer6, f"aspp_{i}")[0]) for i in range(5)]
        self.l6, self.l9 = model.layer7[0], _Cls2(f, model.layer9, self.device)      # layer7 is what _ASPPNoBN calls its layer6
        self.midc = MID

    def _drop(self, y, layers, p):
        """Given draws come per call of a module ([calls,B,256]); the tail's modules are called once per pass."""
        if self.draws is None or p <= 0.0:
            return super()._drop(y, layers, p)
        saved = self.draws
        self.draws = {k: saved[k][self._pass] for k in layers}
        try:
            return super()._drop(y, layers, p)
        finally:
            self.draws = saved

    def _mask(self, name, rows, p):
        """``rows`` Dropout2d multipliers [rows,256] of module ``name`` in call order (None at rate 0)."""
        if p <= 0.0:
            return None
        u = None
        if self.draws is not None:
            u = self.draws[name]
            if u.numel() != rows * MID or u.dtype != torch.float32 or u.device != self.flat.data.device or not u.is_contiguous():
                raise ValueError(f"dropout2d draws of {name}: want contiguous float32 [{rows // u.shape[1]},{u.shape[1]},{MID}] on {self.device}")
            u = u.view(rows, MID)
        return T.dropout2d_mask(rows, MID, p, self.rng, self.device, uniforms=u)

    def _padded(self, key, *shape):
        """A zero buffer whose padding channels (258..) stay zero: only channels 0..257 are ever written."""
        buf = self.pad_in.get((key, shape))
        if buf is None:
            buf = self.pad_in[(key, shape)] = torch.zeros(shape, dtype=torch.float32, device=self.device)
        return buf

    # -- forward --------------------------------------------------------------------------------
    def _features(self, images, keep):
        """One ``extract_feature_res`` call in train() mode: the trunk and layer5 (conv + bias -> batch-statistics BatchNorm ->
        ReLU) on ONE group of images; every BatchNorm moves its running statistics once.  -> (layer5's output, cat((f2, f3)),
        layer5's tape | None)."""
        torch._foreach_add_(self.bn_counters, 1)
        self.bn5.bn.num_batches_tracked += 1
        y, _ = self._cbn_fwd(self._pack([images]), *self.stem, relu=True)
        x, _ = T.maxpool_idx(y, 3, 2, 1, ceil_mode=True)
        f3, f2 = self._frozen_blocks(x, self.blocks, tap=self.f2_block)
        cat23 = torch.cat((f2, f3), dim=3)
        z = conv2d(cat23, self.l5.fwd_params(relu=False))               # with the bias: the running mean holds it
        bn = self.bn5.bn
        mean, invstd = self.bn5.stats(z, self.ws)
        f5 = T.bn_apply(z, mean, invstd, bn.weight.data, bn.bias.data, torch.empty_like(z), relu=True)
        return f5, cat23, (dict(cat23=cat23, z=z, y=f5, mean=mean, invstd=invstd) if keep else None)

    def forward(self, sup_img, sup_mask, qry_img):
        """sup_img [B,1,3,H,W], sup_mask [B,1,2,H,W], qry_img [B,1,3,H,W] -> [out0, out1, out2], low-resolution logits [B,2,h,w]."""
        f = self.flat
        B, _, _, H, W = sup_img.shape
        f.refresh_dgrad_mirror()
        self.rng.begin_step()
        f5s, cat_s, _ = self._features(sup_img.flatten(0, 1), keep=False)   # supports first, as the reference
        f5q, cat_q, t5 = self._features(qry_img.flatten(0, 1), keep=True)
        self.last_cat23 = (cat_s, cat_q)
        h, w = f5q.shape[1:3]
        # prototypes and probability maps: constants of the step
        fg = sup_mask.reshape(B, 2, H, W)[:, :1].permute(0, 2, 3, 1).float()
        m = ops.resize_bilinear_ac(fg, (h, w), out=self._new(B, h, w, 1))
        self.model.step_pmm_init()
        mu = ops.rpmms_em(f5s, m.view(B, h, w), self.model.pmm_mu0)
        self.last_mu = mu
        # layer55: one conv of the query + the ten prototype columns, one Dropout2d draw per column
        p, c55 = self.drop_rate2, self.l55
        w55 = f.krsc(c55.conv.weight).view(MID, 9, 2 * MID)
        pq = ConvParams(w55[:, :, :MID].reshape(MID, 9 * MID), None, None, MID, MID, 3, 3, 1, c55.pad, c55.dil, 9 * MID, False, False)
        base = conv2d(f5q, pq)
        m55 = self._mask("layer55.2", ops.RPMMS_COLS * B, p)
        mult = (torch.ones((B, ops.RPMMS_COLS, MID), dtype=torch.float32, device=self.device) if m55 is None
                else m55.view(ops.RPMMS_COLS, B, MID).permute(1, 0, 2).contiguous())
        x56 = self._padded("l56", PASSES, B, h, w, HIST_WGRAD)
        _, taps = T.rpmms_proto_sum_train(w55[:, :, MID:].permute(1, 0, 2).contiguous(), mu, base, c55.conv.bias.data, mult, x56[..., :MID],
                                          dil=c55.dil)
        ops.rpmms_prob_map(f5q, mu, x56)
        # layer56: one conv over the 3B images, then ReLU and Dropout2d with one draw per pass
        c56 = self.l56
        self.w_56[:, :, :c56.cin].copy_(f.krsc(c56.conv.weight).view(MID, 9, c56.cin))
        p56 = ConvParams(self.w_56.view(MID, 9 * HIST_FWD), None, c56.conv.bias.data, HIST_FWD, MID, 3, 3, 1, c56.pad, c56.dil, 9 * HIST_FWD,
                         False, True)
        x56n = x56.view(PASSES * B, h, w, HIST_WGRAD)
        y56 = conv2d(x56n[..., :HIST_FWD], p56)
        m56 = self._mask("layer56.2", PASSES * B, p)
        f56 = y56 if m56 is None else T.channel_scale(y56, m56)
        # the three Segmentation passes
        c1 = self.res[0][0]
        self.w_hist[:, :, :c1.cin].copy_(f.krsc(c1.conv.weight).view(MID, 9, c1.cin))
        preds, tapes, hist = [], [], None
        for k in range(PASSES):
            self._pass = k
            pred, tp = self._tail_forward(f56[k * B:(k + 1) * B], hist, k)
            preds.append(pred)
            tapes.append(tp)
            if k + 1 < PASSES:
                hist = ops.canet_history_update(pred, out=torch.empty_like(pred))
        self.tape = dict(t5=t5, f5q=f5q, mu=mu, base=base, mult=mult, taps=taps, x56=x56n, y56=y56, m56=m56, passes=tapes)
        return preds

    def _tail_forward(self, out, hist, k):
        """``Segmentation`` (rpmms.py:271-287) of pass ``k`` on B images; ``hist`` [B,2,h,w]: the softmax of the pass before
        (None: zeros) -> (logits [B,2,h,w], the pass's tape)."""
        B, h, w, _ = out.shape
        tape = dict(hist=hist, blocks=[])
        for j, (c1, c2) in enumerate(self.res):
            if j == 0:
                inp = self._padded(("hist", k), B, h, w, HIST_WGRAD)      # one per pass: the backward reads it
                ops.canet_block_input(out, inp, history=hist, with_history=True)
                p1 = ConvParams(self.w_hist.view(MID, 9 * HIST_FWD), None, c1.conv.bias.data, HIST_FWD, MID, 3, 3, 1, c1.pad, c1.dil,
                                9 * HIST_FWD, False, True)
                t = conv2d(inp[..., :HIST_FWD], p1)
            else:
                inp = ops.canet_block_input(out, self._new(B, h, w, MID))
                t = conv2d(inp, c1.fwd_params(relu=True))
            nxt = conv2d(t, c2.fwd_params(relu=False), residual=out)
            tape["blocks"].append(dict(inp=inp, t=t))
            out = nxt
        y7 = self._aspp_forward(out, tape, out_relu=True)
        x7, m7 = self._drop(y7, ("layer7.2",), self.drop_rate2)
        pred = self.l9.forward(x7, self._new(B, 2, h, w))
        tape.update(y7=y7, m7=m7, x7=x7)
        return pred, tape

    # -- backward -------------------------------------------------------------------------------
    def backward(self, dpreds):
        """``dpreds``: the gradients of the three cross-entropies at their low-resolution logits, [B,2,h,w] each (passes 0 and 1
        receive the history gradient of the pass after them in place).  Fills the flat gradient buffer."""
        f, tp, ws = self.flat, self.tape, self.ws
        self._begin_backward()
        B, _, h, w = dpreds[0].shape
        c1 = self.res[0][0]
        self.w_hd[:2].copy_(f.dgrad_krsc(c1.conv.weight)[MID:MID + 2])              # once per step, behind the mirror's refresh
        df56 = self._new(PASSES * B, h, w, MID)
        tail, acc = f.grad[self.tail_lo:], None
        for k in (2, 1, 0):
            self._pass, self.tape = k, tp["passes"][k]
            self._tail_backward(dpreds[k], dpreds[k - 1] if k else None, df56[k * B:(k + 1) * B])
            # the tail's writers overwrite: add this pass's gradients into the accumulator (2 + 1 + 0), then let the next overwrite
            f.join_side_stream()
            if acc is None:
                acc = tail.clone()
            else:
                acc.add_(tail)
        tail.copy_(acc)
        self.tape = tp
        # layer56 over the 3B images
        c56 = self.l56
        g56 = torch.empty_like(df56)
        T.relu_bias_bwd(self._drop_bwd(df56, tp["m56"]), tp["y56"], g56, relu=True, ws_cache=ws, out=c56.conv.bias.grad)
        dw56 = f.krsc_grad(c56.conv.weight).view(MID, 9, c56.cin)
        _enqueue_wgrad(f, _SliceWgrad(HIST_WGRAD, MID, [(dw56, slice(c56.cin))], 3, c56.pad, c56.dil), tp["x56"], g56, ws)
        wd = f.dgrad_krsc(c56.conv.weight)[:MID]                     # the probability maps have no gradient
        dsum = conv2d(g56, ConvParams(wd, None, None, MID, MID, 3, 3, 1, c56.dil * 2 - c56.pad, c56.dil, wd.shape[1], False, False))
        # layer55: the ten columns' adjoint, then the query half through the conv kernels
        c55 = self.l55
        dw55 = f.krsc_grad(c55.conv.weight).view(MID, 9, 2 * MID)
        dbase, _ = T.rpmms_proto_sum_bwd(dsum.view(PASSES, B, h, w, MID), tp["base"], c55.conv.bias.data, tp["taps"], tp["mult"], dil=c55.dil,
                                         mu=tp["mu"], dw_z=dw55[:, :, MID:], dbias=c55.conv.bias.grad, ws_cache=ws)
        _enqueue_wgrad(f, _SliceWgrad(MID, MID, [(dw55[:, :, :MID], slice(None))], 3, c55.pad, c55.dil), tp["f5q"], dbase, ws)
        wd = f.dgrad_krsc(c55.conv.weight)[:MID]
        df5 = conv2d(dbase, ConvParams(wd, None, None, MID, MID, 3, 3, 1, c55.dil * 2 - c55.pad, c55.dil, wd.shape[1], False, False))
        # layer5, query group only (the supports feed constants); the conv's bias sits in front of a batch-statistics BatchNorm:
        # its gradient is zero and stays the zero the step started from
        t5, bn = tp["t5"], self.bn5
        dz = torch.empty_like(t5["z"])
        T.bn_bwd(df5, t5["y"], t5["z"], t5["mean"], t5["invstd"], bn.bn.weight.data, dz, relu=True, ws_cache=ws, out=bn.grad_out())
        self.l5.wgrad(t5["cat23"], dz, ws)
        f.join_side_stream()
        self.tape = None

    def _tail_backward(self, dpred, dpred_prev, d_in):
        """Backward of one ``Segmentation`` pass (``self.tape``: its tape) -> ``d_in`` [B,h,w,256], the gradient at its input;
        ``dpred_prev`` (None for pass 0) += the history's gradient."""
        f, tp, ws = self.flat, self.tape, self.ws
        B, _, h, w = dpred.shape
        dx7 = self.l9.backward(dpred, tp["x7"], ws)
        g7 = torch.empty_like(dx7)
        T.relu_bias_bwd(self._drop_bwd(dx7, tp["m7"]), tp["y7"], g7, relu=True, want_dbias=False)     # _aspp_backward: layer7's bias
        d = self._aspp_backward(g7)
        # residual blocks, last to first: out_k = out_{k-1} + conv2(relu(conv1(relu(out_{k-1}))))
        for j in (2, 1, 0):
            (c1, c2), rec = self.res[j], tp["blocks"][j]
            c2.conv.bias.grad.copy_((ops.global_avgpool(d) * float(h * w)).sum(dim=0))
            c2.wgrad(rec["t"], d, ws)
            g1 = torch.empty_like(rec["t"])
            T.relu_bias_bwd(conv2d(d, c2.dgrad_params()), rec["t"], g1, relu=True, ws_cache=ws, out=c1.conv.bias.grad)
            inp = rec["inp"]
            if j == 0:                         # the history block: padded input, 258 live weight channels
                dw1 = f.krsc_grad(c1.conv.weight).view(MID, 9, c1.cin)
                _enqueue_wgrad(f, _SliceWgrad(HIST_WGRAD, MID, [(dw1, slice(c1.cin))], 3, c1.pad, c1.dil), inp, g1, ws)
                wd = f.dgrad_krsc(c1.conv.weight)[:MID]
                dprm = ConvParams(wd, None, None, MID, MID, 3, 3, 1, c1.dil * 2 - c1.pad, c1.dil, wd.shape[1], False, False)
                if dpred_prev is not None:     # the history is a softmax (> 0): the block's leading ReLU passes it unchanged
                    dh = conv2d(g1, ConvParams(self.w_hd, None, None, MID, 64, 3, 3, 1, c1.dil * 2 - c1.pad, c1.dil, 9 * MID, False, False))
                    T.rpmms_history_bwd(dh[..., :2], tp["hist"], dpred_prev)
            else:
                c1.wgrad(inp, g1, ws)
                dprm = c1.dgrad_params()
            dprev = d_in if j == 0 else torch.empty_like(d)
            T.relu_bias_bwd(conv2d(g1, dprm), inp[..., :MID], dprev, relu=True, want_dbias=False)      # relu(out) > 0 <=> out > 0
            T.relu_bias_bwd(d, None, dprev, add=dprev, relu=False, want_dbias=False)                  # + the skip path
            d = dprev


class RPMMsTrainer(Stage1Trainer):
    """``train_step`` of the reference's RPMMs Trainer (entry/rpmms.py:107-115) for a FROZEN trunk (module docstring): forward,
    the sum of the three passes' cross-entropies on the bilinearly up-sampled logits, backward through the head, SGD step
    without gradient clipping -> (loss, CE of out2, CE of out1).  Eager only; 1-shot, one query (``model.check_inputs``)."""

    def __init__(self, model, lr=1e-3, momentum=0.9, weight_decay=5e-4, device=None, loss="ce", sigma=5.0, use_graph=False,
                 trunk_precision="f32_chain"):
        self._eager_only(use_graph, "RPMMs")
        _check_frozen(model)
        check_trunk_precision(trunk_precision)
        self._setup(model, device, lr, momentum, weight_decay, 0.0, loss, sigma, False)
        self.eng = RPMMsHeadTrainEngine(model, self.device, trunk_precision)

    def forward_backward(self, sup_img, sup_mask, qry_img, qry_msk):
        """Fills the flat gradient buffer -> (loss, (out0, out1, out2)), the three passes' low-resolution logits [B,2,h,w];
        ``self.last_losses``: the three passes' cross-entropies."""
        eng = self.eng
        self.model.check_inputs(sup_img, qry_img)
        eng.flat.attach_grads()
        eng.flat.grad.zero_()
        preds = eng.forward(sup_img, sup_mask, qry_img)
        tgt = qry_msk.reshape(-1, *qry_msk.shape[-2:]).contiguous()
        wmap = self.loss_obj.weight_map(tgt)                                                   # (no weight map for plain CE)
        ce = [self._ce_upsampled(pred, tgt, wmap) for pred in preds]
        self.last_losses = [c[0].float() for c in ce]
        eng.backward([c[2] for c in ce])
        return self.last_losses[0] + self.last_losses[1] + self.last_losses[2], tuple(preds)

    def train_step(self, sup_img, sup_mask, qry_img, qry_msk=None):
        """-> (loss, loss_p1, loss_p2) as the reference's: the sum, the final pass's cross-entropy, the second pass's."""
        loss, _ = self._step((sup_img, sup_mask, qry_img, qry_msk), self.forward_backward)
        return loss, self.last_losses[2], self.last_losses[1]
