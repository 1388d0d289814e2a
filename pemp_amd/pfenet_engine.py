"""PFENet inference engine (reference: networks/pfenet.py:157-274, networks/pfe_resent.py:97-160): the deep-base dilated
ResNet-50 trunk to layer 4, the prior mask and the feature enrichment module (FEM), as one chain of libpemp_hip.so launches
on one stream from a static ``Arena`` (hipGraph capture works as for the other models).

Layout choices:
- layer 2's output is written into channels 1024..1535 and layer 3's into 0..1023 of one [n,h,w,1536] buffer: the
  ``cat([feat_3, feat_2])`` of the 1x1 ``down_query`` / ``down_supp`` convs (:175,195) is never formed;
- layer 4 runs once over supports and queries: its input is layer 3 times the support mask (:193), the queries' rows
  times 1 (exact);
- ``init_merge`` sees [query 256 | support 256 | prior 1] (:251): the support channels are constant over space, so their
  1x1 conv is a per-image shift (CONV_SHIFT_PER_IMAGE); the prior is zero-padded into the conv's K (channel 256 of a
  288-channel input, channels 257..287 zero: the conv engine takes Cin % 32 == 0);
- ``relu(conv(.)) + x`` (:261,264,270) runs as the conv with its ReLU, then ``ops.scale_add``: the conv engine's residual
  epilogue computes relu(conv + x), which is not the same function;
- the 256 -> 2 classifier conv is packed with 62 zero output channels (Cout % 64), its two live channels resized into the
  [B,2,h,w] logits in one pass;
- ``inner_cls`` (:266) feeds only the training loss (:276-285): not run.

Support banks (``pemp_amd.bank.PFENetBank``): everything the supports contribute -- their trunk passes, the masked layer 4,
``down_supp`` + Weighted GAP and the masked, normalised support operand of the prior GEMM -- depends on them alone.
``enroll_supports`` runs that side once and packs the prior operand (foreground rows only); ``segment`` runs the query side
against the bank.  Both make the launches ``lowres`` makes on the same rows, so the results agree with it bit for bit.
"""
import torch

from . import ops
from .engine import _BlockPlan, _BottleneckTrunk, classifier2, conv_params, logits_nchw, pack_episode, with_split3
from .ops import ConvParams

PYRAMID_BINS = (60, 30, 15, 8)
REDUCE = 256
MERGE_CIN = REDUCE + 32                 # query channels + the prior channel, zero-padded to a multiple of 32


def feat_size(H):
    """Side of the layer-2 .. layer-4 maps for an H x H input: the stem's stride-2 conv, the max-pool, layer 2's stride."""
    for _ in range(3):
        H = ops.conv_out_size(H, 3, 2, 1, 1)
    return H


class DeepBaseResNetEngine(_BottleneckTrunk):
    """pfe_resent.ResNet(Bottleneck, [3, 4, 6, 3], deep_base=True) with PFENet's dilations (pfenet.py:68-77): a three-conv stem, a
    max-pool without ceil_mode and v1.5 bottlenecks (the stride sits on the 3x3 conv; layer 3 / 4 dilated with stride 1)."""
    PRESPLIT = False
    GROUP_DS = False                    # see _BottleneckTrunk: grouping conv1 with the downsample conv would change PFENet's speed

    def __init__(self, model, arena):
        self.arena = arena
        l0 = model.layer0
        self.stem = [conv_params(l0[0], l0[1], relu=True, stem4=True), conv_params(l0[3], l0[4], relu=True),
                     conv_params(l0[6], l0[7], relu=True)]
        self.stages = [[_BlockPlan(b) for b in getattr(model, f"layer{i}")] for i in (1, 2, 3, 4)]

    def forward_to_layer3(self, x4):
        """x4 NHWC4 [n,H,W,4] -> [n,h,w,1536]: layer 3 in channels 0..1023, layer 2 in 1024..1535."""
        a = self.arena
        n, H, W, _ = x4.shape
        x = x4
        for i, cp in enumerate(self.stem):
            h, w = x.shape[1:3]
            ho, wo = ops.conv_out_size(h, 3, cp.stride, cp.pad, 1), ops.conv_out_size(w, 3, cp.stride, cp.pad, 1)
            x = ops.conv2d(x, cp, out=a.get(("pf_stem", i & 1), (n, ho, wo, cp.cout)))
        h, w = x.shape[1:3]
        hp, wp = ops._pool_out(h, 3, 2, 1, False), ops._pool_out(w, 3, 2, 1, False)      # MaxPool2d(3, 2, 1), no ceil_mode
        x = ops.maxpool2d(x, 3, 2, 1, out=a.get("pf_pool", (n, hp, wp, x.shape[3])))
        x = self._stage(x, 0)
        h2 = ops.conv_out_size(x.shape[1], 3, 2, 1, 1)
        w2 = ops.conv_out_size(x.shape[2], 3, 2, 1, 1)
        cat = a.get("pf_cat23", (n, h2, w2, 1536))
        f2 = self._stage(x, 1, final_out=cat[..., 1024:])
        self._stage(f2, 2, final_out=cat[..., :1024])
        return cat

    def layer4(self, x, out):
        return self._stage(x, 3, final_out=out)


class PFENetEngine:
    """The whole eval forward: ``lowres(sup_img, sup_mask, qry_img)`` -> logits [B,2,h,w] at feature resolution."""

    def __init__(self, model, arena):
        self.arena = arena
        self.trunk = DeepBaseResNetEngine(model, arena)
        self.down_q = conv_params(model.down_query[0], None, relu=True)
        self.down_s = conv_params(model.down_supp[0], None, relu=True)
        self.merge, self.merge_s = [], []
        for m in model.init_merge:
            conv = m[0]
            w = conv.weight.detach().float()[:, :, 0, 0]                        # [256, 513]: query | support | prior
            wq = torch.zeros((REDUCE, MERGE_CIN), dtype=torch.float32, device=w.device)
            wq[:, :REDUCE] = w[:, :REDUCE]
            wq[:, REDUCE] = w[:, 2 * REDUCE]
            self.merge.append(with_split3(ConvParams(wq.contiguous(), None, None, MERGE_CIN, REDUCE, 1, 1, 1, 0, 1, MERGE_CIN,
                                                     False, True)))
            self.merge_s.append(conv_params(conv, None, relu=False, in_slice=(REDUCE, 2 * REDUCE)))
        self.alpha = [conv_params(m[0], None, relu=True) for m in model.alpha_conv]
        self.beta = [(conv_params(m[0], None, relu=True), conv_params(m[2], None, relu=True)) for m in model.beta_conv]
        self.res1 = conv_params(model.res1[0], None, relu=True)
        self.res2 = (conv_params(model.res2[0], None, relu=True), conv_params(model.res2[2], None, relu=True))
        self.cls0 = conv_params(model.cls[0], None, relu=True)
        self.cls3 = classifier2(model.cls[3])
        self._ones = set()

    # lowres() is three stages, each of them the same launches whether an episode's supports and queries pass together
    # (lowres) or apart (enroll_supports / segment: support banks, pemp_amd.bank.PFENetBank): _layer4 (trunk, mask resize,
    # masked layer 4) on any mix of ns supports and nq queries, _support_vector, and _tail (down_query + FEM + classifier).

    def _layer4(self, groups, sup_mask, ns):
        """``groups``: image groups (the ns supports first) -> (cat23 [n,h,w,1536], mfeat [n,h,w], f4 [n,h,w,2048])."""
        a = self.arena
        x4 = pack_episode(a, groups)
        n, H, W = x4.shape[:3]
        cat23 = self.trunk.forward_to_layer3(x4)                                 # [n,h,w,1536]
        h, w = cat23.shape[1:3]
        # support masks at feature resolution (:182-185, == 1 then bilinear align_corners), the queries' rows = 1
        mfeat = a.get(("pf_mfeat", ns), (n, h, w))
        if mfeat.data_ptr() not in self._ones:
            mfeat[ns:].fill_(1.0)
            self._ones.add(mfeat.data_ptr())
        if ns:
            fg = sup_mask.reshape(ns, 2, H, W)[:, 0].unsqueeze(-1)
            ops.resize_bilinear_ac(fg, (h, w), out=mfeat[:ns].unsqueeze(-1), binarize=True)
        # layer 4 over layer3 * mask (:193; the queries' layer 4 of :171 is the same chain on their unmasked rows)
        x4in = ops.scale_add(cat23[..., :1024], mask=mfeat, out=a.get("pf_l4in", (n, h, w, 1024)))
        f4 = self.trunk.layer4(x4in, a.get("pf_l4", (n, h, w, 2048)))
        return cat23, mfeat, f4

    def _support_vector(self, cat23_s, mfeat_s, S, out):
        """down_supp (:195-196) and the Weighted-GAP support vector (:197,229-233) of ns = B * S supports -> ``out`` [B,256]."""
        ns, h, w = mfeat_s.shape
        dsup = ops.conv2d(cat23_s, self.down_s, out=self.arena.get("pf_ds", (ns, h, w, REDUCE)))
        return ops.weighted_gap(dsup, mfeat_s, S, out=out)

    def lowres(self, sup_img, sup_mask, qry_img):
        """sup_img [B,S,3,H,W], sup_mask [B,S,2,H,W] (plane 0: foreground), qry_img [B,1,3,H,W] on the device."""
        a = self.arena
        B, S = sup_img.shape[:2]
        ns = B * S
        cat23, mfeat, f4 = self._layer4((sup_img.flatten(0, 1), qry_img.flatten(0, 1)), sup_mask, ns)
        h, w = cat23.shape[1:3]
        self.last_layer4 = f4
        prior = ops.prior_mask(f4[ns:], f4[:ns], mfeat[:ns], S, out=a.get("pf_prior", (B, h, w)), ws_cache=a.ws)
        self.last_prior = prior
        # down_query (:175-176) comes first in _tail; down_supp and the support vector after it, as ever
        dq = ops.conv2d(cat23[ns:], self.down_q, out=a.get("pf_dq", (B, h, w, REDUCE)))
        svec = self._support_vector(cat23[:ns], mfeat[:ns], S, a.get("pf_svec", (B, REDUCE)))
        self.last_supp_vec = svec
        return self._tail(dq, prior, svec, 1)

    def enroll_supports(self, sup_img, sup_mask, rows=None, norms=None, count=None, svec=None, cap=None):
        """The support side of ``lowres`` for K classes: sup_img [K,S,3,H,W], sup_mask [K,S,2,H,W] -> (rows, norms, count, svec,
        HW): the packed prior operand (``ops.prior_bank_pack``) and the support vectors [K,256], written into the given
        tensors (a bank's storage) or into new ones with ``cap`` rows per slot.  The caller has made sure that every class fits
        (``support_counts``)."""
        K, S = sup_img.shape[:2]
        cat23, mfeat, f4 = self._layer4((sup_img.flatten(0, 1),), sup_mask, K * S)
        if svec is None:
            svec = torch.empty((K, REDUCE), dtype=torch.float32, device=f4.device)
        self._support_vector(cat23, mfeat, S, svec)
        rows, norms, count = ops.prior_bank_pack(f4, mfeat, K, S, cap=cap, rows=rows, norms=norms, count=count)
        return rows, norms, count, svec, f4.shape[1] * f4.shape[2]

    def support_counts(self, sup_mask, feat_hw):
        """Rows every (class, shot) needs in a bank slot, before anything else runs: sup_mask [K,S,2,H,W] -> int32 [K,S] (device)."""
        K, S, _, H, W = sup_mask.shape
        mfeat = self.arena.get(("pf_mcount", K * S), (K * S,) + tuple(feat_hw))
        ops.resize_bilinear_ac(sup_mask.reshape(K * S, 2, H, W)[:, 0].unsqueeze(-1), tuple(feat_hw), out=mfeat.unsqueeze(-1),
                               binarize=True)
        return ops.prior_bank_count(mfeat, K, S)

    def segment(self, bank, qry_img, index_dev):
        """The query side of ``lowres`` against a ``PFENetBank``: qry_img [N,3,H,W]; ``index_dev`` int32 [N] on the device
        (query n meets class index[n]) -> logits [N,2,h,w]; None (every query meets every class) -> [N,K,2,h,w]."""
        a = self.arena
        N, K = qry_img.shape[0], len(bank)
        cat23, _, f4 = self._layer4((qry_img,), None, 0)
        h, w = cat23.shape[1:3]
        lead = (N,) if index_dev is not None else (N, K)
        prior = ops._prior_bank(f4, bank.rows, bank.norms, bank.count, index_dev, out=a.get("pf_bprior", lead + (h, w)), ws_cache=a.ws)
        self.last_bank_prior = prior
        dq = ops.conv2d(cat23, self.down_q, out=a.get("pf_dq", (N, h, w, REDUCE)))
        svec = ops.bank_gather_rows(bank.svec, index_dev, N, out=a.get("pf_bsvec", lead + (REDUCE,)))
        rep = 1 if index_dev is not None else K
        pred = self._tail(dq, prior.view(N * rep, h, w), svec.view(N * rep, REDUCE), rep)
        return pred.view(lead + tuple(pred.shape[1:]))

    def _tail(self, dq, prior, svec, rep):
        """The FEM (:238-268) and the classifier over P = N * rep (query, class) pairs: dq [N,h,w,256] (down_query, per query),
        prior [P,h,w], svec [P,256], pair n * rep + k = query n.  What depends on the query alone -- the four adaptive pools of
        dq -- runs once per query; rep > 1 copies it to the query's pairs."""
        a = self.arena
        N, h, w, _ = dq.shape
        B = N * rep
        res1_in = a.get("pf_res1_in", (B, h, w, REDUCE * len(PYRAMID_BINS)))
        self.last_bins = []
        for idx, bn in enumerate(PYRAMID_BINS):                                  # FEM (:238-268)
            inp = a.get(("pf_mrg_in", idx), (B, bn, bn, MERGE_CIN), zero=True)  # channels 257.. stay zero
            if rep == 1:
                ops.adaptive_avgpool(dq, bn, out=inp[..., :REDUCE])
            else:
                pooled = ops.adaptive_avgpool(dq, bn, out=a.get(("pf_dqpool", idx), (N, bn, bn, REDUCE)))
                per_query = inp.view(N, rep, bn, bn, MERGE_CIN)
                for k in range(rep):                                             # identity resize: an exact strided copy
                    ops.resize_bilinear_ac(pooled, bn, out=per_query[:, k, :, :, :REDUCE])
            ops.resize_bilinear_ac(prior.unsqueeze(-1), bn, out=inp[..., REDUCE:REDUCE + 1])
            self.last_bins.append(inp[..., REDUCE])
            shift = ops.conv2d(svec.view(B, 1, 1, REDUCE), self.merge_s[idx], out=a.get(("pf_mrg_s", idx), (B, 1, 1, REDUCE)))
            rec = a.get(("pf_rec", idx), (B, bn, bn, 2 * REDUCE))
            merge = ops.conv2d(inp, self.merge[idx], out=rec[..., :REDUCE], shift_override=shift.view(B, REDUCE),
                               per_image_shift=True)
            if idx >= 1:
                prev = res1_in[..., (idx - 1) * REDUCE:idx * REDUCE]
                ops.resize_bilinear_ac(prev, bn, out=rec[..., REDUCE:])
                t = ops.conv2d(rec, self.alpha[idx - 1], out=a.get(("pf_t", idx), (B, bn, bn, REDUCE)))
                merge = ops.scale_add(t, residual=merge, out=a.get(("pf_m2", idx), (B, bn, bn, REDUCE)))
            b0, b1 = self.beta[idx]
            t1 = ops.conv2d(merge, b0, out=a.get(("pf_b0", idx), (B, bn, bn, REDUCE)))
            t2 = ops.conv2d(t1, b1, out=a.get(("pf_b1", idx), (B, bn, bn, REDUCE)))
            merge = ops.scale_add(t2, residual=merge, out=a.get(("pf_m3", idx), (B, bn, bn, REDUCE)))
            ops.resize_bilinear_ac(merge, (h, w), out=res1_in[..., idx * REDUCE:(idx + 1) * REDUCE])
        self.last_res1_in = res1_in
        q1 = ops.conv2d(res1_in, self.res1, out=a.get("pf_q1", (B, h, w, REDUCE)))
        r = ops.conv2d(q1, self.res2[0], out=a.get("pf_r0", (B, h, w, REDUCE)))
        r = ops.conv2d(r, self.res2[1], out=a.get("pf_r1", (B, h, w, REDUCE)))
        q2 = ops.scale_add(r, residual=q1, out=a.get("pf_q2", (B, h, w, REDUCE)))
        c = ops.conv2d(q2, self.cls0, out=a.get("pf_c0", (B, h, w, REDUCE)))
        c = ops.conv2d(c, self.cls3, out=a.get("pf_c3", (B, h, w, 64)))
        return logits_nchw(c, a.get("pf_pred", (B, 2, h, w)))
