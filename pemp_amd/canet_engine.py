"""CANet inference engine (reference: networks/canet.py:127-209): the [3,4,6] dilated ResNet-50 trunk, the dense comparison,
the three pre-activation residual blocks with the history channels and the ASPP, as one chain of libpemp_hip.so launches on
one stream from a static ``Arena`` (hipGraph capture works as for the other models).

Layout choices:
- layer 2's last block writes channels 0..511 and layer 3's last block channels 512..1535 of one [n,h,w,1536] buffer: the
  ``cat((f2, f3))`` of :168 is never formed;
- ``layer5`` runs once over supports and queries; eval-mode ``Dropout2d`` is the identity;
- ``layer55`` sees ``cat(query 256, z 256)`` with z constant over space, but its 3x3 dilated conv pads with ZEROS, so the z
  half is not a per-image shift: ``ops.canet_zterm`` sums, per pixel, the taps that fall inside the image (R), and the conv
  over the 256 query channels takes R as its ``residual``: relu(conv + bias + R) = relu(layer55(cat)).  PEMP_CANET_ZCAT=1
  materialises the 512-channel input instead (same function; the A/B switch of scratch/canet_bench.py);
- a residual block ``out + residual_k(out)``: ``ops.canet_block_input`` writes relu(out) (+ relu(history) into channels
  256, 257 of a 288-channel input whose channels 258..287 stay zero: the conv engine takes Cin % 32 == 0), the first conv
  runs with its ReLU, the second with ``relu=False, residual=out``;
- the history comes from a caller tensor or from row ``slot[b]`` of a device-resident table (entry.canet.Evaluator);
- ``layer7`` (256 -> 2) is packed with 62 zero output channels (Cout % 64), its two live channels copied into NCHW logits.
"""
import os
import types

import torch

from . import ops
from .engine import ASPPEngine, ResNetEngine, conv_params, with_split3
from .ops import ConvParams

MID = 256
HIST_CIN = MID + 32                     # block-1 input: 256 features + 2 history channels, zero-padded to a multiple of 32
#: PEMP_CANET_ZCAT=1: layer55 over the materialised cat(query, z) instead of the z-term path (read when an engine is built)
ZCAT = os.environ.get("PEMP_CANET_ZCAT", "0") == "1"


def feature_hw(H, W):
    """Feature size of the trunk for an H x W input: 7x7/2 stem, ceil-mode 3x3/2 max pool, layer 2's stride 2."""
    def one(v):
        v = ops.conv_out_size(v, 7, 2, 3, 1)
        v = ops._pool_out(v, 3, 2, 1, True)
        return ops.conv_out_size(v, 1, 2, 0, 1)
    return one(int(H)), one(int(W))


def _pack_padded_in(conv, cin_pad, relu):
    """[Cout, C, k, k] -> KRSC over ``cin_pad`` input channels (zero weights on the padding channels)."""
    w = conv.weight.detach().float()
    co, ci, kh, kw = w.shape
    wp = torch.zeros((co, kh, kw, cin_pad), dtype=torch.float32, device=w.device)
    wp[..., :ci] = w.permute(0, 2, 3, 1)
    return with_split3(ConvParams(wp.reshape(co, kh * kw * cin_pad).contiguous(), None, conv.bias.detach().float().contiguous(),
                                  cin_pad, co, kh, kw, 1, conv.padding[0], conv.dilation[0], kh * kw * cin_pad, False, relu))


class CANetEngine:
    """The whole eval forward: ``lowres(sup_img, sup_mask, qry_img, history, slot)`` -> logits [B,2,h,w]."""

    def __init__(self, model, arena):
        self.arena = arena
        self.use_history = bool(model.use_history)
        self.zcat = ZCAT
        self.trunk = ResNetEngine(model.encoder, arena)
        self.l5 = conv_params(model.layer5[0], None, relu=True)
        c55 = model.layer55[0]
        self.l55_q = conv_params(c55, None, relu=True, in_slice=(0, MID))
        self.l55_cat = conv_params(c55, None, relu=True) if self.zcat else None
        self.wz = ops.pack_canet_zweights(c55.weight[:, MID:])
        self.dil55 = c55.dilation[0]
        self.res = []
        for k, seq in enumerate((model.residual_1, model.residual_2, model.residual_3)):
            first = _pack_padded_in(seq[1], HIST_CIN, True) if (k == 0 and self.use_history) else conv_params(seq[1], None, relu=True)
            self.res.append((first, conv_params(seq[3], None, relu=False)))
        prm = types.SimpleNamespace(layer6=model.layer6[0], **{f"aspp_{i}": getattr(model, f"aspp_{i}") for i in range(5)})
        self.aspp = ASPPEngine(prm, arena, out_relu=True)
        l7 = model.layer7
        w = torch.zeros((64, MID), dtype=torch.float32, device=l7.weight.device)
        w[:2] = l7.weight.detach().float()[:, :, 0, 0]
        b = torch.zeros(64, dtype=torch.float32, device=l7.weight.device)
        b[:2] = l7.bias.detach().float()
        self.l7 = with_split3(ConvParams(w.contiguous(), None, b.contiguous(), MID, 64, 1, 1, 1, 0, 1, MID, False, False))

    def lowres(self, sup_img, sup_mask, qry_img, history=None, slot=None):
        """sup_img [B,S,3,H,W], sup_mask [B,S,2,H,W] (plane 0: foreground), qry_img [B,1,3,H,W] on the device.  ``history``:
        None (zeros), a [B,2,h,w] tensor, or -- with ``slot`` int32 [B] -- a table [nslots,2,h,w] read at row slot[b]."""
        a = self.arena
        B, S, ch, H, W = sup_img.shape
        ns, n = B * S, B * S + B
        x4 = a.get("x4", (n, H, W, 4))
        ops.pack_input(sup_img.reshape(ns, ch, H, W).contiguous(), out=x4[:ns])
        ops.pack_input(qry_img.reshape(B, ch, H, W).contiguous(), out=x4[ns:])
        h, w = feature_hw(H, W)
        cat23 = a.get("ca_cat23", (n, h, w, 1536))
        self.trunk.forward(x4, stage_outs={1: cat23[..., :512], 2: cat23[..., 512:]})
        f5 = ops.conv2d(cat23, self.l5, out=a.get("ca_l5", (n, h, w, MID)))
        self.last_layer5 = f5
        z = ops.canet_support_vector(f5[:ns], sup_mask.reshape(ns, 2, H, W).contiguous(), S, out=a.get("ca_z", (B, MID)))
        self.last_z = z
        if self.zcat:
            cat55 = a.get("ca_cat55", (B, h, w, 2 * MID))
            cat55[..., :MID].copy_(f5[ns:])
            cat55[..., MID:] = z.view(B, 1, 1, MID)
            out = ops.conv2d(cat55, self.l55_cat, out=a.get("ca_l55", (B, h, w, MID)))
        else:
            R = ops.canet_zterm(self.wz, z, h, w, self.dil55, out=a.get("ca_R", (B, h, w, MID)), taps=a.get("ca_T", (B, 9, MID)))
            out = ops.conv2d(f5[ns:], self.l55_q, out=a.get("ca_l55", (B, h, w, MID)), residual=R)
        self.last_layer55 = out
        for k, (c1, c2) in enumerate(self.res):
            if k == 0 and self.use_history:
                inp = a.get("ca_in_hist", (B, h, w, HIST_CIN), zero=True)       # channels 258.. stay zero
                ops.canet_block_input(out, inp, history=history, slot=slot, with_history=True)
            else:
                inp = ops.canet_block_input(out, a.get("ca_in", (B, h, w, MID)))
            t = ops.conv2d(inp, c1, out=a.get("ca_t", (B, h, w, MID)))
            out = ops.conv2d(t, c2, out=a.get(("ca_res", k), (B, h, w, MID)), residual=out, relu=False)
        self.last_aspp_in = out
        feat = self.aspp.forward(out)
        c = ops.conv2d(feat, self.l7, out=a.get("ca_l7", (B, h, w, 64)))
        pred = a.get("ca_pred", (B, 2, h, w))
        ops.resize_bilinear_ac(c[..., :2], (h, w), out=pred.permute(0, 2, 3, 1))    # NHWC -> NCHW (identity resize: exact)
        return pred
