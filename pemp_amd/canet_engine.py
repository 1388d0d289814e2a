"""CANet inference engine (reference: networks/canet.py:127-209): the [3,4,6] dilated ResNet-50 trunk, the dense comparison,
the three pre-activation residual blocks with the history channels and the ASPP, as one chain of libpemp_hip.so launches on
one stream from a static ``Arena`` (hipGraph capture works as for the other models).

Layout choices:
- layer 2's last block writes channels 0..511 and layer 3's last block channels 512..1535 of one [n,h,w,1536] buffer: the
  ``cat((f2, f3))`` of :168 is never formed;
- ``layer5`` runs once over supports and queries; eval-mode ``Dropout2d`` is the identity;
- ``layer55`` sees ``cat(query 256, z 256)`` with z constant over space, but its 3x3 dilated conv pads with ZEROS, so the z
  half is not a per-image shift: ``ops.canet_zterm`` sums, per pixel, the taps that fall inside the image (R), and the conv
  over the 256 query channels takes R as its ``residual``: relu(conv + bias + R) = relu(layer55(cat));
- a residual block ``out + residual_k(out)``: ``ops.canet_block_input`` writes relu(out) (+ relu(history) into channels
  256, 257 of a 288-channel input whose channels 258..287 stay zero: the conv engine takes Cin % 32 == 0), the first conv
  runs with its ReLU, the second with ``relu=False, residual=out``;
- the history comes from a caller tensor or from row ``slot[b]`` of a device-resident table (entry.canet.Evaluator);
- ``layer7`` (256 -> 2) is packed with 62 zero output channels (Cout % 64), its two live channels copied into NCHW logits;
- everything behind ``layer55`` is ``CANetTail``, which RPMMs runs three times behind its own prototype stage.
"""
import types

from . import ops
from .engine import ASPPEngine, ResNetEngine, classifier2, conv_params, logits_nchw, pack_episode, pack_padded_in

MID = 256
HIST_CIN = MID + 32                     # block-1 input: 256 features + 2 history channels, zero-padded to a multiple of 32


def feature_hw(H, W):
    """Feature size of the trunk for an H x W input: 7x7/2 stem, ceil-mode 3x3/2 max pool, layer 2's stride 2."""
    def one(v):
        v = ops.conv_out_size(v, 7, 2, 3, 1)
        v = ops._pool_out(v, 3, 2, 1, True)
        return ops.conv_out_size(v, 1, 2, 0, 1)
    return one(int(H)), one(int(W))


class CANetTail:
    """What follows ``layer55`` / ``layer56``: the three pre-activation residual blocks (the first one with the two history
    channels when ``use_history``), the ASPP with ``layer6`` and the 2-class classifier -> NCHW logits.  CANet runs it once,
    RPMMs once per pass (same weights, same buffers)."""

    def __init__(self, arena, residuals, aspp, layer6, classifier, use_history=True):
        self.arena, self.use_history = arena, use_history
        self.res = []
        for k, seq in enumerate(residuals):
            first = pack_padded_in(seq[1], HIST_CIN, True) if (k == 0 and use_history) else conv_params(seq[1], None, relu=True)
            self.res.append((first, conv_params(seq[3], None, relu=False)))
        prm = types.SimpleNamespace(layer6=layer6, **{f"aspp_{i}": getattr(aspp, f"aspp_{i}") for i in range(5)})
        self.aspp = ASPPEngine(prm, arena, out_relu=True)
        self.cls = classifier2(classifier)

    def forward(self, x, pred_out, history=None, slot=None):
        """x [B,h,w,256] -> ``pred_out`` [B,2,h,w].  ``history``: None (zeros), a [B,2,h,w] tensor, or -- with ``slot`` int32
        [B] -- a table [nslots,2,h,w] read at row slot[b]; not read without ``use_history``."""
        a = self.arena
        B, h, w, _ = x.shape
        out = x
        for k, (c1, c2) in enumerate(self.res):
            if k == 0 and self.use_history:
                inp = a.get("tail_in_hist", (B, h, w, HIST_CIN), zero=True)     # channels 258.. stay zero
                ops.canet_block_input(out, inp, history=history, slot=slot, with_history=True)
            else:
                inp = ops.canet_block_input(out, a.get("tail_in", (B, h, w, MID)))
            t = ops.conv2d(inp, c1, out=a.get("tail_t", (B, h, w, MID)))
            out = ops.conv2d(t, c2, out=a.get(("tail_res", k), (B, h, w, MID)), residual=out, relu=False)
        self.last_aspp_in = out
        c = ops.conv2d(self.aspp.forward(out), self.cls, out=a.get("tail_cls", (B, h, w, 64)))
        return logits_nchw(c, pred_out)


class CANetEngine:
    """The whole eval forward: ``lowres(sup_img, sup_mask, qry_img, history, slot)`` -> logits [B,2,h,w]."""
    last_aspp_in = property(lambda self: self.tail.last_aspp_in)

    def __init__(self, model, arena):
        self.arena = arena
        self.trunk = ResNetEngine(model.encoder, arena)
        self.l5 = conv_params(model.layer5[0], None, relu=True)
        c55 = model.layer55[0]
        self.l55_q = conv_params(c55, None, relu=True, in_slice=(0, MID))
        self.wz = ops.pack_canet_zweights(c55.weight[:, MID:])
        self.dil55 = c55.dilation[0]
        self.tail = CANetTail(arena, (model.residual_1, model.residual_2, model.residual_3), model, model.layer6[0], model.layer7,
                              bool(model.use_history))

    def lowres(self, sup_img, sup_mask, qry_img, history=None, slot=None):
        """sup_img [B,S,3,H,W], sup_mask [B,S,2,H,W] (plane 0: foreground), qry_img [B,1,3,H,W] on the device.  ``history``:
        None (zeros), a [B,2,h,w] tensor, or -- with ``slot`` int32 [B] -- a table [nslots,2,h,w] read at row slot[b]."""
        a = self.arena
        B, S, _, H, W = sup_img.shape
        ns, n = B * S, B * S + B
        x4 = pack_episode(a, (sup_img.flatten(0, 1), qry_img.flatten(0, 1)))
        h, w = feature_hw(H, W)
        cat23 = a.get("ca_cat23", (n, h, w, 1536))
        self.trunk.forward(x4, stage_outs={1: cat23[..., :512], 2: cat23[..., 512:]})
        f5 = ops.conv2d(cat23, self.l5, out=a.get("ca_l5", (n, h, w, MID)))
        self.last_layer5 = f5
        z = ops.canet_support_vector(f5[:ns], sup_mask.reshape(ns, 2, H, W).contiguous(), S, out=a.get("ca_z", (B, MID)))
        self.last_z = z
        R = ops.canet_zterm(self.wz, z, h, w, self.dil55, out=a.get("ca_R", (B, h, w, MID)), taps=a.get("ca_T", (B, 9, MID)))
        out = ops.conv2d(f5[ns:], self.l55_q, out=a.get("ca_l55", (B, h, w, MID)), residual=R)
        self.last_layer55 = out
        return self.tail.forward(out, a.get("ca_pred", (B, 2, h, w)), history, slot)
